"""What the four checkpoint-format networks (vae.VAEDecoder, sd_unet.SDUNet, clip_vision.CLIPVisionTower, clip_text.CLIPTextTower) share on
the way from a stock diffusers / transformers state dict to a launch sequence on the HIP kernels:
  Params                         f32 upload, norm pairs, conv / Linear weights packed for dts_conv2d (zero-padded where asked), stacked q | k | v
  resnet_params, resnet          diffusers' ResnetBlock2D (resnet.py), with or without the time-embedding addend and the concatenated skip
  clip_layers, clip_encoder      transformers' CLIPEncoderLayer (modeling_clip.py); the attention call is the tower's own
  clip_encoder_x3                the same layer in the split-precision mode (both towers' parity-grade forms; the text tower passes its masked attention)
  clip_config_errors, clip_section, clip_files, diffusers_weights, read_tensors, check_shapes, require_gpu
                                 the refusals and the file reading: every network names what it does not take, none guesses
Kernels are called through the module (`ops.conv2d(...)`, never a name imported from it): the tools under tools/ time a forward by replacing
attributes of `ops`.  networks.py and classifier.py (EDM's own key naming, out_perm, the f16x3 mode) share nothing of this.
"""
import json
import os
import types

import torch

from . import ops


def require_gpu(name):
    if not torch.cuda.is_available():
        raise RuntimeError(f'{name} (HIP) needs a GPU: there is no CPU fallback in this package')


# ---- parameters ----------------------------------------------------------------------------------
def stack_qkv(sd, key, names=('q_proj', 'k_proj', 'v_proj')):
    """(weight [3C, C], bias [3C] or None) of one projection whose output is q | k | v blocks, from `key`.{names}.{weight,bias}"""
    w = torch.cat([sd[f'{key}.{n}.weight'] for n in names], 0)
    b = torch.cat([sd[f'{key}.{n}.bias'] for n in names], 0) if f'{key}.{names[0]}.bias' in sd else None
    return w, b


class Params:
    """state-dict tensors -> what the kernels read, on `device`: float32 vectors and weights packed in the activation `dtype`"""

    def __init__(self, device, dtype):
        self.device, self.dtype = device, dtype

    def f32(self, t):
        return t.detach().to(self.device, torch.float32).contiguous()

    def norm(self, sd, key):
        return self.f32(sd[key + '.weight']), self.f32(sd[key + '.bias'])

    def pack(self, w, b=None, pad_in=None, pad_out=None):
        """f32 weight [O, I] / [O, I, k, k] (+ bias) on the device -> (packed [O][k][k][I] in the activation dtype, f32 bias or None).
        A Linear is a 1x1 conv; pad_in / pad_out: zero input / output channels (and bias entries) up to the MFMA granule."""
        if w.dim() == 2:
            w = w[:, :, None, None]
        if pad_in is not None and w.shape[1] < pad_in:
            w = torch.cat([w, torch.zeros(w.shape[0], pad_in - w.shape[1], *w.shape[2:], device=w.device)], 1)
        if pad_out is not None and w.shape[0] < pad_out:
            w = torch.cat([w, torch.zeros(pad_out - w.shape[0], *w.shape[1:], device=w.device)], 0)
            if b is not None:
                b = torch.cat([b, torch.zeros(pad_out - b.shape[0], device=b.device)])
        return ops.pack_conv_weight(w.contiguous(), self.dtype), (None if b is None else b.contiguous())

    def conv(self, sd, key, **pad):
        return self.pack(self.f32(sd[key + '.weight']), self.f32(sd[key + '.bias']), **pad)

    def qkv(self, sd, key, names=('q_proj', 'k_proj', 'v_proj')):
        w, b = stack_qkv(sd, key, names)
        return self.pack(self.f32(w), None if b is None else self.f32(b))


# ---- ResnetBlock2D -------------------------------------------------------------------------------
def resnet_params(params, sd, key):
    P = types.SimpleNamespace()
    P.g1, P.b1 = params.norm(sd, key + '.norm1')
    P.w1, P.c1 = params.conv(sd, key + '.conv1')
    P.g2, P.b2 = params.norm(sd, key + '.norm2')
    P.w2, P.c2 = params.conv(sd, key + '.conv2')
    P.ws, P.cs = params.conv(sd, key + '.conv_shortcut') if key + '.conv_shortcut.weight' in sd else (None, None)
    return P


def resnet(x, P, groups, eps, bias_nc=None, skip=None):
    """ResnetBlock2D.forward (resnet.py): norm1-silu-conv1 (+ bias_nc, time_emb_proj(silu(emb)) per sample and channel)-norm2-silu-conv2,
    + the input or its 1x1 shortcut.  skip: the second half of the up blocks' torch.cat([x, skip], 1), read in place."""
    h = ops.group_norm(x, groups, eps, P.g1, P.b1, x2=skip, silu=True)
    h = ops.conv2d(h, P.w1, P.c1, bias_nc=bias_nc, gn_stats=True)
    h = ops.group_norm(h, groups, eps, P.g2, P.b2, silu=True)
    if P.ws is not None:
        sk = ops.conv2d(x, P.ws, P.cs, x2=skip)
    elif skip is None:
        sk = x
    else:
        raise ValueError('SDUNet: a resnet over concatenated inputs needs its conv_shortcut')
    return ops.conv2d(h, P.w2, P.c2, residual=sk, gn_stats=True)


# ---- CLIPEncoderLayer ----------------------------------------------------------------------------
def clip_layers(params, sd, prefix, n_layers):
    """the parameters of `prefix`encoder.layers.0 .. n_layers - 1, q_proj | k_proj | v_proj stacked into one projection"""
    layers = []
    for i in range(n_layers):
        key = f'{prefix}encoder.layers.{i}'
        P = types.SimpleNamespace(ln1=params.norm(sd, key + '.layer_norm1'), ln2=params.norm(sd, key + '.layer_norm2'))
        P.w_qkv, P.b_qkv = params.qkv(sd, key + '.self_attn')
        P.w_o, P.b_o = params.conv(sd, key + '.self_attn.out_proj')
        P.w_fc1, P.b_fc1 = params.conv(sd, key + '.mlp.fc1')
        P.w_fc2, P.b_fc2 = params.conv(sd, key + '.mlp.fc2')
        layers.append(P)
    return layers


def clip_encoder(h, layers, eps, act, attend):
    """h [n, t, 1, C] through the layers; attend(qkv [n, t, 3C]) -> [n, t, C] is the tower's attention (plain, or causal with key lengths)"""
    n, t, _, C = h.shape
    for P in layers:
        # CLIPEncoderLayer.forward: x + out_proj(attention(layer_norm1(x))), then x + fc2(act(fc1(layer_norm2(x))))
        y = ops.layer_norm(h, *P.ln1, eps=eps)
        qkv = ops.conv2d(y, P.w_qkv, P.b_qkv)
        a = attend(qkv.view(n, t, 3 * C))
        h = ops.conv2d(a.view(n, t, 1, C), P.w_o, P.b_o, residual=h)
        y = ops.layer_norm(h, *P.ln2, eps=eps)
        f = ops.conv2d(y, P.w_fc1, P.b_fc1)
        ops.gelu(f, act, out=f)
        h = ops.conv2d(f, P.w_fc2, P.b_fc2, residual=h)
    return h


def clip_encoder_x3(h, layers, eps, act, heads, scale, attend=None):
    """clip_encoder in the split-precision mode (ops.F16X3; the layers' weights are X3Weights): the residual stream h [n, t, 1, C] is float32
    throughout, and every operand of a projection is written as its image by the kernel that produces it (layer_norm_x3, gelu_x3 and, where
    ops.attention_x3_ok, the qkv projection's and the attention's own epilogues) -- no float32 tensor exists between them, no split pass runs.
    attend None (the vision tower): plain attention, d = 64 at t >= 128 on the split-precision kernel, every other shape on the float32 one.
    attend a callable (the text tower: ops.attention_x3_masked with its mask, split_out=True): it receives the qkv projection's SplitQKV
    [n, t, 3C] and returns the proj convolution's SplitAct; the fused images are then used whatever t is (the qkv epilogue takes any pixel
    count, so no dts_split2_f16 pass is needed for the short sequences either) and ops.attention_x3_ok is not asked."""
    n, t, _, C = h.shape
    fuse = attend is not None or ops.attention_x3_ok(t, C // heads)
    for P in layers:
        y = ops.layer_norm_x3(h, *P.ln1, eps=eps)
        qkv = ops.conv2d(y, P.w_qkv, P.b_qkv, out_split2=fuse)
        if attend is not None:
            a = attend(qkv.view(n, t, 3 * C))
        else:
            a = ops.attention(qkv.view(n, t, 3 * C), heads, scale, x3=True, split_out=fuse)
        h = ops.conv2d(a if fuse else a.view(n, t, 1, C), P.w_o, P.b_o, residual=h)
        y = ops.layer_norm_x3(h, *P.ln2, eps=eps)
        f = ops.conv2d(y, P.w_fc1, P.b_fc1)
        h = ops.conv2d(ops.gelu_x3(f, act), P.w_fc2, P.b_fc2, residual=h)
    return h


# ---- configuration and files ---------------------------------------------------------------------
def clip_config_errors(dtype, hidden_size, num_attention_heads, intermediate_size, hidden_act, projection_dim, head_dims, head_kernel,
                       split_precision=False):
    """the settings of a CLIP tower that this build's kernels do not take, each with its value: the clauses both towers share.  head_dims:
    the head dims of the tower's attention kernel, head_kernel: how the message names them.  split_precision: the check of the tower's ops.F16X3
    form (clip_vision.CLIPVisionTowerX3, clip_text.CLIPTextTowerX3)."""
    bad = []
    if split_precision:
        if not (isinstance(dtype, str) and dtype == ops.F16X3):
            bad.append(f'dtype={dtype} ({ops.F16X3} is the split-precision tower\'s only dtype: there is no float32 form of this tower, '
                       f'and float16 / bfloat16 are the 16-bit tower\'s)')
    elif dtype not in (torch.float16, torch.bfloat16):
        bad.append(f'dtype={dtype} (float16 or bfloat16: there is no float32 form of this tower)')
    if hidden_size <= 0 or hidden_size % 64:
        bad.append(f'hidden_size={hidden_size} is not a multiple of 64 (the channel granularity of dts_conv2d)')
    if hidden_size > 2048:
        bad.append(f'hidden_size={hidden_size} exceeds 2048 (the row dts_layer_norm holds in registers)')
    if num_attention_heads <= 0 or hidden_size % num_attention_heads or hidden_size // num_attention_heads not in head_dims:
        hd = hidden_size / num_attention_heads if num_attention_heads > 0 else float('nan')
        bad.append(f'head dim {hd:g} (hidden_size={hidden_size} / num_attention_heads={num_attention_heads}) is not {head_kernel}')
    if intermediate_size <= 0 or intermediate_size % 64:
        bad.append(f'intermediate_size={intermediate_size} is not a multiple of 64')
    if hidden_act not in ops.GELU_KINDS:
        bad.append(f'hidden_act={hidden_act!r} (dts_gelu computes {sorted(ops.GELU_KINDS)})')
    if projection_dim is not None and projection_dim <= 0:
        bad.append(f'projection_dim={projection_dim}')
    return bad


def clip_section(cfg, section, defaults):
    """the settings named by `defaults` of a CLIP config.json dict: from its nested `section` (a CLIPModel's) or from the dict itself (a
    single tower's own), absent keys taking the defaults; projection_dim is the top-level one of a CLIPModel (the shape of its projection)"""
    sc = cfg.get(section) or cfg
    out = {k: sc.get(k, d) for k, d in defaults.items()}
    if section in cfg and 'projection_dim' in cfg:
        out['projection_dim'] = cfg['projection_dim']
    return out


def clip_files(path):
    """(config.json as a dict, the path of model.safetensors) of a local directory that `save_pretrained` wrote"""
    cfg_file, st_file = os.path.join(path, 'config.json'), os.path.join(path, 'model.safetensors')
    if not os.path.exists(cfg_file):
        raise FileNotFoundError(f'{path}: no config.json')
    if not os.path.exists(st_file):
        raise FileNotFoundError(f'{path}: no model.safetensors (a .bin pickle is not read: convert it to safetensors)')
    with open(cfg_file) as f:
        return json.load(f), st_file


def diffusers_weights(path):
    """the parameter file of a diffusers model directory"""
    for n in ('diffusion_pytorch_model.safetensors', 'diffusion_pytorch_model.fp16.safetensors'):
        if os.path.exists(os.path.join(path, n)):
            return os.path.join(path, n)
    raise FileNotFoundError(f'{path}: no diffusion_pytorch_model[.fp16].safetensors (a .bin pickle is not read: convert it to safetensors)')


def read_tensors(file, keep, what=None):
    """{name: host tensor} of a safetensors file.  keep(stored keys) -> {stored key: name to store it under}: a key it leaves out is never
    read (tensors load lazily, so the other half of a checkpoint stays on disk).  what: refuse a file that yields nothing, by this name."""
    import safetensors
    with safetensors.safe_open(file, framework='pt', device='cpu') as f:
        sd = {name: f.get_tensor(k) for k, name in keep(list(f.keys())).items()}
    if what and not sd:
        raise ValueError(f'{file}: no {what} tensors')
    return sd


def check_shapes(name, sd, want, absent_text, settings_text):
    """the parameters must be those of the configuration the object was given: a mismatch is named here, not met as a reshape error.
    want: {key: shape}; absent_text / settings_text: the settings a missing key / a wrong shape is held against, as the message spells them."""
    for key, shape in want.items():
        if key not in sd:
            raise ValueError(f'{name}: the state dict has no {key!r} ({absent_text})')
        if tuple(sd[key].shape) != shape:
            raise ValueError(f'{name}: {key} has shape {tuple(sd[key].shape)}, but {settings_text} ask for {shape}')
