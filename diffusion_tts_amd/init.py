"""Random-init weights for the hot-path networks, as flat state dicts with the reference's key names.

BASELINE prescribes random-init weights (no checkpoints travel).  The draws follow the reference
constructors' order on the torch global CPU generator, so `edm_state_dict(cfg, seed)` equals
`EDMPrecond(...).state_dict()` built under `torch.manual_seed(seed)` parameter for parameter
(edm/training/networks.py:19-24 weight_init, :31-37 Linear, :50-66 Conv2d, :135-164 UNetBlock,
:230-318 SongUNet, :373-433 DhariwalUNet), and `classifier_state_dict` equals the random-init
`EncoderUNetModel` of edm/unet.py:708-870 (torch.nn default initialisers).

`refill_degenerate` implements the weight rule of SURVEY.md section 8(d): a freshly constructed ADM
denoiser has every residual-branch output conv zero-initialised (networks.py:392), so F_x == 0 and the
U-Net would be numerically invisible; every parameter whose max-abs is < 1e-4 is re-drawn.
"""
import math
from collections import OrderedDict

import numpy as np
import torch

from .config import EDMConfig, ClassifierConfig, edm_blocks, classifier_layers


def _winit(shape, mode, fan_in, fan_out):
    if mode == 'xavier_uniform':
        return np.sqrt(6 / (fan_in + fan_out)) * (torch.rand(*shape) * 2 - 1)
    if mode == 'kaiming_uniform':
        return np.sqrt(3 / fan_in) * (torch.rand(*shape) * 2 - 1)
    if mode == 'kaiming_normal':
        return np.sqrt(1 / fan_in) * torch.randn(*shape)
    raise ValueError(mode)


class _Builder:
    def __init__(self):
        self.sd = OrderedDict()

    def linear(self, name, fin, fout, bias=True, mode='kaiming_normal', w=1, b=0):
        self.sd[f'{name}.weight'] = _winit([fout, fin], mode, fin, fout) * w
        if bias:
            self.sd[f'{name}.bias'] = _winit([fout], mode, fin, fout) * b

    def conv(self, name, cin, cout, k, mode='kaiming_normal', w=1, b=0, resample_filter=None):
        if k:
            self.sd[f'{name}.weight'] = _winit([cout, cin, k, k], mode, cin * k * k, cout * k * k) * w
            self.sd[f'{name}.bias'] = _winit([cout], mode, cin * k * k, cout * k * k) * b
        if resample_filter is not None:            # the buffer of an up / down Conv2d (networks.py:64-66), after its parameters
            self.sd[f'{name}.resample_filter'] = resample_filter_2d(resample_filter)

    def norm(self, name, c):
        self.sd[f'{name}.weight'] = torch.ones(c)
        self.sd[f'{name}.bias'] = torch.zeros(c)


def resample_filter_2d(taps):
    """the `resample_filter` buffer of a reference Conv2d (networks.py:64-65): outer(f, f) / sum(f)^2, float32 [1, 1, k, k]"""
    f = torch.as_tensor(list(taps), dtype=torch.float32)
    return f.ger(f).unsqueeze(0).unsqueeze(1) / f.sum().square()


def vp_sigma_range(beta_d=19.9, beta_min=0.1, epsilon_t=1e-5):
    """(sigma_min, sigma_max) of a VPPrecond (networks.py:491-492, 511-513): float(sigma(epsilon_t)), float(sigma(1)) with sigma(t) evaluated
    on a default-dtype (float32) scalar tensor, as `torch.as_tensor(<python number>)` makes it"""
    def sigma(t):
        t = torch.as_tensor(t, dtype=torch.float32)
        return ((0.5 * beta_d * (t ** 2) + beta_min * t).exp() - 1).sqrt()
    return float(sigma(epsilon_t)), float(sigma(1.0))


def iddpm_u(M=1000, C_1=0.001, C_2=0.008):
    """The `u` buffer of an iDDPMPrecond (networks.py:594-597, 617-619): the noise levels of the M + 1 DDPM timesteps, u[M] = 0, built
    backwards in float32 -- alpha_bar(j) = sin(pi/2 * j / M / (C_2 + 1))^2 on an integer tensor times a Python float, i.e. in float32 --
    with the reference's own sequence of tensor operations, so the table is the constructor's bit for bit on the same host (a float32 sine is
    not rounded alike by every CPU's vector library: a checkpoint's table is the file's own, never this one)."""
    def alpha_bar(j):
        j = torch.as_tensor(j)
        return (0.5 * np.pi * j / M / (C_2 + 1)).sin() ** 2
    u = torch.zeros(M + 1)
    for j in range(M, 0, -1):
        u[j - 1] = ((u[j] ** 2 + 1) / (alpha_bar(j - 1) / alpha_bar(j)).clip(min=C_1) - 1).sqrt()
    return u


def edm_state_dict(cfg: EDMConfig, seed: int = 0, prefix: str = 'model.'):
    """Parameters of the reference constructor, draw for draw.  With the NCSN++ options the buffers travel too, in state_dict() order: the
    Fourier embedding's `map_noise.freqs` is a random draw the network needs (networks.py:215), and the [1, 3, 3, 1] `resample_filter`s are
    what checkpoint.load_edm_pickle checks a file's filter by.  (The DDPM++ dict keeps its historical form: parameters only.)
    The VP and VE wrappers add nothing to the denoiser's draws; iDDPM (cfg.precond == 'iddpm') draws the last convolution with
    2 * img_channels outputs (networks.py:592) and carries the wrapper's own `u` buffer, first in the dict and without `prefix`, as in
    state_dict() order (a module's buffers precede its children)."""
    torch.manual_seed(seed)
    adm = cfg.arch == 'adm'
    mc, emb = cfg.model_channels, cfg.emb_channels
    B = _Builder()
    if adm:
        init = dict(mode='kaiming_uniform', w=np.sqrt(1 / 3), b=np.sqrt(1 / 3))
        zero = dict(mode='kaiming_uniform', w=0, b=0)
        attn = init
        if cfg.augment_dim:
            B.linear('map_augment', cfg.augment_dim, mc, bias=False, **zero)
        B.linear('map_layer0', mc, emb, **init)
        B.linear('map_layer1', emb, emb, **init)
        if cfg.label_dim:
            B.linear('map_label', cfg.label_dim, emb, bias=False, mode='kaiming_normal', w=np.sqrt(cfg.label_dim))
    else:
        init = dict(mode='xavier_uniform', w=1, b=0)
        zero = dict(mode='xavier_uniform', w=1e-5, b=0)
        attn = dict(mode='xavier_uniform', w=np.sqrt(0.2), b=0)
        nc = cfg.noise_channels
        if cfg.embedding_type == 'fourier':
            B.sd['map_noise.freqs'] = torch.randn(nc // 2) * 16         # FourierEmbedding.__init__, networks.py:213-215
        if cfg.label_dim:
            B.linear('map_label', cfg.label_dim, nc, **init)
        if cfg.augment_dim:
            B.linear('map_augment', cfg.augment_dim, nc, bias=False, **init)
        B.linear('map_layer0', nc, emb, **init)
        B.linear('map_layer1', emb, emb, **init)
    enc, dec, cfin = edm_blocks(cfg)
    filt = list(cfg.resample_filter) if cfg.fir else None
    for blk in enc + dec:
        n = blk.name
        rf = filt if (blk.up or blk.down) else None
        if blk.kind == 'conv':
            B.conv(n, blk.cin, blk.cout, 3, **init)
            continue
        if blk.kind == 'aux_residual':
            B.conv(n, blk.cin, blk.cout, 3, resample_filter=rf, **init)
            continue
        B.norm(f'{n}.norm0', blk.cin)
        B.conv(f'{n}.conv0', blk.cin, blk.cout, 3, resample_filter=rf, **init)
        B.linear(f'{n}.affine', emb, blk.cout * (2 if adm else 1), **init)
        B.norm(f'{n}.norm1', blk.cout)
        B.conv(f'{n}.conv1', blk.cout, blk.cout, 3, **zero)
        if blk.cin != blk.cout or blk.up or blk.down:
            k = 1 if ((not adm) or blk.cin != blk.cout) else 0      # resample_proj=True only for SongUNet
            B.conv(f'{n}.skip', blk.cin, blk.cout, k, resample_filter=rf, **init)
        if blk.heads:
            B.norm(f'{n}.norm2', blk.cout)
            B.conv(f'{n}.qkv', blk.cout, blk.cout * 3, 1, **attn)
            B.conv(f'{n}.proj', blk.cout, blk.cout, 1, **zero)
    r = cfg.img_resolution
    if adm:
        B.norm('out_norm', cfin)
        B.conv('out_conv', cfin, cfg.out_channels, 3, **zero)
    else:
        B.norm(f'dec.{r}x{r}_aux_norm', cfin)
        B.conv(f'dec.{r}x{r}_aux_conv', cfin, cfg.out_channels, 3, **zero)
    out = OrderedDict()
    if cfg.precond == 'iddpm':
        out['u'] = iddpm_u(cfg.M, cfg.C_1, cfg.C_2)
    out.update((prefix + k, v.to(torch.float32)) for k, v in B.sd.items())
    return out


def classifier_state_dict(cfg: ClassifierConfig, seed: int = 1):
    """Random-init EncoderUNetModel(pool='attention', use_scale_shift_norm, resblock_updown) parameters.
    torch.nn modules are instantiated (and discarded) in the reference's construction order so the
    default initialisers consume the generator identically."""
    nn = torch.nn
    torch.manual_seed(seed)
    sd = OrderedDict()

    def take(prefix, mod, zero=False):
        for k, v in mod.named_parameters():
            sd[f'{prefix}.{k}'] = (torch.zeros_like(v) if zero else v.detach().clone())

    mc = cfg.model_channels
    emb = mc * 4
    take('time_embed.0', nn.Linear(mc, emb))
    take('time_embed.2', nn.Linear(emb, emb))
    layers, ch, res = classifier_layers(cfg)
    for L in layers:
        p = L.prefix
        if L.kind == 'conv_in':
            take(p, nn.Conv2d(L.cin, L.cout, 3, padding=1))
        elif L.kind == 'res':
            take(f'{p}.in_layers.0', nn.GroupNorm(32, L.cin))
            take(f'{p}.in_layers.2', nn.Conv2d(L.cin, L.cout, 3, padding=1))
            take(f'{p}.emb_layers.1', nn.Linear(emb, 2 * L.cout))
            take(f'{p}.out_layers.0', nn.GroupNorm(32, L.cout))
            take(f'{p}.out_layers.3', nn.Conv2d(L.cout, L.cout, 3, padding=1), zero=True)
            if L.cin != L.cout:
                take(f'{p}.skip_connection', nn.Conv2d(L.cin, L.cout, 1))
        else:
            take(f'{p}.norm', nn.GroupNorm(32, L.cin))
            take(f'{p}.qkv', nn.Conv1d(L.cin, 3 * L.cin, 1))
            take(f'{p}.proj_out', nn.Conv1d(L.cin, L.cin, 1), zero=True)
    take('out.0', nn.GroupNorm(32, ch))
    sd['out.2.positional_embedding'] = torch.randn(ch, res ** 2 + 1) / ch ** 0.5
    take('out.2.qkv_proj', nn.Conv1d(ch, 3 * ch, 1))
    take('out.2.c_proj', nn.Conv1d(ch, cfg.out_channels, 1))
    return sd


HEAD_SCALE_DECIDABLE = 20.0


def scale_classifier_head(sd, head_scale: float = HEAD_SCALE_DECIDABLE):
    """The second, documented classifier fixture: the same constructor draws and seeds, with the output head
    (AttentionPool2d.c_proj, edm/unet.py:61-69) multiplied by `head_scale`, so that the 1000 logits of the random-init classifier have
    a standard deviation of ~3.4 (0.17 x 20) like a trained classifier's instead of 0.17, and the target-class probability of two
    candidates differs by per cent instead of by 1e-4 relative.  Used alike by the oracle and the build (it is a state dict)."""
    out = OrderedDict(sd)
    for k in ('out.2.c_proj.weight', 'out.2.c_proj.bias'):
        out[k] = sd[k] * head_scale
    return out


def refill_degenerate(sd, seed: int, threshold: float = 1e-4):
    """SURVEY.md 8(d) weight rule.  Parameters with max|.| < threshold are re-drawn, in dict order, from
    torch.Generator().manual_seed(seed + 1): tensors with >= 2 dims as U(-b, b), b = sqrt(3 / fan_in),
    fan_in = prod(shape[1:]); 1-D tensors (biases) as U(-0.1, 0.1).  Returns (new dict, refilled names)."""
    g = torch.Generator().manual_seed(seed + 1)
    out, names = OrderedDict(), []
    for k, v in sd.items():
        if v.numel() and float(v.abs().max()) < threshold:
            u = torch.rand(v.shape, generator=g, dtype=torch.float32) * 2 - 1
            if v.dim() >= 2:
                fan_in = int(np.prod(v.shape[1:]))
                v = u * math.sqrt(3.0 / fan_in)
            else:
                v = u * 0.1
            names.append(k)
        out[k] = v
    return out, names


def checksum(sd):
    """Order-sensitive fingerprint of a state dict: (sum, sum|.|, numel) in float64."""
    s = a = 0.0
    n = 0
    for v in sd.values():
        v64 = v.double()
        s += float(v64.sum())
        a += float(v64.abs().sum())
        n += v.numel()
    return dict(sum=s, abs_sum=a, numel=n)


class _DiffusersBuilder:
    """The seeded initialiser behind vae_decoder_state_dict and sd_unet_state_dict: every tensor is one draw of a generator of its own, in
    call order (the goldens were made from these state dicts: the order of the draws is the contract).  Fan-in scaled weights, small biases,
    norms near identity.  Keys in construction order."""

    def __init__(self, seed):
        self.g, self.sd = torch.Generator().manual_seed(seed), OrderedDict()

    def conv(self, key, cout, cin, k, gain=1.0):
        self.sd[key + '.weight'] = torch.randn(cout, cin, k, k, generator=self.g) * (gain / math.sqrt(cin * k * k))
        self.sd[key + '.bias'] = torch.randn(cout, generator=self.g) * 0.05

    def lin(self, key, cout, cin, gain=1.0, bias=True):
        self.sd[key + '.weight'] = torch.randn(cout, cin, generator=self.g) * (gain / math.sqrt(cin))
        if bias:
            self.sd[key + '.bias'] = torch.randn(cout, generator=self.g) * 0.05

    def norm(self, key, c):
        self.sd[key + '.weight'] = 1.0 + 0.1 * torch.randn(c, generator=self.g)
        self.sd[key + '.bias'] = 0.1 * torch.randn(c, generator=self.g)

    def resnet(self, key, cin, cout, temb=None):
        """ResnetBlock2D; temb: the width of the time embedding its time_emb_proj reads (None: a block without one, the VAE's)"""
        self.norm(key + '.norm1', cin); self.conv(key + '.conv1', cout, cin, 3)
        if temb is not None:
            self.lin(key + '.time_emb_proj', cout, temb, gain=1.5)
        self.norm(key + '.norm2', cout); self.conv(key + '.conv2', cout, cout, 3, gain=0.5)
        if cin != cout:
            self.conv(key + '.conv_shortcut', cout, cin, 1)


def vae_decoder_state_dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, seed=0):
    """Random-init parameters of the SD VAE *decoder* (+ post_quant_conv) under diffusers' key names
    (sd/diffusers/src/diffusers/models/autoencoders/vae.py:204-279, autoencoder_kl.py:105-110): BASELINE config 4 prescribes
    random-init weights (SD-1.5's cannot be fetched).  Own seeded initialiser, fan-in scaled so activations stay O(1) through the
    17 residual blocks; norms near identity.  Keys in construction order."""
    b = _DiffusersBuilder(seed)
    conv, lin, norm, resnet = b.conv, b.lin, b.norm, b.resnet
    top = block_out_channels[-1]
    conv('post_quant_conv', latent_channels, latent_channels, 1)
    conv('decoder.conv_in', top, latent_channels, 3)
    resnet('decoder.mid_block.resnets.0', top, top)
    a = 'decoder.mid_block.attentions.0'
    norm(a + '.group_norm', top)
    for n in ('to_q', 'to_k', 'to_v'):
        lin(a + '.' + n, top, top)
    lin(a + '.to_out.0', top, top, gain=0.5)
    resnet('decoder.mid_block.resnets.1', top, top)
    rev = list(reversed(block_out_channels))
    prev = rev[0]
    for i, c in enumerate(rev):
        for j in range(layers_per_block + 1):
            resnet(f'decoder.up_blocks.{i}.resnets.{j}', prev if j == 0 else c, c)
        if i != len(rev) - 1:
            conv(f'decoder.up_blocks.{i}.upsamplers.0.conv', c, c, 3)
        prev = c
    norm('decoder.conv_norm_out', block_out_channels[0])
    conv('decoder.conv_out', 3, block_out_channels[0], 3)
    return b.sd


def sd_unet_state_dict(block_out_channels=(320, 640, 1280, 1280), heads=8, cross_attention_dim=768, layers_per_block=2, seed=0):
    """Random-init parameters of the SD-1.x U-Net under diffusers' key names and shapes (`UNet2DConditionModel.state_dict()`,
    sd/diffusers/src/diffusers/models/unets/unet_2d_condition.py; 686 tensors at SD-1.5's size): BASELINE config 4 prescribes random-init
    weights (SD-1.5's cannot be fetched).  Own seeded initialiser, fan-in scaled so that activations stay O(1) through the 22 residual and
    16 transformer blocks.  The gains of the time-embedding path (time_embedding.*, time_emb_proj) and of the text path (attn2: peaked
    softmax over the tokens, full-gain output projection) are raised so that the output DEPENDS on the timestep and on the context by
    far more than a 16-bit pipeline's error -- a golden test could not otherwise tell a model that ignores them
    (tests/golden/make_golden_sd_unet.py asserts the margins).  `heads`: diffusers' `attention_head_dim` of SD-1.x, i.e. the number of
    heads of every transformer block.  Keys in construction order."""
    b = _DiffusersBuilder(seed)
    conv, lin, norm = b.conv, b.lin, b.norm
    boc = tuple(block_out_channels)
    temb = 4 * boc[0]
    resnet = lambda key, cin, cout: b.resnet(key, cin, cout, temb=temb)

    def transformer(key, c):
        norm(key + '.norm', c)
        conv(key + '.proj_in', c, c, 1)
        t = key + '.transformer_blocks.0'
        norm(t + '.norm1', c)
        for n in ('to_q', 'to_k', 'to_v'):
            lin(f'{t}.attn1.{n}', c, c, bias=False)
        lin(t + '.attn1.to_out.0', c, c, gain=0.5)
        norm(t + '.norm2', c)
        lin(t + '.attn2.to_q', c, c, gain=2.0, bias=False)
        lin(t + '.attn2.to_k', c, cross_attention_dim, gain=2.0, bias=False)
        lin(t + '.attn2.to_v', c, cross_attention_dim, bias=False)
        lin(t + '.attn2.to_out.0', c, c, gain=1.0)
        norm(t + '.norm3', c)
        lin(t + '.ff.net.0.proj', 8 * c, c)
        lin(t + '.ff.net.2', c, 4 * c, gain=0.5)
        conv(key + '.proj_out', c, c, 1, gain=0.5)

    conv('conv_in', boc[0], 4, 3)
    lin('time_embedding.linear_1', temb, boc[0], gain=2.0)
    lin('time_embedding.linear_2', temb, temb, gain=2.0)
    skips = [boc[0]]
    prev = boc[0]
    for i, c in enumerate(boc):
        last = i == len(boc) - 1
        for j in range(layers_per_block):
            resnet(f'down_blocks.{i}.resnets.{j}', prev, c)
            if not last:
                transformer(f'down_blocks.{i}.attentions.{j}', c)
            prev = c
            skips.append(c)
        if not last:
            conv(f'down_blocks.{i}.downsamplers.0.conv', c, c, 3)
            skips.append(c)
    top = boc[-1]
    resnet('mid_block.resnets.0', top, top)
    transformer('mid_block.attentions.0', top)
    resnet('mid_block.resnets.1', top, top)
    for i, c in enumerate(boc[::-1]):
        for j in range(layers_per_block + 1):
            resnet(f'up_blocks.{i}.resnets.{j}', prev + skips.pop(), c)
            if i != 0:
                transformer(f'up_blocks.{i}.attentions.{j}', c)
            prev = c
        if i != len(boc) - 1:
            conv(f'up_blocks.{i}.upsamplers.0.conv', c, c, 3)
    norm('conv_norm_out', boc[0])
    conv('conv_out', 4, boc[0], 3)
    return b.sd
