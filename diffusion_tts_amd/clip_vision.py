"""The image tower of CLIP on the HIP kernels: drop-in for `CLIPModel.get_image_features(pixel_values=...)` in the scorer of the SD
search loop (scorers.CLIPScorer, sd/scorers.py:175-183 of the reference), i.e. for CLIPVisionTransformer.forward + visual_projection of
transformers (models/clip/modeling_clip.py: CLIPVisionEmbeddings, CLIPEncoderLayer, CLIPAttention, CLIPMLP).

Every decoded candidate of a search passes through these 24 layers at 257 tokens (ViT-L/14); here they run on this build's kernels:
  patch embedding Conv2d(3, hidden, p, stride p) -> dts_patchify (patch rows) + one 1x1 dts_conv2d (weight flattened, zero-padded to 64 columns)
  class token + position table               -> dts_vit_tokens
  pre_layrnorm, layer_norm1 / 2              -> dts_layer_norm
  q_proj | k_proj | v_proj                   -> ONE 1x1 dts_conv2d (rows and biases stacked at load time)
  softmax(q k^T / sqrt d) v                  -> dts_attention
  out_proj, fc2                              -> 1x1 dts_conv2d with the bias and the residual add in the epilogue
  fc1 + activation                           -> 1x1 dts_conv2d + dts_gelu (quick-GELU or erf GELU, in place)
  post_layernorm(token 0), visual_projection -> dts_vit_head + dts_linear (f32)
Activations are [n, tokens, 1, channels] in `dtype`.  float16 / bfloat16: a 16-bit THROUGHPUT mode of the scorer (the reference scores in
float32).  CLIPVisionTowerX3 (dtype ops.F16X3, 'f16x3'): the PARITY-GRADE mode -- float32 activations, every matrix product in split precision on the 16-bit matrix
cores (dts_conv2d in DTS_F16X3; dts_attention_x3 at head dim 64 and >= 128 tokens, the float32 dts_attention otherwise), and between them
the float32 forms of the kernels above, which write the next product's operand image themselves:
  patch rows -> dts_patchify_x3; tokens -> dts_vit_tokens_f32; pre_layrnorm, layer_norm1 / 2 -> dts_layer_norm_x3; activation -> dts_gelu_x3;
  head -> dts_vit_head_f32 + dts_linear
It is held to the float32 module's own distance from float64 (tests/test_gpu_clip_vision_x3.py).  torch.float32 itself is refused: there is
no float32 matrix-instruction form of this tower.  CLIPVisionTower itself keeps refusing every dtype but the two 16-bit ones, 'f16x3'
included: the split-precision mode is a class of its own, as its kernels are entry points of their own.

Parameters: a state dict with transformers' key names (`vision_model.*`, `visual_projection.weight`).  Shapes the kernels do not take are
refused by name at construction (check_config).  The forward makes no device-to-host synchronisation and no data-dependent step.
"""
import types

import torch

from . import blocks, ops
from .blocks import stack_qkv       # noqa: F401  (the rule lives in blocks; tests and callers read it here)

PREFIX = 'vision_model.'
PROJECTION = 'visual_projection.weight'
# transformers' CLIPVisionConfig defaults: config.json stores only what differs from them
CONFIG_DEFAULTS = {'hidden_size': 768, 'intermediate_size': 3072, 'num_hidden_layers': 12, 'num_attention_heads': 12, 'image_size': 224,
                   'patch_size': 32, 'hidden_act': 'quick_gelu', 'layer_norm_eps': 1e-5, 'projection_dim': 512}


def check_config(hidden_size, num_attention_heads, intermediate_size, image_size, patch_size, hidden_act, dtype, projection_dim=None,
                 split_precision=False):
    """Raises ValueError naming every setting of a CLIP vision configuration that this build's kernels do not take, with its value.
    split_precision: the check of CLIPVisionTowerX3, whose only dtype is ops.F16X3 (CLIPVisionTower's are float16 and bfloat16)."""
    bad = blocks.clip_config_errors(dtype, hidden_size, num_attention_heads, intermediate_size, hidden_act, projection_dim,
                                    (64, 128, 256), 'one of dts_attention\'s 64 / 128 / 256', split_precision=split_precision)
    if patch_size <= 0 or image_size <= 0 or image_size % patch_size:
        bad.append(f'image_size={image_size} is not a multiple of patch_size={patch_size}')
    if bad:
        raise ValueError('CLIPVisionTower: ' + '; '.join(bad))


def patch_weight_matrix(w, kpad=None):
    """patch_embedding.weight [hidden, 3, p, p] -> [hidden, kpad]: each filter flattened in (c, py, px) order -- the column order of
    ops.patchify -- followed by zero columns up to kpad (default ops.patch_kpad(p))."""
    hidden, cin, p, p2 = w.shape
    if cin != 3 or p != p2:
        raise ValueError(f'CLIPVisionTower: patch_embedding.weight {tuple(w.shape)} is not [hidden, 3, p, p]')
    kpad = ops.patch_kpad(p) if kpad is None else kpad
    out = torch.zeros((hidden, kpad), dtype=w.dtype, device=w.device)
    out[:, :3 * p * p] = w.reshape(hidden, 3 * p * p)
    return out


def vision_config(cfg):
    """the vision settings of a config.json dict (a CLIPModel's, with `vision_config` nested, or a CLIPVisionModelWithProjection's own),
    absent keys taking transformers' defaults; projection_dim is the top-level one of a CLIPModel (the shape of visual_projection)"""
    return blocks.clip_section(cfg, 'vision_config', CONFIG_DEFAULTS)


def read_vision_tensors(path):
    """(vision settings, state dict) of a local directory holding `config.json` + `model.safetensors` (what `save_pretrained` writes):
    only `vision_model.*` and `visual_projection.weight` are read -- the text tower never leaves disk.  Host tensors; no GPU needed."""
    cfg, st_file = blocks.clip_files(path)
    sd = blocks.read_tensors(st_file, lambda keys: {k: k for k in keys if k.startswith(PREFIX) or k == PROJECTION}, PREFIX + '*')
    return vision_config(cfg), sd


class CLIPVisionTower:
    """dtype torch.float16 / torch.bfloat16: the 16-bit THROUGHPUT modes (the default, float16, is what the scorer's vision_tower='hip' has
    always run).  The PARITY-GRADE mode is CLIPVisionTowerX3 below."""
    SPLIT_PRECISION, DEFAULT_DTYPE = False, torch.float16

    def __init__(self, state_dict, hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=24, image_size=224,
                 patch_size=14, hidden_act='quick_gelu', layer_norm_eps=1e-5, projection_dim=None, device='cuda', dtype=torch.float16):
        """The defaults are ViT-L/14's (openai/clip-vit-large-patch14, the reference's scorer).  projection_dim None: taken from
        visual_projection.weight."""
        check_config(hidden_size, num_attention_heads, intermediate_size, image_size, patch_size, hidden_act, dtype, projection_dim,
                     split_precision=self.SPLIT_PRECISION)
        blocks.require_gpu('CLIPVisionTower')
        self.device, self.dtype, self.x3 = torch.device(device), dtype, self.SPLIT_PRECISION
        self.hidden, self.heads, self.inter, self.layers_n = int(hidden_size), int(num_attention_heads), int(intermediate_size), int(num_hidden_layers)
        self.image_size, self.patch, self.act, self.eps = int(image_size), int(patch_size), hidden_act, float(layer_norm_eps)
        self.grid = self.image_size // self.patch
        self.tokens = self.grid * self.grid + 1
        self.scale = (self.hidden // self.heads) ** -0.5
        self.kpad = ops.patch_kpad(self.patch)
        self.proj_dim = projection_dim
        self.config = types.SimpleNamespace(hidden_size=self.hidden, num_attention_heads=self.heads, intermediate_size=self.inter,
                                            num_hidden_layers=self.layers_n, image_size=self.image_size, patch_size=self.patch,
                                            hidden_act=self.act, layer_norm_eps=self.eps, projection_dim=projection_dim)
        self.rows = 0
        self._load(state_dict)

    @classmethod
    def from_clip_model(cls, model, dtype=None, device='cuda'):
        """From a `transformers.CLIPModel` or `CLIPVisionModelWithProjection`: only its state dict and configuration are read, no reference
        to the module is kept.  dtype None: the class's default (float16; f16x3 for CLIPVisionTowerX3)."""
        dtype = cls.DEFAULT_DTYPE if dtype is None else dtype
        vc = getattr(model.config, 'vision_config', None) or model.config
        sd = {k: v for k, v in model.state_dict().items() if k.startswith(PREFIX) or k == PROJECTION}
        return cls(sd, hidden_size=vc.hidden_size, num_attention_heads=vc.num_attention_heads, intermediate_size=vc.intermediate_size,
                   num_hidden_layers=vc.num_hidden_layers, image_size=vc.image_size, patch_size=vc.patch_size, hidden_act=vc.hidden_act,
                   layer_norm_eps=vc.layer_norm_eps, device=device, dtype=dtype)

    @classmethod
    def from_pretrained(cls, path, dtype=None, device='cuda'):
        """Reads a local directory of `config.json` + `model.safetensors` (read_vision_tensors: the vision tensors only)."""
        dtype = cls.DEFAULT_DTYPE if dtype is None else dtype
        cfg, sd = read_vision_tensors(path)
        cfg.pop('projection_dim')                     # the tensor's own shape decides
        return cls(sd, device=device, dtype=dtype, **cfg)

    # ---- parameters ----------------------------------------------------------------------------
    def _check_shapes(self, sd):
        """the parameters must be those of the configuration this object was given: a mismatch is named here, not met as a reshape error"""
        C, I, L, p, T = self.hidden, self.inter, self.layers_n, self.patch, self.tokens
        last = f'{PREFIX}encoder.layers.{L - 1}'
        want = {f'{PREFIX}embeddings.class_embedding': (C,), f'{PREFIX}embeddings.patch_embedding.weight': (C, 3, p, p),
                f'{PREFIX}embeddings.position_embedding.weight': (T, C), f'{PREFIX}pre_layrnorm.weight': (C,),
                f'{PREFIX}post_layernorm.weight': (C,), f'{last}.self_attn.q_proj.weight': (C, C), f'{last}.mlp.fc1.weight': (I, C),
                f'{last}.mlp.fc2.weight': (C, I)}
        blocks.check_shapes('CLIPVisionTower', sd, want, f'num_hidden_layers={L}',
                            f'hidden_size={C}, intermediate_size={I}, image_size={self.image_size}, patch_size={p}')
        if f'{PREFIX}encoder.layers.{L}.layer_norm1.weight' in sd:
            raise ValueError(f'CLIPVisionTower: the state dict has more than num_hidden_layers={L} layers')
        if f'{PREFIX}embeddings.patch_embedding.bias' in sd:
            raise ValueError('CLIPVisionTower: a patch embedding with a bias is not CLIP\'s')
        if PROJECTION not in sd:
            raise ValueError(f'CLIPVisionTower: the state dict has no {PROJECTION!r} (a CLIPModel or CLIPVisionModelWithProjection is needed)')
        proj = tuple(sd[PROJECTION].shape)
        if len(proj) != 2 or proj[1] != C or (self.proj_dim is not None and proj[0] != self.proj_dim):
            raise ValueError(f'CLIPVisionTower: {PROJECTION} has shape {proj}, but hidden_size={C}, projection_dim={self.proj_dim}')

    def _load(self, sd):
        self._check_shapes(sd)
        p, e = blocks.Params(self.device, self.dtype), PREFIX + 'embeddings.'
        self.w_patch, _ = p.pack(patch_weight_matrix(p.f32(sd[e + 'patch_embedding.weight']), self.kpad))
        self.cls, self.pos = p.f32(sd[e + 'class_embedding']), p.f32(sd[e + 'position_embedding.weight'])
        self.pre_ln, self.post_ln = p.norm(sd, PREFIX + 'pre_layrnorm'), p.norm(sd, PREFIX + 'post_layernorm')
        self.layers = blocks.clip_layers(p, sd, PREFIX, self.layers_n)
        self.w_proj = p.f32(sd[PROJECTION])                            # f32 [projection_dim, hidden], no bias
        self.proj_dim = self.config.projection_dim = self.w_proj.shape[0]
        torch.cuda.synchronize(self.device)

    # ---- forward -------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, pixel_values):
        """pixel_values [n, 3, image_size, image_size] (what CLIPImageProcessor / clip_preprocess.DevicePreprocessor make)
        -> float32 [n, projection_dim], the `image_embeds` before normalisation (CLIPModel.get_image_features)."""
        S, C, T, g = self.image_size, self.hidden, self.tokens, self.grid
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, S, S):
            raise ValueError(f'CLIPVisionTower: pixel_values {tuple(pixel_values.shape)} is not [n, 3, {S}, {S}]')
        n = pixel_values.shape[0]
        x = pixel_values.to(self.device, torch.float32).contiguous()
        if self.x3:
            return self._forward_x3(x, n)
        rows = ops.patchify(x, self.patch, self.dtype, self.kpad)                                  # [n, g*g, kpad]
        emb = ops.conv2d(rows.view(n, g, g, self.kpad), self.w_patch)                              # the patch embedding has no bias
        h = ops.vit_tokens(emb.view(n, g * g, C), self.cls, self.pos)
        h = ops.layer_norm(h, *self.pre_ln, eps=self.eps).view(n, T, 1, C)
        h = blocks.clip_encoder(h, self.layers, self.eps, self.act, lambda qkv: ops.attention(qkv, self.heads, self.scale))
        pooled = ops.vit_head(h.view(n, T, C), *self.post_ln, eps=self.eps)                        # f32 [n, C]: the class token only
        self.rows += n
        return ops.linear(pooled, self.w_proj)

    def _forward_x3(self, x, n):
        """the same forward in the split-precision mode: float32 activations, X3Weight matrix products (ops.F16X3)"""
        C, T, g = self.hidden, self.tokens, self.grid
        emb = ops.conv2d(ops.patchify_x3(x, self.patch, self.kpad), self.w_patch)                  # f32 [n, g, g, C]
        h = ops.vit_tokens_f32(emb.view(n, g * g, C), self.cls, self.pos)
        h = ops.layer_norm_x3(h, *self.pre_ln, eps=self.eps, want_f32=True, want_split=False).view(n, T, 1, C)     # the residual stream
        h = blocks.clip_encoder_x3(h, self.layers, self.eps, self.act, self.heads, self.scale)
        pooled = ops.vit_head_f32(h.view(n, T, C), *self.post_ln, eps=self.eps)
        self.rows += n
        return ops.linear(pooled, self.w_proj)

    forward = __call__

    def flops(self, n=1):
        """algorithmic FLOPs (2 per multiply-add) of a forward over n images, counted from the layer shapes: the matrix products of the patch
        embedding, the four projections, the two attention products, the MLP and the output projection"""
        C, I, T, L = self.hidden, self.inter, self.tokens, self.layers_n
        per_layer = 2 * T * C * 3 * C + 2 * T * C * C + 2 * 2 * T * T * C + 2 * 2 * T * C * I
        return n * (2 * (T - 1) * 3 * self.patch * self.patch * C + L * per_layer + 2 * C * self.proj_dim)


class CLIPVisionTowerX3(CLIPVisionTower):
    """The parity-grade form of the tower: float32 activations, every matrix product in split precision (dtype ops.F16X3, its only dtype),
    held to a small factor of the float32 transformers module's own rounding error against float64 -- use it where the scorer's
    selections must match the reference's.  Same constructor, state dict, from_clip_model / from_pretrained and flops() as CLIPVisionTower."""
    SPLIT_PRECISION, DEFAULT_DTYPE = True, ops.F16X3

    def __init__(self, state_dict, *args, dtype=ops.F16X3, **kw):
        super().__init__(state_dict, *args, dtype=dtype, **kw)
