"""The text tower of CLIP on the HIP kernels: drop-in for `CLIPTextModel` as the text encoder of the SD search loop
(sd_pipeline.SDSearchPipeline.encode_prompt) and for `CLIPModel.get_text_features` in the scorer (scorers.CLIPScorer), i.e. for
CLIPTextTransformer.forward + text_projection of transformers (models/clip/modeling_clip.py: CLIPTextEmbeddings, CLIPEncoderLayer,
CLIPAttention with the causal mask, CLIPMLP).  The twin of clip_vision.CLIPVisionTower:
  token_embedding(ids) + position_embedding  -> dts_text_tokens (f32 sum, rounded once; the ids are checked on the host)
  layer_norm1 / 2, final_layer_norm          -> dts_layer_norm
  q_proj | k_proj | v_proj                   -> ONE 1x1 dts_conv2d (rows and biases stacked at load time)
  causal softmax(q k^T / sqrt d) v           -> dts_attention_masked (causal, plus a per-sample key length from a right-padding mask)
  out_proj, fc2                              -> 1x1 dts_conv2d with the bias and the residual add in the epilogue
  fc1 + activation                           -> 1x1 dts_conv2d + dts_gelu (quick-GELU or erf GELU, in place)
  last_hidden_state[b, eos position]         -> torch indexing (plumbing); the positions come from the ids on the host (pooled_positions)
  text_projection                            -> dts_cast_to_f32 + dts_linear (f32), when the state dict has one
Activations are [n, t, 1, channels] in `dtype` (float16 or bfloat16): a 16-bit THROUGHPUT mode (SD's text encoder runs in float16 in the
reference; its CLIP scorer embeds the prompt in float32).  CLIPTextTowerX3 (dtype ops.F16X3, 'f16x3') is the PARITY-GRADE mode, the twin of
clip_vision.CLIPVisionTowerX3 -- float32 activations, every matrix product in split precision on the 16-bit matrix cores:
  tokens -> dts_text_tokens_f32; layer_norm1 / 2, final_layer_norm -> dts_layer_norm_x3; projections -> dts_conv2d in DTS_F16X3 (the qkv
  projection writes the attention's operand image); causal attention -> dts_attention_x3_masked at every t (it writes out_proj's operand
  image); activation -> dts_gelu_x3; text_projection -> dts_linear on the float32 pooled row
It is held to the float32 module's own distance from float64 (tests/test_gpu_clip_text_x3.py).  torch.float32 itself is refused by both
classes: there is no float32 matrix-instruction form of this tower.  CLIPTextTower keeps refusing every dtype but the two 16-bit ones,
'f16x3' included: the split-precision mode is a class of its own with a check of its own (check_config_x3).  NO graph capture: the tower
runs once per prompt over 2 x 77 tokens, it is not a hot path.

Parameters: a state dict with transformers' key names (`text_model.*`, `text_projection.weight`).  Shapes the kernels do not take are
refused by name at construction (check_config); an attention mask that is not right padding is refused by name at call time.
"""
import types

import torch

from . import blocks, ops

PREFIX = 'text_model.'
PROJECTION = 'text_projection.weight'
# transformers' CLIPTextConfig defaults: config.json stores only what differs from them
CONFIG_DEFAULTS = {'vocab_size': 49408, 'hidden_size': 512, 'intermediate_size': 2048, 'num_hidden_layers': 12, 'num_attention_heads': 8,
                   'max_position_embeddings': 77, 'hidden_act': 'quick_gelu', 'layer_norm_eps': 1e-5, 'eos_token_id': 49407,
                   'projection_dim': 512}


def check_config(hidden_size, num_attention_heads, intermediate_size, hidden_act, dtype, vocab_size=49408, max_position_embeddings=77,
                 projection_dim=None):
    """Raises ValueError naming every setting of a CLIP text configuration that this build's kernels do not take, with its value."""
    bad = blocks.clip_config_errors(dtype, hidden_size, num_attention_heads, intermediate_size, hidden_act, projection_dim,
                                    (64,), 'dts_attention_masked\'s 64')
    if vocab_size <= 0 or max_position_embeddings <= 0:
        bad.append(f'vocab_size={vocab_size}, max_position_embeddings={max_position_embeddings}')
    if bad:
        raise ValueError('CLIPTextTower: ' + '; '.join(bad))


def check_config_x3(hidden_size, num_attention_heads, intermediate_size, hidden_act, dtype, vocab_size=49408, max_position_embeddings=77,
                    projection_dim=None):
    """check_config for CLIPTextTowerX3, whose only dtype is ops.F16X3 (head dim 64: dts_attention_x3_masked's)"""
    bad = blocks.clip_config_errors(dtype, hidden_size, num_attention_heads, intermediate_size, hidden_act, projection_dim,
                                    (64,), 'dts_attention_x3_masked\'s 64', split_precision=True)
    if vocab_size <= 0 or max_position_embeddings <= 0:
        bad.append(f'vocab_size={vocab_size}, max_position_embeddings={max_position_embeddings}')
    if bad:
        raise ValueError('CLIPTextTower: ' + '; '.join(bad))


def pooled_positions(ids, eos_token_id):
    """int64 [n] on the host: the token whose hidden state is the pooled output, by transformers' rule (CLIPTextTransformer.forward).  The
    legacy eos_token_id == 2 (configurations written before transformers stored the real id): argmax(ids) -- the end-of-text token has the
    largest id of CLIP's vocabulary; otherwise the first position equal to eos_token_id (position 0 if there is none, as the argmax of an
    all-false row)."""
    ids = ids.detach().cpu().to(torch.int64)
    if ids.dim() != 2:
        raise ValueError(f'pooled_positions: ids {tuple(ids.shape)} is not [n, t]')
    if eos_token_id == 2:
        return ids.argmax(dim=-1)
    return (ids == eos_token_id).to(torch.int64).argmax(dim=-1)


def mask_key_len(attention_mask, n, t):
    """attention_mask [n, t] (or None) -> None (no mask, or all ones: nothing to hide) or int32 [n] on the host, the number of ones of
    every row, for a RIGHT-padded mask: a prefix of ones, at least one, then zeros.  Anything else -- left padding, a hole, an all-zero row,
    values other than 0 and 1 -- is refused by name: dts_attention_masked takes a key length per sample, not a mask."""
    if attention_mask is None:
        return None
    m = attention_mask.detach().cpu()
    if tuple(m.shape) != (n, t):
        raise ValueError(f'CLIPTextTower: attention_mask {tuple(m.shape)} does not match input_ids {(n, t)}')
    m = m.to(torch.int64)
    if bool(((m != 0) & (m != 1)).any()):
        raise ValueError('CLIPTextTower: attention_mask holds values other than 0 and 1')
    lens = m.sum(-1)
    for b in range(n):
        L = int(lens[b])
        if L == 0:
            raise ValueError(f'CLIPTextTower: attention_mask row {b} is all zero (every row needs at least one token)')
        if int(m[b, 0]) == 0:
            raise ValueError(f'CLIPTextTower: attention_mask row {b} is left-padded (it starts with 0); only right padding is taken')
        if not bool(m[b, :L].all()):
            raise ValueError(f'CLIPTextTower: attention_mask row {b} has a hole (a 0 at position {int((m[b] == 0).to(torch.int64).argmax())} '
                             f'before a 1); only right padding is taken')
    if bool((lens == t).all()):
        return None
    return lens.to(torch.int32)


def text_config(cfg):
    """the text settings of a config.json dict (a CLIPModel's, with `text_config` nested, or a CLIPTextModel's own), absent keys taking
    transformers' defaults; projection_dim is the top-level one of a CLIPModel (the shape of text_projection)"""
    return blocks.clip_section(cfg, 'text_config', CONFIG_DEFAULTS)


def text_keys(keys):
    """{key as stored: key in the `text_model.*` naming} for the text tensors among `keys`.  A CLIPModel and a CLIPTextModelWithProjection
    store them as `text_model.*` (+ `text_projection.weight`), and so does the text_encoder/ directory of a published SD checkpoint; a
    CLIPTextModel of transformers 5 stores them bare (`embeddings.*`, `encoder.*`, `final_layer_norm.*`): recognised by its
    `embeddings.token_embedding.weight` and renamed."""
    keys = list(keys)
    bare = 'embeddings.token_embedding.weight' in keys
    out = {}
    for k in keys:
        if k.startswith(PREFIX) or k == PROJECTION:
            out[k] = k
        elif bare and k.startswith(('embeddings.', 'encoder.', 'final_layer_norm.')):
            out[k] = PREFIX + k
    return out


def read_text_tensors(path):
    """(text settings, state dict) of a local directory holding `config.json` + `model.safetensors` (what `save_pretrained` writes: an SD
    checkpoint's text_encoder/ directory, or a CLIP directory): only `text_model.*` and `text_projection.weight` are read -- the vision
    tower never leaves disk.  Host tensors; no GPU needed."""
    cfg, st_file = blocks.clip_files(path)
    return text_config(cfg), blocks.read_tensors(st_file, text_keys, PREFIX + '*')


class TextOutput:
    """what the tower returns: `[0]` / `.last_hidden_state` [n, t, C] and `.pooler_output` [n, C] in the tower's dtype (float32 from
    CLIPTextTowerX3), and, with a projection, `.text_embeds` float32 [n, projection_dim] (else None)"""

    def __init__(self, last_hidden_state, pooler_output, text_embeds):
        self.last_hidden_state, self.pooler_output, self.text_embeds = last_hidden_state, pooler_output, text_embeds

    def __getitem__(self, i):
        return (self.last_hidden_state, self.pooler_output)[i]


class CLIPTextTower:
    """dtype torch.float16 / torch.bfloat16: the 16-bit modes.  The PARITY-GRADE mode is CLIPTextTowerX3 below."""
    SPLIT_PRECISION, DEFAULT_DTYPE = False, torch.float16

    def __init__(self, state_dict, vocab_size=49408, hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=12,
                 max_position_embeddings=77, hidden_act='quick_gelu', layer_norm_eps=1e-5, eos_token_id=49407, projection_dim=None,
                 device='cuda', dtype=torch.float16):
        """The defaults are those of SD-1.5's text encoder (openai/clip-vit-large-patch14's text side).  projection_dim None: taken from
        text_projection.weight when the state dict has one (a CLIPTextModel has none: no `.text_embeds` then)."""
        (check_config_x3 if self.SPLIT_PRECISION else check_config)(hidden_size, num_attention_heads, intermediate_size, hidden_act, dtype,
                                                                    vocab_size, max_position_embeddings, projection_dim)
        blocks.require_gpu('CLIPTextTower')
        self.device, self.dtype, self.x3 = torch.device(device), dtype, self.SPLIT_PRECISION
        self.vocab, self.hidden, self.heads, self.inter = int(vocab_size), int(hidden_size), int(num_attention_heads), int(intermediate_size)
        self.layers_n, self.max_pos, self.act, self.eps = int(num_hidden_layers), int(max_position_embeddings), hidden_act, float(layer_norm_eps)
        self.eos = int(eos_token_id)
        self.scale = (self.hidden // self.heads) ** -0.5
        self.proj_dim = projection_dim
        # (no use_attention_mask: SDSearchPipeline.encode_prompt then passes no mask, as it does for SD-1.x's CLIPTextModel)
        self.config = types.SimpleNamespace(vocab_size=self.vocab, hidden_size=self.hidden, num_attention_heads=self.heads,
                                            intermediate_size=self.inter, num_hidden_layers=self.layers_n,
                                            max_position_embeddings=self.max_pos, hidden_act=self.act, layer_norm_eps=self.eps,
                                            eos_token_id=self.eos, projection_dim=projection_dim)
        self.rows = 0
        self._load(state_dict)

    @classmethod
    def from_text_model(cls, model, dtype=None, device='cuda'):
        """From a `transformers.CLIPTextModel`, `CLIPTextModelWithProjection` or `CLIPModel`: only its state dict (`text_model.*`,
        `text_projection.weight`) and text configuration are read, no reference to the module is kept.  dtype None: the class's default
        (float16; f16x3 for CLIPTextTowerX3)."""
        dtype = cls.DEFAULT_DTYPE if dtype is None else dtype
        tc = getattr(model.config, 'text_config', None) or model.config
        full = model.state_dict()
        sd = {name: full[k] for k, name in text_keys(full).items()}
        return cls(sd, vocab_size=tc.vocab_size, hidden_size=tc.hidden_size, num_attention_heads=tc.num_attention_heads,
                   intermediate_size=tc.intermediate_size, num_hidden_layers=tc.num_hidden_layers,
                   max_position_embeddings=tc.max_position_embeddings, hidden_act=tc.hidden_act, layer_norm_eps=tc.layer_norm_eps,
                   eos_token_id=tc.eos_token_id, device=device, dtype=dtype)

    @classmethod
    def from_pretrained(cls, path, dtype=None, device='cuda'):
        """Reads a local directory of `config.json` + `model.safetensors` (read_text_tensors: the text tensors only)."""
        dtype = cls.DEFAULT_DTYPE if dtype is None else dtype
        cfg, sd = read_text_tensors(path)
        cfg.pop('projection_dim')                     # the tensor's own shape decides
        return cls(sd, device=device, dtype=dtype, **cfg)

    # ---- parameters ----------------------------------------------------------------------------
    def _check_shapes(self, sd):
        """the parameters must be those of the configuration this object was given: a mismatch is named here, not met as a reshape error"""
        C, I, L, V, P = self.hidden, self.inter, self.layers_n, self.vocab, self.max_pos
        last = f'{PREFIX}encoder.layers.{L - 1}'
        want = {f'{PREFIX}embeddings.token_embedding.weight': (V, C), f'{PREFIX}embeddings.position_embedding.weight': (P, C),
                f'{PREFIX}final_layer_norm.weight': (C,), f'{last}.self_attn.q_proj.weight': (C, C), f'{last}.mlp.fc1.weight': (I, C),
                f'{last}.mlp.fc2.weight': (C, I)}
        blocks.check_shapes('CLIPTextTower', sd, want, f'num_hidden_layers={L}',
                            f'vocab_size={V}, hidden_size={C}, intermediate_size={I}, max_position_embeddings={P}')
        if f'{PREFIX}encoder.layers.{L}.layer_norm1.weight' in sd:
            raise ValueError(f'CLIPTextTower: the state dict has more than num_hidden_layers={L} layers')
        if PROJECTION in sd:
            proj = tuple(sd[PROJECTION].shape)
            if len(proj) != 2 or proj[1] != C or (self.proj_dim is not None and proj[0] != self.proj_dim):
                raise ValueError(f'CLIPTextTower: {PROJECTION} has shape {proj}, but hidden_size={C}, projection_dim={self.proj_dim}')
        elif self.proj_dim is not None:
            raise ValueError(f'CLIPTextTower: projection_dim={self.proj_dim}, but the state dict has no {PROJECTION!r}')

    def _load(self, sd):
        self._check_shapes(sd)
        p, e = blocks.Params(self.device, self.dtype), PREFIX + 'embeddings.'
        self.tok, self.pos = p.f32(sd[e + 'token_embedding.weight']), p.f32(sd[e + 'position_embedding.weight'])
        self.final_ln = p.norm(sd, PREFIX + 'final_layer_norm')
        self.layers = blocks.clip_layers(p, sd, PREFIX, self.layers_n)
        self.w_proj = p.f32(sd[PROJECTION]) if PROJECTION in sd else None      # f32 [projection_dim, hidden], no bias
        self.proj_dim = self.config.projection_dim = None if self.w_proj is None else self.w_proj.shape[0]
        torch.cuda.synchronize(self.device)

    # ---- forward -------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, input_ids, attention_mask=None):
        """input_ids integer [n, t] (the tokenizer's; host or device), attention_mask None or a right-padding mask [n, t] -> TextOutput.
        The ids and the mask are read on the host (a device tensor is copied back: one synchronisation per prompt)."""
        if not torch.is_tensor(input_ids) or input_ids.dim() != 2:
            raise ValueError('CLIPTextTower: input_ids must be an integer tensor [n, t]')
        n, t = input_ids.shape
        if t > self.max_pos:
            raise ValueError(f'CLIPTextTower: {t} tokens exceed max_position_embeddings={self.max_pos}')
        C = self.hidden
        ids = input_ids.detach().cpu()
        lens = mask_key_len(attention_mask, n, t)
        key_len = None if lens is None else lens.to(self.device)
        pos = pooled_positions(ids, self.eos)
        if self.x3:
            return self._forward_x3(ids, key_len, pos, n, t)
        h = ops.text_tokens(ids, self.tok, self.pos, self.dtype).view(n, t, 1, C)                  # checks 0 <= id < vocab on the host
        h = blocks.clip_encoder(h, self.layers, self.eps, self.act,
                                lambda qkv: ops.attention_masked(qkv, self.heads, self.scale, causal=True, key_len=key_len))
        last = ops.layer_norm(h, *self.final_ln, eps=self.eps).view(n, t, C)                       # every token
        pooled = last[torch.arange(n, device=self.device), pos.to(self.device)].contiguous()
        embeds = None if self.w_proj is None else ops.linear(ops.cast_to_f32(pooled), self.w_proj)
        self.rows += n
        return TextOutput(last, pooled, embeds)

    def _forward_x3(self, ids, key_len, pos, n, t):
        """the same forward in the split-precision mode: float32 activations, X3Weight matrix products (ops.F16X3), the masked
        split-precision attention between the qkv projection's and out_proj's operand images at every sequence length"""
        C = self.hidden
        h = ops.text_tokens_f32(ids, self.tok, self.pos).view(n, t, 1, C)                           # checks 0 <= id < vocab on the host
        attend = lambda qkv: ops.attention_x3_masked(qkv, self.heads, self.scale, causal=True, key_len=key_len, split_out=True)
        h = blocks.clip_encoder_x3(h, self.layers, self.eps, self.act, self.heads, self.scale, attend=attend)
        last = ops.layer_norm_x3(h, *self.final_ln, eps=self.eps, want_f32=True, want_split=False).view(n, t, C)     # every token, float32
        pooled = last[torch.arange(n, device=self.device), pos.to(self.device)].contiguous()
        embeds = None if self.w_proj is None else ops.linear(pooled, self.w_proj)
        self.rows += n
        return TextOutput(last, pooled, embeds)

    forward = __call__

    def get_text_features(self, input_ids, attention_mask=None):
        """float32 [n, projection_dim], the `text_embeds` before normalisation (CLIPModel.get_text_features)"""
        if self.w_proj is None:
            raise ValueError(f'CLIPTextTower: the state dict had no {PROJECTION!r} (a CLIPModel or CLIPTextModelWithProjection is needed)')
        return self(input_ids, attention_mask).text_embeds


class CLIPTextTowerX3(CLIPTextTower):
    """The parity-grade form of the tower: float32 activations and outputs, every matrix product in split precision (dtype ops.F16X3, its
    only dtype), held to a small factor of the float32 transformers module's own rounding error against float64 -- use it where the
    scorer's rewards must match the reference's.  Same constructor, state dict, from_text_model / from_pretrained as CLIPTextTower."""
    SPLIT_PRECISION, DEFAULT_DTYPE = True, ops.F16X3

    def __init__(self, state_dict, *args, dtype=ops.F16X3, **kw):
        super().__init__(state_dict, *args, dtype=dtype, **kw)
