"""The SD-1.x U-Net on the HIP kernels: drop-in for the `unet` object of the SD search loop
(`unet(sample, t, encoder_hidden_states=..., return_dict=False)[0]`, `.config`, `.dtype`, `.device`), i.e. for `UNet2DConditionModel.forward`
of the vendored diffusers (sd/diffusers/src/diffusers/models/unets/unet_2d_condition.py, unet_2d_blocks.py, resnet.py,
transformers/transformer_2d.py, attention.py, attention_processor.py).

Two U-Net rows per candidate per DDIM step are the largest cost of an SD search; here they run on the same kernels as the EDM denoisers
and the VAE decoder, plus the three the transformer blocks need:
  3x3 / 1x1 convs, every Linear      -> dts_conv2d (implicit GEMM on MFMA; nearest-2x upsample fused into the gather; time-embedding
                                        addend, residual add in the epilogue; the up blocks' channel concat as the x2 operand, never a copy)
  GroupNorm(32) [+ SiLU]             -> dts_gn_* (statistics fused into the producing conv's epilogue where possible)
  self-attention                     -> dts_attention
  attention over the text tokens     -> dts_cross_attention (K and V of a head in LDS at once; rows that share a context share its k|v)
  LayerNorm, GEGLU                   -> dts_layer_norm, dts_geglu
  time embedding                     -> dts_pos_embedding, dts_linear (f32)
  Downsample2D (3x3, stride 2)       -> dts_space_to_depth2 + a 3x3 stride-1 conv over 4C channels (ops.stride2_conv_weight): downsample='s2d',
                                        the default; downsample='strided': dts_conv2d's stride-2 form over the C channels themselves
  torch.unique(dim=0) over the contexts -> dts_group_rows (which rows carry the same text context, in order of first occurrence, no sort)
The forward is a host part (argument checks, the timestep, grouping) and a fixed-shape device part (_device_forward: the distinct contexts and
a row map in, no host read) that graphs.GraphCache captures once per shape and replays, like the EDM denoisers' forwards.
Activations are NHWC in `dtype` (float16 like the reference pipeline, or bfloat16).  The 4 latent channels are zero-padded to 64 for the
MFMA conv (cin % 64 == 0) and conv_out's 4 output channels likewise (cout % 64 == 0).  SD-1.5's head dims 40 / 80 / 160 are zero-padded to
64 / 128 / 256 at load time (rows of to_q / to_k / to_v, columns of to_out.0; scale = 1/sqrt(true dim)): exact, see pad_head_rows.  That is
head_dims='padded', the default; head_dims='native' keeps them as stored (the attention kernels take 40 / 80 / 160 and pad on chip), so
the q/k/v/out projections run at 320 / 640 / 1280 channels instead of 512 / 1024 / 2048 (native_head_dim).

Parameters: a state dict with diffusers' key names (`UNet2DConditionModel.state_dict()` / the safetensors file of SD-1.5's unet/).
Stock SD-1.x configuration only (check_config); anything else is refused by name.
"""
import math
import types

import torch

from . import blocks, ops
from .graphs import GraphCache

STOCK = {
    '_class_name': 'UNet2DConditionModel',
    'down_block_types': ['CrossAttnDownBlock2D', 'CrossAttnDownBlock2D', 'CrossAttnDownBlock2D', 'DownBlock2D'],
    'mid_block_type': 'UNetMidBlock2DCrossAttn',
    'up_block_types': ['UpBlock2D', 'CrossAttnUpBlock2D', 'CrossAttnUpBlock2D', 'CrossAttnUpBlock2D'],
    'use_linear_projection': False, 'act_fn': 'silu', 'norm_num_groups': 32, 'norm_eps': 1e-5, 'resnet_time_scale_shift': 'default',
    'flip_sin_to_cos': True, 'freq_shift': 0, 'transformer_layers_per_block': 1, 'class_embed_type': None, 'addition_embed_type': None,
    'num_class_embeds': None, 'time_cond_proj_dim': None, 'encoder_hid_dim': None, 'encoder_hid_dim_type': None,
    'dual_cross_attention': False, 'only_cross_attention': False, 'upcast_attention': False, 'center_input_sample': False,
    'in_channels': 4, 'out_channels': 4, 'time_embedding_type': 'positional', 'time_embedding_dim': None, 'timestep_post_act': None,
    'time_embedding_act_fn': None, 'conv_in_kernel': 3, 'conv_out_kernel': 3, 'downsample_padding': 1, 'mid_block_scale_factor': 1,
    'num_attention_heads': None, 'attention_type': 'default', 'cross_attention_norm': None, 'resnet_skip_time_act': False,
    'resnet_out_scale_factor': 1.0, 'class_embeddings_concat': False, 'mid_block_only_cross_attention': None,
    'reverse_transformer_layers_per_block': None, 'addition_time_embed_dim': None, 'projection_class_embeddings_input_dim': None,
    'dropout': 0.0,
}


def check_config(cfg):
    """Raises ValueError naming the first key of a diffusers U-Net config that is not the stock SD-1.x setting (keys that are absent
    have diffusers' defaults, which are the stock ones)."""
    for key, want in STOCK.items():
        if key not in cfg:
            continue
        got = cfg[key]
        if isinstance(got, tuple):
            got = list(got)
        if got != want:
            raise ValueError(f'SDUNet: {key}={cfg[key]!r} is not the stock SD-1.x U-Net ({want!r})')
    for key in ('attention_head_dim', 'layers_per_block', 'cross_attention_dim'):
        if key in cfg and not isinstance(cfg[key], int):
            raise ValueError(f'SDUNet: {key}={cfg[key]!r} is not the stock SD-1.x U-Net (one integer)')
    if 'block_out_channels' in cfg and len(cfg['block_out_channels']) != 4:
        raise ValueError(f'SDUNet: block_out_channels={cfg["block_out_channels"]!r} is not the stock SD-1.x U-Net (four levels)')


def padded_head_dim(d):
    """the head dim of the attention kernels (64 / 128 / 256) that holds a true head dim d"""
    for dp in (64, 128, 256):
        if d <= dp:
            return dp
    raise ValueError(f'SDUNet: head dim {d} exceeds the attention kernels\' 256')


HEAD_DIMS = ('padded', 'native')
DOWNSAMPLE = ('s2d', 'strided')


def native_head_dim(d, heads):
    """head_dims='native': the smallest head dim the 16-bit attention kernels take (40 / 64 / 80 / 128 / 160 / 256) that holds a true head
    dim d AND leaves heads * dn a multiple of 64 -- the projections are 1x1 dts_conv2d calls, which need cin % 64 == 0 (to_out.0 reads
    heads * dn channels).  SD-1.x (8 heads of 40 / 80 / 160) keeps its own dims; 2 heads of 32 take 64, since 2 * 40 = 80 would not do."""
    for dn in (40, 64, 80, 128, 160, 256):
        if d <= dn and (heads * dn) % 64 == 0:
            return dn
    raise ValueError(f'SDUNet: head dim {d} exceeds the attention kernels\' 256')


def pad_head_rows(w, heads, dpad):
    """to_q / to_k / to_v weight [heads*d, cin] -> [heads*dpad, cin]: each head's d output rows followed by dpad - d zero rows.  With the
    matching pad_head_cols of to_out.0 the attention is unchanged: the padded q and k components add 0 to every q.k, the padded v
    components are 0 and meet zero columns of to_out.0 -- as long as the softmax scale stays 1/sqrt(d) of the TRUE head dim."""
    hd, cin = w.shape
    d = hd // heads
    out = torch.zeros((heads, dpad, cin), dtype=w.dtype, device=w.device)
    out[:, :d] = w.view(heads, d, cin)
    return out.view(heads * dpad, cin)


def pad_head_cols(w, heads, dpad):
    """to_out.0 weight [cout, heads*d] -> [cout, heads*dpad] (zero columns where the padded value channels arrive)"""
    cout, hd = w.shape
    d = hd // heads
    out = torch.zeros((cout, heads, dpad), dtype=w.dtype, device=w.device)
    out[:, :, :d] = w.view(cout, heads, d)
    return out.view(cout, heads * dpad)


class SDUNet:
    takes_context_rows = True       # __call__(..., context_rows=): the distinct contexts and a row map instead of one context per row

    def __init__(self, state_dict, block_out_channels=(320, 640, 1280, 1280), attention_head_dim=8, cross_attention_dim=768,
                 layers_per_block=2, sample_size=64, device='cuda', dtype=torch.float16, head_dims='padded', downsample='s2d'):
        """attention_head_dim: the NUMBER of heads of every transformer block (diffusers' historical name for it, unet_2d_condition.py:
        `num_attention_heads = num_attention_heads or attention_head_dim`).
        head_dims: 'padded' (default) zero-pads every head to 64 / 128 / 256 at load time (padded_head_dim); 'native' keeps the smallest
        head dim the attention kernels take (native_head_dim: 40 / 80 / 160 as stored at SD-1.x widths, nothing padded).
        downsample: 's2d' (default) runs the three Downsample2D layers as space-to-depth + a 3x3 stride-1 convolution over 4*C channels
        (9 of its 36 tap-by-phase slots live); 'strided' runs them as the stride-2 3x3 convolution they are (ops.conv2d(stride=2): a
        quarter of the multiply-adds and of the packed weight, no space-to-depth pass).  Independent of head_dims."""
        if head_dims not in HEAD_DIMS:
            raise ValueError(f'SDUNet: head_dims={head_dims!r} is not one of {HEAD_DIMS}')
        if downsample not in DOWNSAMPLE:
            raise ValueError(f'SDUNet: downsample={downsample!r} is not one of {DOWNSAMPLE}')
        self.head_dims, self.downsample = head_dims, downsample
        blocks.require_gpu('SDUNet')
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError('SDUNet: activations are float16 or bfloat16')
        self.device, self.dtype = torch.device(device), dtype
        self.boc, self.heads, self.ctx_dim, self.lpb = tuple(block_out_channels), int(attention_head_dim), int(cross_attention_dim), int(layers_per_block)
        self.groups, self.eps = 32, 1e-5
        self.config = types.SimpleNamespace(in_channels=4, out_channels=4, sample_size=sample_size, time_cond_proj_dim=None,
                                            addition_embed_type=None, block_out_channels=list(block_out_channels),
                                            attention_head_dim=self.heads, cross_attention_dim=self.ctx_dim, layers_per_block=self.lpb)
        self.rows = 0
        self._load(state_dict)
        self._graphs = GraphCache(self._device_forward)      # one capture per (rows, latent size, number of distinct contexts)

    @classmethod
    def from_pretrained(cls, path, device='cuda', dtype=torch.float16, head_dims='padded', downsample='s2d'):
        """Reads a diffusers `unet/` directory: `config.json` for the shape and `diffusion_pytorch_model[.fp16].safetensors` for the
        parameters -- the on-disk format of SD-1.5's U-Net.  A `.bin` pickle is not read.  head_dims, downsample: as the constructor's."""
        import json
        import os
        if head_dims not in HEAD_DIMS:
            raise ValueError(f'SDUNet: head_dims={head_dims!r} is not one of {HEAD_DIMS}')
        if downsample not in DOWNSAMPLE:
            raise ValueError(f'SDUNet: downsample={downsample!r} is not one of {DOWNSAMPLE}')
        cfg_file = os.path.join(path, 'config.json')
        if not os.path.exists(cfg_file):
            raise FileNotFoundError(f'{path}: no config.json (the configuration is not guessed: only a stock SD-1.x U-Net is accepted, by name)')
        with open(cfg_file) as f:
            cfg = json.load(f)
        check_config(cfg)
        sd = blocks.read_tensors(blocks.diffusers_weights(path), lambda keys: {k: k for k in keys})
        kw = {k: cfg[k] for k in ('attention_head_dim', 'cross_attention_dim', 'layers_per_block', 'sample_size') if k in cfg}
        if 'block_out_channels' in cfg:
            kw['block_out_channels'] = tuple(cfg['block_out_channels'])
        return cls(sd, device=device, dtype=dtype, head_dims=head_dims, downsample=downsample, **kw)

    # ---- parameters ----------------------------------------------------------------------------
    def _resnet_params(self, sd, key):
        P = blocks.resnet_params(self._p, sd, key)
        # time_emb_proj of every block is one row block of a single f32 matrix: one dts_linear per forward instead of 22
        P.cout = P.w1.shape[0]
        P.toff = self._tcols
        self._tw.append(self._p.f32(sd[key + '.time_emb_proj.weight']))
        self._tb.append(self._p.f32(sd[key + '.time_emb_proj.bias']))
        self._tcols += P.cout
        return P

    def _transformer_params(self, sd, key, c):
        H, p = self.heads, self._p
        if c % H:
            raise ValueError(f'SDUNet: {c} channels do not split into {H} heads')
        d = c // H
        dp = native_head_dim(d, H) if self.head_dims == 'native' else padded_head_dim(d)
        A = types.SimpleNamespace(heads=H, scale=1.0 / math.sqrt(d), hp=H * dp)
        A.g, A.b = p.norm(sd, key + '.norm')
        if sd[key + '.proj_in.weight'].dim() != 4:
            raise ValueError('SDUNet: use_linear_projection=True (a Linear proj_in) is not the stock SD-1.x U-Net')
        A.w_in, A.b_in = p.conv(sd, key + '.proj_in')
        A.w_out, A.b_out = p.conv(sd, key + '.proj_out')
        t = key + '.transformer_blocks.0'
        if key + '.transformer_blocks.1.norm1.weight' in sd:
            raise ValueError('SDUNet: transformer_layers_per_block > 1 is not the stock SD-1.x U-Net')
        A.ln = [p.norm(sd, f'{t}.norm{i}') for i in (1, 2, 3)]
        rows = lambda name: pad_head_rows(p.f32(sd[f'{t}.{name}.weight']), H, dp)
        A.w_qkv, _ = p.pack(torch.cat([rows('attn1.to_q'), rows('attn1.to_k'), rows('attn1.to_v')], 0))      # q | k | v blocks
        A.w_o1, A.b_o1 = p.pack(pad_head_cols(p.f32(sd[f'{t}.attn1.to_out.0.weight']), H, dp), p.f32(sd[f'{t}.attn1.to_out.0.bias']))
        A.w_q2, _ = p.pack(rows('attn2.to_q'))
        A.w_kv2, _ = p.pack(torch.cat([rows('attn2.to_k'), rows('attn2.to_v')], 0))                           # k | v blocks, cin = text width
        A.w_o2, A.b_o2 = p.pack(pad_head_cols(p.f32(sd[f'{t}.attn2.to_out.0.weight']), H, dp), p.f32(sd[f'{t}.attn2.to_out.0.bias']))
        A.w_ff1, A.b_ff1 = p.conv(sd, f'{t}.ff.net.0.proj')
        A.w_ff2, A.b_ff2 = p.conv(sd, f'{t}.ff.net.2')
        A.index = len(self._tfm)
        self._tfm.append(A)
        return A

    def _check_shapes(self, sd):
        """the parameters must be those of the configuration this object was given: a mismatch is named here, not met as a reshape error"""
        boc, temb = self.boc, 4 * self.boc[0]
        want = {'conv_in.weight': (boc[0], 4, 3, 3), 'conv_out.weight': (4, boc[0], 3, 3), 'time_embedding.linear_1.weight': (temb, boc[0]),
                'mid_block.resnets.0.conv1.weight': (boc[-1], boc[-1], 3, 3),
                'mid_block.attentions.0.transformer_blocks.0.attn2.to_k.weight': (boc[-1], self.ctx_dim),
                f'up_blocks.{len(boc) - 1}.resnets.{self.lpb}.conv2.weight': (boc[0], boc[0], 3, 3)}
        for i, c in enumerate(boc):
            want[f'down_blocks.{i}.resnets.{self.lpb - 1}.conv2.weight'] = (c, c, 3, 3)
            if i != len(boc) - 1:
                want[f'down_blocks.{i}.attentions.0.transformer_blocks.0.attn1.to_q.weight'] = (c, c)
            if c % self.heads:
                raise ValueError(f'SDUNet: block_out_channels {boc} do not split into attention_head_dim={self.heads} heads')
        blocks.check_shapes('SDUNet', sd, want, f'block_out_channels={boc}, layers_per_block={self.lpb}',
                            f'block_out_channels={boc}, cross_attention_dim={self.ctx_dim}')
        extra = f'down_blocks.0.resnets.{self.lpb}.conv1.weight'
        if extra in sd:
            raise ValueError(f'SDUNet: the state dict has {extra!r}: more than layers_per_block={self.lpb} resnets per block')

    def _load(self, sd):
        self._check_shapes(sd)
        boc, lpb = self.boc, self.lpb
        p = self._p = blocks.Params(self.device, self.dtype)
        self._tw, self._tb, self._tcols, self._tfm = [], [], 0, []
        half = boc[0] // 2
        self.freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half).to(self.device)    # freq_shift = 0
        self.t1 = (p.f32(sd['time_embedding.linear_1.weight']), p.f32(sd['time_embedding.linear_1.bias']))
        self.t2 = (p.f32(sd['time_embedding.linear_2.weight']), p.f32(sd['time_embedding.linear_2.bias']))
        self.conv_in = p.conv(sd, 'conv_in', pad_in=64)
        self.down = []
        for i, c in enumerate(boc):
            cross = i != len(boc) - 1
            layers = []
            for j in range(lpb):
                layers.append((self._resnet_params(sd, f'down_blocks.{i}.resnets.{j}'),
                               self._transformer_params(sd, f'down_blocks.{i}.attentions.{j}', c) if cross else None))
            ds = None
            if i != len(boc) - 1 and self.downsample == 'strided':
                ds = p.conv(sd, f'down_blocks.{i}.downsamplers.0.conv')              # the plain 3x3 layer [C, 3, 3, C]
            elif i != len(boc) - 1:
                w = ops.stride2_conv_weight(p.f32(sd[f'down_blocks.{i}.downsamplers.0.conv.weight']))
                ds = p.pack(w, p.f32(sd[f'down_blocks.{i}.downsamplers.0.conv.bias']))
            self.down.append((layers, ds))
        self.mid = (self._resnet_params(sd, 'mid_block.resnets.0'), self._transformer_params(sd, 'mid_block.attentions.0', boc[-1]),
                    self._resnet_params(sd, 'mid_block.resnets.1'))
        self.up = []
        rev = boc[::-1]
        for i, c in enumerate(rev):
            cross = i != 0
            layers = []
            for j in range(lpb + 1):
                layers.append((self._resnet_params(sd, f'up_blocks.{i}.resnets.{j}'),
                               self._transformer_params(sd, f'up_blocks.{i}.attentions.{j}', c) if cross else None))
            us = p.conv(sd, f'up_blocks.{i}.upsamplers.0.conv') if i != len(rev) - 1 else None
            self.up.append((layers, us))
        self.out_g, self.out_b = p.norm(sd, 'conv_norm_out')
        self.conv_out = p.conv(sd, 'conv_out', pad_out=64)
        self.tproj = (torch.cat(self._tw, 0).contiguous(), torch.cat(self._tb).contiguous())
        del self._tw, self._tb, self._p
        torch.cuda.synchronize(self.device)

    # ---- forward -------------------------------------------------------------------------------
    def _resnet(self, x, P, temb, skip=None):
        return blocks.resnet(x, P, self.groups, self.eps, bias_nc=temb[:, P.toff:P.toff + P.cout], skip=skip)

    def _transformer(self, x, A, kv, kv_rows):
        """Transformer2DModel.forward with one BasicTransformerBlock (transformer_2d.py, attention.py): tokens stay in NHWC, every
        Linear is a 1x1 convolution with the residual add in its epilogue."""
        n, hh, ww, c = x.shape
        t = hh * ww
        h = ops.group_norm(x, self.groups, 1e-6, A.g, A.b, silu=False)
        h = ops.conv2d(h, A.w_in, A.b_in)
        y = ops.layer_norm(h, *A.ln[0])
        qkv = ops.conv2d(y, A.w_qkv)
        a = ops.attention(qkv.view(n, t, 3 * A.hp), A.heads, A.scale)
        h = ops.conv2d(a.view(n, hh, ww, A.hp), A.w_o1, A.b_o1, residual=h)
        y = ops.layer_norm(h, *A.ln[1])
        q = ops.conv2d(y, A.w_q2)
        a = ops.cross_attention(q.view(n, t, A.hp), kv[A.index], A.heads, A.scale, kv_rows=kv_rows)
        h = ops.conv2d(a.view(n, hh, ww, A.hp), A.w_o2, A.b_o2, residual=h)
        y = ops.layer_norm(h, *A.ln[2])
        f = ops.geglu(ops.conv2d(y, A.w_ff1, A.b_ff1))
        h = ops.conv2d(f, A.w_ff2, A.b_ff2, residual=h)
        return ops.conv2d(h, A.w_out, A.b_out, residual=x, gn_stats=True)

    def _device_forward(self, sample, tt, ctx, kv_rows):
        """The fixed-shape device part of the forward, what self._graphs captures and replays: sample [n, 4, h, w] (float32 or `dtype`),
        tt float32 [n], ctx [G, L, cross_attention_dim] in `dtype` (the DISTINCT contexts), kv_rows int32 [n] with entries in [0, G)
        -> [n, 4, h, w] in `dtype`.  No host read, no shape that depends on data, no copy from host memory."""
        emb = ops.pos_embedding(tt, self.freqs)                                        # cos | sin (flip_sin_to_cos)
        emb = ops.linear(emb, *self.t1, act_out=True)
        emb = ops.linear(emb, *self.t2)
        temb = ops.cast_from_f32(ops.linear(emb, *self.tproj, act_in=True), self.dtype)      # every block's time_emb_proj(silu(emb))
        # The k | v projections of the text tokens for every transformer block: they do not depend on the latents, and the 2N rows of a
        # search step hold two distinct contexts -- projected once per DISTINCT row; dts_cross_attention reads them through the row map.
        G, L, cd = ctx.shape
        ctx = ctx.view(G, L, 1, cd)
        kv = [ops.conv2d(ctx, A.w_kv2).view(G, L, 2 * A.hp) for A in self._tfm]

        x = ops.nchw_to_nhwc_pad(sample.float().contiguous(), self.dtype, 64)
        x = ops.conv2d(x, *self.conv_in, gn_stats=True)
        skips = [x]
        for layers, ds in self.down:
            for P, A in layers:
                x = self._resnet(x, P, temb)
                if A is not None:
                    x = self._transformer(x, A, kv, kv_rows)
                skips.append(x)
            if ds is not None:
                if self.downsample == 'strided':
                    x = ops.conv2d(x, *ds, stride=2, gn_stats=True)
                else:
                    x = ops.conv2d(ops.space_to_depth2(x, self.dtype), *ds, gn_stats=True)
                skips.append(x)
        x = self._resnet(x, self.mid[0], temb)
        x = self._transformer(x, self.mid[1], kv, kv_rows)
        x = self._resnet(x, self.mid[2], temb)
        for layers, us in self.up:
            for P, A in layers:
                x = self._resnet(x, P, temb, skip=skips.pop())
                if A is not None:
                    x = self._transformer(x, A, kv, kv_rows)
            if us is not None:
                x = ops.conv2d(x, *us, up=True, gn_stats=True)                         # Upsample2D: nearest-2x fused into the conv's gather
        h = ops.group_norm(x, self.groups, self.eps, self.out_g, self.out_b, silu=True)
        y = ops.conv2d(h, *self.conv_out)                                              # 4 live output channels of 64
        return y[..., :4].permute(0, 3, 1, 2).contiguous()

    def _timesteps(self, timestep, n):
        """float32 [n] on the device.  A number, a 0-d or a one-element host tensor becomes a fill kernel (no copy from pageable memory); a
        device tensor is converted and broadcast on the device."""
        if torch.is_tensor(timestep) and timestep.is_cuda:
            tt = timestep.to(self.device, torch.float32).reshape(-1)
        elif (timestep.numel() == 1) if torch.is_tensor(timestep) else not hasattr(timestep, '__len__'):
            return torch.full((n,), float(timestep), dtype=torch.float32, device=self.device)
        else:                                                                          # a host tensor / sequence of n values: one upload
            tt = torch.as_tensor(timestep, dtype=torch.float32, device=self.device).reshape(-1)
        if tt.numel() not in (1, n):
            raise ValueError(f'SDUNet: {tt.numel()} timesteps for {n} samples')
        return tt.expand(n).contiguous()

    @torch.no_grad()
    def __call__(self, sample, timestep, encoder_hidden_states=None, return_dict=False, context_rows=None, **unused):
        """sample [n, 4, h, w], timestep a number / 0-d tensor / [n] tensor, encoder_hidden_states [n, L <= 128, cross_attention_dim]
        -> ([n, 4, h, w] in `dtype`,).

        The stock call surface groups identical encoder_hidden_states rows on the device (ops.group_rows) and reads back their number, 4
        bytes: the one host synchronisation of a call.  context_rows (this build's keyword; `takes_context_rows` announces it) removes it:
        encoder_hidden_states then holds the G <= n DISTINCT contexts [G, L, cross_attention_dim] and context_rows -- an int32 [n] device
        tensor, or a sequence of n integers that is uploaded here -- names the context of every sample.  Its VALUES are never read back:
        the caller vouches that they lie in [0, G) (the attention kernel clamps them for memory safety only)."""
        for k, v in unused.items():
            if v is not None:
                raise ValueError(f'SDUNet: argument {k} is not supported (stock SD-1.x call surface only)')
        if encoder_hidden_states is None:
            raise ValueError('SDUNet: encoder_hidden_states is required')
        sample = sample.to(self.device)
        n, cin, hh, ww = sample.shape
        if cin != 4 or hh % 8 or ww % 8:
            raise ValueError(f'SDUNet: sample {tuple(sample.shape)}: 4 channels and a height / width divisible by 8 (three 2x levels)')
        ehs = encoder_hidden_states.to(self.device, self.dtype).contiguous()
        if ehs.dim() != 3 or ehs.shape[2] != self.ctx_dim:
            raise ValueError(f'SDUNet: encoder_hidden_states {tuple(ehs.shape)}: [rows, tokens, {self.ctx_dim}]')
        if context_rows is None:
            if ehs.shape[0] != n:
                raise ValueError(f'SDUNet: {ehs.shape[0]} encoder_hidden_states rows for {n} samples')
            tt = self._timesteps(timestep, n)
            kv_rows, reps, count = ops.group_rows(ehs)
            ctx = ehs.index_select(0, reps[:int(count)])                               # the call's one host synchronisation: 4 bytes
        else:
            if not 1 <= ehs.shape[0] <= n:
                raise ValueError(f'SDUNet: {ehs.shape[0]} distinct contexts for {n} samples (context_rows: 1 .. n of them)')
            if torch.is_tensor(context_rows):
                if context_rows.dtype != torch.int32 or not context_rows.is_cuda:
                    raise ValueError(f'SDUNet: context_rows is an int32 device tensor (or a sequence of integers), got {context_rows.dtype} on {context_rows.device}')
                kv_rows = context_rows.to(self.device).contiguous()
            else:
                kv_rows = torch.tensor([int(r) for r in context_rows], dtype=torch.int32).to(self.device)
            if tuple(kv_rows.shape) != (n,):
                raise ValueError(f'SDUNet: context_rows has shape {tuple(kv_rows.shape)}, expected ({n},)')
            tt = self._timesteps(timestep, n)
            ctx = ehs
        out = self._graphs(sample if sample.dtype == self.dtype else sample.float(), tt, ctx, kv_rows)
        self.rows += n
        if return_dict:
            return types.SimpleNamespace(sample=out)
        return (out,)

    forward = __call__
