"""The SD VAE decoder on the HIP kernels: drop-in for the `vae` object of the SD search loop (`vae.decode(z, return_dict=False)[0]`,
`vae.config.scaling_factor`), i.e. for `AutoencoderKL.decode` of the vendored diffusers
(sd/diffusers/src/diffusers/models/autoencoders/autoencoder_kl.py:287-320, vae.py:204-323 `Decoder`).

Decoding is the largest single cost of an SD candidate (2.48 TFLOP per 512x512 image) and the reference decodes
the candidates of an iteration one at a time; here all N go through as one batch, on the same kernels as the EDM path:
  3x3 / 1x1 convs           -> dts_conv2d (implicit GEMM on MFMA; nearest-2x upsample fused into the gather; residual add in the epilogue)
  GroupNorm(32, eps 1e-6)+SiLU -> dts_gn_* (statistics fused into the producing conv's epilogue where possible)
  mid-block attention       -> dts_attention (one head of dim 512: two 256-wide value slices)
  conv_out (128 -> 3)       -> dts_conv_out3
Activations are NHWC in `dtype` (float16 like the reference pipeline, or bfloat16); the 4 latent channels are zero-padded to 64 for
the MFMA conv (cin % 64 == 0).  Parameters: a state dict with diffusers' key names (`AutoencoderKL.state_dict()` / the safetensors
file of SD-1.5's vae/).  Stock configuration only: group norm, SiLU, one attention in the mid block, UpDecoderBlock2D.
"""
import math
import types

import torch

from . import blocks, ops


class VAEDecoder:
    def __init__(self, state_dict, block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4, norm_num_groups=32,
                 scaling_factor=0.18215, device='cuda', dtype=torch.float16):
        blocks.require_gpu('VAEDecoder')
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError('VAEDecoder: activations are float16 or bfloat16 (head dim 512 attention is 16-bit only)')
        self.device, self.dtype = torch.device(device), dtype
        self.boc, self.lpb, self.groups, self.lat = tuple(block_out_channels), layers_per_block, norm_num_groups, latent_channels
        self.config = types.SimpleNamespace(scaling_factor=scaling_factor, block_out_channels=list(block_out_channels),
                                            latent_channels=latent_channels, force_upcast=False)
        self.decodes = 0
        self._load(state_dict)

    @classmethod
    def from_pretrained(cls, path, device='cuda', dtype=torch.float16):
        """Reads a diffusers `vae/` directory (or a single `.safetensors` file): `config.json` for the shape and
        `diffusion_pytorch_model[.fp16].safetensors` for the parameters -- the on-disk format of SD-1.5's VAE.
        Only the decoder half (`decoder.*`, `post_quant_conv.*`) is read; tensors are loaded lazily, so the encoder never leaves disk."""
        import json
        import os
        cfg = {}
        if os.path.isdir(path):
            cfg_file = os.path.join(path, 'config.json')
            if os.path.exists(cfg_file):
                with open(cfg_file) as f:
                    cfg = json.load(f)
            path = blocks.diffusers_weights(path)
        for key, want in (('act_fn', 'silu'), ('_class_name', 'AutoencoderKL')):
            if key in cfg and cfg[key] != want:
                raise ValueError(f'VAEDecoder: {key}={cfg[key]!r} is not the stock SD VAE ({want!r})')
        for t in cfg.get('up_block_types', []):
            if t != 'UpDecoderBlock2D':
                raise ValueError(f'VAEDecoder: up block {t!r} unsupported')
        sd = blocks.read_tensors(path, lambda keys: {k: k for k in keys if k.startswith(('decoder.', 'post_quant_conv.'))}, 'decoder.*')
        kw = {k: cfg[k] for k in ('layers_per_block', 'latent_channels', 'norm_num_groups', 'scaling_factor') if k in cfg}
        if 'block_out_channels' in cfg:
            kw['block_out_channels'] = tuple(cfg['block_out_channels'])
        return cls(sd, device=device, dtype=dtype, **kw)

    # ------------------------------------------------------------------------------------------
    def _load(self, sd):
        p = blocks.Params(self.device, self.dtype)
        self.pq = p.conv(sd, 'post_quant_conv', pad_in=64, pad_out=64) if 'post_quant_conv.weight' in sd else None
        self.conv_in = p.conv(sd, 'decoder.conv_in', pad_in=64)
        self.mid0 = blocks.resnet_params(p, sd, 'decoder.mid_block.resnets.0')
        self.mid1 = blocks.resnet_params(p, sd, 'decoder.mid_block.resnets.1')
        a = 'decoder.mid_block.attentions.0'
        A = types.SimpleNamespace()
        A.g, A.b = p.norm(sd, a + '.group_norm')
        A.wqkv, A.bqkv = p.qkv(sd, a, ('to_q', 'to_k', 'to_v'))                                                      # q | k | v blocks
        A.wo, A.bo = p.conv(sd, a + '.to_out.0')
        self.attn = A
        self.up = []
        for i in range(len(self.boc)):
            res = [blocks.resnet_params(p, sd, f'decoder.up_blocks.{i}.resnets.{j}') for j in range(self.lpb + 1)]
            ups = p.conv(sd, f'decoder.up_blocks.{i}.upsamplers.0.conv') if i != len(self.boc) - 1 else None
            self.up.append((res, ups))
        self.out_g, self.out_b = p.norm(sd, 'decoder.conv_norm_out')
        self.out_w = p.f32(sd['decoder.conv_out.weight']).permute(0, 2, 3, 1).contiguous()         # [3][kh][kw][c]
        self.out_cb = p.f32(sd['decoder.conv_out.bias'])
        torch.cuda.synchronize(self.device)

    # ------------------------------------------------------------------------------------------
    def _attention(self, x):
        """AttnProcessor2_0 on [n, hw, c]: group norm, fused q|k|v projection, one head of dim c, output projection + residual."""
        A = self.attn
        n, hh, ww, c = x.shape
        hn = ops.group_norm(x, self.groups, 1e-6, A.g, A.b, silu=False)
        qkv = ops.conv2d(hn, A.wqkv, A.bqkv)
        o = ops.attention(qkv.view(n, hh * ww, 3 * c), 1, 1.0 / math.sqrt(c))
        return ops.conv2d(o.view(n, hh, ww, c), A.wo, A.bo, residual=x, gn_stats=True)

    @torch.no_grad()
    def decode(self, z, return_dict=False, generator=None):
        """z [n, latent_channels, h, w] (already divided by the scaling factor by the caller, pipeline...:1112) -> ([n, 3, 8h, 8w],)."""
        z = z.to(self.device)
        n = z.shape[0]
        x = ops.nchw_to_nhwc_pad(z.float().contiguous(), self.dtype, 64)
        if self.pq is not None:
            x = ops.conv2d(x, self.pq[0], self.pq[1])                           # 1x1 on the 4 (of 64) live channels
        x = ops.conv2d(x, self.conv_in[0], self.conv_in[1], gn_stats=True)
        x = blocks.resnet(x, self.mid0, self.groups, 1e-6)                      # ResnetBlock2D with temb None
        x = self._attention(x)
        x = blocks.resnet(x, self.mid1, self.groups, 1e-6)
        for res, ups in self.up:
            for P in res:
                x = blocks.resnet(x, P, self.groups, 1e-6)
            if ups is not None:
                x = ops.conv2d(x, ups[0], ups[1], up=True, gn_stats=True)       # nearest-2x fused into the conv's gather
        h = ops.group_norm(x, self.groups, 1e-6, self.out_g, self.out_b, silu=True)
        img = ops.conv_out3(h, self.out_w, self.out_cb).to(self.dtype)
        self.decodes += n
        if return_dict:
            return types.SimpleNamespace(sample=img)
        return (img,)
