#!/usr/bin/env python3
"""Golden vectors for the SD U-Net: the REFERENCE's vendored `UNet2DConditionModel.forward` (sd/diffusers/src/diffusers/models/unets/
unet_2d_condition.py) on CPU, fp32, for a narrow model -- block_out_channels (64, 128, 192, 192), 2 heads (head dims 32 / 64 / 96: one is
not a power of two), text width 64, 11 tokens -- and for SD-1.5's own configuration (320, 640, 1280, 1280), 8 heads, [2, 77, 768] context,
with the weights of the product's own seeded initialiser (diffusion_tts_amd.init.sd_unet_state_dict) loaded into the reference module
with strict=True, so that nothing but inputs, outputs and a weight checksum is stored.

The manifest also records, per case, measured here:
  (a) the reference module's OWN error when it runs in float16 / bfloat16 on the CPU, against its fp32 output, as max|d| / max|y|: the
      yardstick of the GPU test (tolerance = 3 x this figure);
  (b) the same relative change of the fp32 output when the two context rows are swapped, and
  (c) when both timesteps are shifted by 20: what a model that ignored the text or the time would get wrong.  The initialiser's gains
      must keep (b) and (c) at least 5 x the largest tolerance; asserted below.
and the reference state dict's key names and shapes.
Run: PYTHONHASHSEED=0 python tests/golden/make_golden_sd_unet.py   (needs the reference checkout, $DTS_REFERENCE).
Writes tests/golden/sd_unet_golden.npz and sd_unet_manifest.json."""
import importlib.util
import json
import os
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np
import torch

warnings.simplefilter('ignore')
import transformers
import transformers.utils
transformers.utils.FLAX_WEIGHTS_NAME = 'flax_model.msgpack'
REF = os.environ.get('DTS_REFERENCE', '/root/reference')
spec = importlib.util.spec_from_file_location('diffusers', os.path.join(REF, 'sd/diffusers/src/diffusers/__init__.py'))
sys.modules['diffusers'] = importlib.util.module_from_spec(spec)
spec.loader.exec_module(sys.modules['diffusers'])
from diffusers import UNet2DConditionModel                             # noqa: E402

from diffusion_tts_amd import init as dinit                            # noqa: E402

CASES = {'narrow': dict(boc=(64, 128, 192, 192), heads=2, ctx_dim=64, ctx_len=11, latent=(2, 4, 16, 16), timesteps=[801, 40], seed=11),
         'sd15': dict(boc=(320, 640, 1280, 1280), heads=8, ctx_dim=768, ctx_len=77, latent=(2, 4, 16, 16), timesteps=[981, 21], seed=12)}
TOL_FACTOR, MARGIN = 3.0, 5.0


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def main():
    torch.set_num_threads(8)
    out, manifest = {}, {'tolerance_factor': TOL_FACTOR, 'sensitivity_margin': MARGIN, 'cases': {}}
    for name, c in CASES.items():
        unet = UNet2DConditionModel(sample_size=c['latent'][-1], block_out_channels=c['boc'], attention_head_dim=c['heads'],
                                    cross_attention_dim=c['ctx_dim']).eval()
        sd = dinit.sd_unet_state_dict(c['boc'], c['heads'], c['ctx_dim'], 2, seed=c['seed'])
        unet.load_state_dict(sd, strict=True)
        g = torch.Generator().manual_seed(c['seed'] + 100)
        x = torch.randn(c['latent'], generator=g)
        ctx = torch.randn(c['latent'][0], c['ctx_len'], c['ctx_dim'], generator=g)
        t = torch.tensor(c['timesteps'])
        with torch.no_grad():
            y = unet(x, t, encoder_hidden_states=ctx, return_dict=False)[0]
            y_swap = unet(x, t, encoder_hidden_states=ctx.flip(0), return_dict=False)[0]
            y_time = unet(x, t - 20, encoder_hidden_states=ctx, return_dict=False)[0]
            own = {}
            for dn, dt in (('float16', torch.float16), ('bfloat16', torch.bfloat16)):
                u16 = unet.to(dt)
                own[dn] = rel(u16(x.to(dt), t, encoder_hidden_states=ctx.to(dt), return_dict=False)[0].float(), y)
                unet.to(torch.float32)
                unet.load_state_dict(sd, strict=True)                  # the fp32 parameters again, not their 16-bit roundings
        m = dict(block_out_channels=list(c['boc']), heads=c['heads'], cross_attention_dim=c['ctx_dim'], context_len=c['ctx_len'],
                 latent=list(c['latent']), timesteps=c['timesteps'], seed=c['seed'], own_error=own, context_swap_change=rel(y_swap, y),
                 timestep_shift_change=rel(y_time, y), output_absmax=float(y.abs().max()), output_std=float(y.std()),
                 checksum=dinit.checksum(sd), state_dict=[[k, list(v.shape)] for k, v in unet.state_dict().items()])
        print(name, tuple(y.shape), {k: (v if not isinstance(v, list) else '...') for k, v in m.items() if k not in ('state_dict',)})
        worst_tol = TOL_FACTOR * max(own.values())
        assert m['context_swap_change'] >= MARGIN * worst_tol, (name, 'context', m['context_swap_change'], worst_tol)
        assert m['timestep_shift_change'] >= MARGIN * worst_tol, (name, 'timestep', m['timestep_shift_change'], worst_tol)
        manifest['cases'][name] = m
        out[f'{name}_x'], out[f'{name}_context'], out[f'{name}_t'], out[f'{name}_y'] = x.numpy(), ctx.numpy(), t.numpy(), y.numpy()
    np.savez_compressed(os.path.join(HERE, 'sd_unet_golden.npz'), **out)
    with open(os.path.join(HERE, 'sd_unet_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1)


if __name__ == '__main__':
    main()
