#!/usr/bin/env python3
"""A sigma step of the EDM beam search (B = 4, N = 16, `generate_image_grid(beam_search=True)`) against an eps-greedy N = 64 iteration
(K = 1, the winner's row reused): `random:adm_imagenet64`, the ImageNet classifier as scorer, f16x3, one process, the two alternating.
Both are 128 denoiser rows + 64 scorer images per sigma step.  Six sigma steps per run with the CLI's churn settings; host clock around a
whole run, ending in a device synchronise, divided by the steps.  Then the beam search with every step's noise handed in (no host draw),
the host draw of one step and its upload on their own.  DESIGN.md section 5 holds the figures.

    python tools/beam_step_bench.py [out.json]"""
import json, os, sys, time, warnings
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings('ignore')
from diffusion_tts_amd import sampler as sm, scorers as S, ops
from diffusion_tts_amd.hashing import seed0_scale

dev = torch.device('cuda')
net = sm.load_network('random:adm_imagenet64', device=dev, dtype=ops.F16X3)
scorer = S.ImageNetScorer(dtype=torch.float32, device=dev, compute_dtype=ops.F16X3)
lat = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(1))
lab = torch.eye(1000)[torch.tensor([207])]
STEPS = 6
kw = dict(seed=0, gridw=1, gridh=1, device=dev, num_steps=STEPS, S_churn=40, S_min=0.05, S_max=50, S_noise=1.003, compute_dtype=ops.F16X3, verbose=False)

def beam():
    return sm.generate_image_grid(net, None, lat, lab, sampling_method=sm.SamplingMethod.BEAM_SEARCH, beam_search=True,
                                  sampling_params=dict(scorer=scorer, B=4, N=16), **kw)

def eps():      # K = 1, the winner's row reused: per sigma step exactly one 64-candidate iteration, no batch-1 pivot step
    return sm.generate_image_grid(net, None, lat, lab, sampling_method=sm.SamplingMethod.EPS_GREEDY, reuse_winner=True, scale_fn=seed0_scale,
                                  sampling_params=dict(scorer=scorer, N=64, K=1, lambda_param=0.15, eps=0.4), **kw)

def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); r = fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / STEPS, r

for _ in range(2):                      # warm every shape (eager, eager, capture ...)
    rb = beam(); re_ = eps()
rows = (rb['net_rows'], re_['net_rows'])
tb, te = [], []
for rep in range(7):
    a, _ = timed(beam); b, _ = timed(eps)
    tb.append(a); te.append(b)
    print(f'rep {rep}: beam {a:.2f} ms / sigma step, eps-greedy {b:.2f} ms / iteration', flush=True)
# what the host draws cost: the beam search draws step i + 1 while the GPU runs step i; eps-greedy draws ahead and uploads from pinned memory on a side stream
every = {i: torch.randn(1, 4, 16, 3, 64, 64, dtype=torch.float64) for i in range(STEPS)}
def beam_pre():
    return sm.generate_image_grid(net, None, lat, lab, sampling_method=sm.SamplingMethod.BEAM_SEARCH, beam_search=True,
                                  sampling_params=dict(scorer=scorer, B=4, N=16), precomputed_noise=every, **kw)
beam_pre()
tp, td, tu = [], [], []
for rep in range(5):
    a, _ = timed(beam_pre); tp.append(a)
    t0 = time.perf_counter(); e = torch.stack([torch.randn((16, 3, 64, 64), dtype=torch.float64) for _ in range(4)]); td.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize(); t0 = time.perf_counter(); d = e.reshape(64, 3, 64, 64).to(dev).contiguous(); torch.cuda.synchronize(); tu.append((time.perf_counter() - t0) * 1e3)
print(f'beam without host draws {np.median(tp):.2f} ms / step; host draw of a step {np.median(td):.2f} ms; pageable upload {np.median(tu):.2f} ms', flush=True)
out = dict(beam_no_draws_ms=tp, host_draw_ms=td, upload_ms=tu, rows=rows, steps=STEPS, beam_ms=tb, eps_ms=te, beam_median=float(np.median(tb)), eps_median=float(np.median(te)),
           beam_spread=[min(tb), max(tb)], eps_spread=[min(te), max(te)], graphs=net._graphs.path_report())
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
