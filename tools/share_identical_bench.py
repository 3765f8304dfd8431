#!/usr/bin/env python3
"""`generate_image_grid(share_identical=True)` against the full run, the headline search: `random:adm_imagenet64`, the ImageNet classifier as
scorer, eps-greedy N = 64, K = 4, 18 sigma steps with the CLI's churn settings (sigma steps 0, 1, 15, 16, 17 add no noise), f16x3, one image,
one process.  Host clock around a whole generate_image_grid call (host draws, uploads and bookkeeping included), ending in a device
synchronise.  Each setting is run once before the window (row shapes warmed, HIP graphs captured), then full / shared alternate, `--reps`
times each; the medians and their ratio are reported.  DESIGN.md section 5 holds the figures.

    python tools/share_identical_bench.py [--reps 3] [--steps 18] [out.json]
    python tools/share_identical_bench.py --full-only          # the run without the keyword alone; passes no new keyword, so the same command
                                                               # runs on a tree from before it: parent against head
    python tools/share_identical_bench.py --config3            # the 72 selections of tests/golden/config3_golden.npz (the reference's own run
                                                               # of BASELINE configs[2]): free-running, with and without the keyword
"""
import argparse, json, os, sys, time, warnings
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings('ignore')
from diffusion_tts_amd import sampler as sm, scorers as S, ops
from diffusion_tts_amd.hashing import seed0_scale

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--steps', type=int, default=18)
ap.add_argument('--full-only', action='store_true')
ap.add_argument('--config3', action='store_true')
ap.add_argument('out', nargs='?')
args = ap.parse_args()
dev = torch.device('cuda')
CHURN = dict(S_churn=40, S_min=0.05, S_max=50, S_noise=1.003)
out = dict(steps=args.steps, reps=args.reps)


def config3():
    """the inputs of tests/test_gpu_fullsize.py::test_config3_whole_search_against_the_reference_run, free-running in f16x3"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from helpers import full_weights
    from diffusion_tts_amd.networks import EDMPrecond
    gd = os.path.join(ROOT, 'tests', 'golden')
    gfull, g = np.load(os.path.join(gd, 'fullsize_golden.npz')), np.load(os.path.join(gd, 'config3_golden.npz'))
    with open(os.path.join(gd, 'fullsize_manifest.json')) as f:
        mfull = json.load(f)
    with open(os.path.join(gd, 'config3_manifest.json')) as f:
        m = json.load(f)
    cfg, sd = full_weights(mfull, 'adm_imagenet64')
    ccfg, csd = full_weights(mfull, 'cls_imagenet64')
    net = EDMPrecond(cfg, sd, device=dev, dtype=ops.F16X3)
    scorer = S.ImageNetScorer(weights=csd, cfg=ccfg, device=dev, compute_dtype=ops.F16X3)
    lat = torch.from_numpy(gfull['eg64_latents'])
    lab = torch.eye(1000)[torch.from_numpy(gfull['eg64_label_idx']).long()]
    ref_sel = [int(v) for v in g['selected']]
    runs = {}
    for share in (False, True):
        h = sm.generate_image_grid(net, None, lat, lab, seed=m['seed'], gridw=1, gridh=1, device=dev, num_steps=18,
                                   sampling_method=sm.SamplingMethod.EPS_GREEDY, sampling_params=dict(scorer=scorer, **m['params']),
                                   scale_fn=seed0_scale, compute_dtype=ops.F16X3, verbose=False, share_identical=share, **m['S'])
        own = [int(s_[0]) for s_ in h['selected']]
        diff = np.abs(h['image'][0].permute(1, 2, 0).numpy().astype(np.int32) - g['image'].astype(np.int32))
        runs[share] = h
        rec = dict(net_rows=int(h['net_rows']), shared_steps=h['shared_steps'], selections_equal_to_reference=sum(int(a == b) for a, b in zip(own, ref_sel)),
                   of=len(ref_sel), x_err=float((h['x'].cpu() - torch.from_numpy(g['last_D']).double()).abs().max()), png_pixels_off=int((diff > 0).sum()))
        out['config3_shared' if share else 'config3_full'] = rec
        print(f'config 3, share_identical={share}: {rec}', flush=True)
    a, c = runs[False], runs[True]
    out['config3_shared_equals_full'] = dict(x=bool(torch.equal(a['x'], c['x'])), image=bool(torch.equal(a['image'], c['image'])),
                                             selected=all(torch.equal(p, q) for p, q in zip(a['selected'], c['selected'])))
    print(f'config 3, shared against full (bit-equal): {out["config3_shared_equals_full"]}', flush=True)


def timed(net, scorer, lat, lab, share):
    extra = {} if share is None else dict(share_identical=share)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = sm.generate_image_grid(net, None, lat, lab, seed=0, gridw=1, gridh=1, device=dev, num_steps=args.steps,
                                 sampling_method=sm.SamplingMethod.EPS_GREEDY, scale_fn=seed0_scale, compute_dtype=ops.F16X3, verbose=False,
                                 sampling_params=dict(scorer=scorer, N=64, K=4, lambda_param=0.15, eps=0.4), **CHURN, **extra)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def bench():
    net = sm.load_network('random:adm_imagenet64', device=dev, dtype=ops.F16X3)
    scorer = S.ImageNetScorer(dtype=torch.float32, device=dev, compute_dtype=ops.F16X3)
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(1, 3, 64, 64, generator=g)
    lab = torch.eye(1000)[torch.randint(1000, size=[1], generator=g)]
    settings = [None] if args.full_only else [False, True]                          # None: the call as it was before the keyword
    name = {None: 'full', False: 'full', True: 'shared'}
    last = {}
    for share in settings:                                                         # warm every row shape of every setting, capture the graphs
        timed(net, scorer, lat, lab, share)
    runs = {name[s]: [] for s in settings}
    for rep in range(args.reps):
        for share in settings:
            dt, res = timed(net, scorer, lat, lab, share)
            last[name[share]] = res
            runs[name[share]].append(dt)
            print(f'rep {rep} {name[share]}: {dt:.3f} s, {res["net_rows"]} denoiser rows, {len(res["rewards"])} scorer decisions', flush=True)
    for k, v in runs.items():
        out[k] = dict(runs=v, median_s=float(np.median(v)), spread_s=[min(v), max(v)], net_rows=int(last[k]['net_rows']))
        print(f'{k}: median {np.median(v):.3f} s ({min(v):.3f} - {max(v):.3f}), {last[k]["net_rows"]} rows', flush=True)
    if not args.full_only:
        a, c = last['full'], last['shared']
        out['shared_steps'] = c['shared_steps']
        out['ratio'] = out['shared']['median_s'] / out['full']['median_s']
        out['bit_equal'] = dict(x=bool(torch.equal(a['x'], c['x'])), image=bool(torch.equal(a['image'], c['image'])),
                                selected=all(torch.equal(p, q) for p, q in zip(a['selected'], c['selected'])))
        print(f'shared / full = {out["ratio"]:.3f} (required: at most 0.80); shared steps {c["shared_steps"]}; bit-equal to the full run: {out["bit_equal"]}', flush=True)
    out['graphs'] = net._graphs.path_report()


if args.config3:
    config3()
else:
    bench()
if args.out:
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
if not args.config3 and not args.full_only and out['ratio'] > 0.80:
    sys.exit(f'shared / full = {out["ratio"]:.3f} is above the required 0.80')
