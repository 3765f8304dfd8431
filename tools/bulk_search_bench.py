#!/usr/bin/env python3
"""Bulk search (`bulk.generate_seeds`, the path behind `main.py --seeds`): the searches of 16 seeds one after the other (search_batch = 1)
against the same 16 seeds in lock-step as one batch (search_batch = 16), f16x3, one process, the two settings alternating, three repeats:
  a  random:adm_imagenet64, eps-greedy N = 4, K = 4, the ImageNet classifier as scorer (4-row against 64-row denoiser calls)
  b  random:ddpmpp_cifar10, rejection sampling N = 16, brightness (16-row against 256-row calls)
  m  random:adm_imagenet64, MCTS N = 4, S = 16, the ImageNet classifier as scorer: one search per seed (the only MCTS path before
     `mcts_lockstep`, and still the path without it) against search_batch = 16 with mcts_lockstep=True (4-row expansions and 1 .. 16-row
     rollout steps against <= 64-row and <= 256-row ones); the result also holds the histogram of rows per denoiser forward of both settings
     (padding rows included: what was launched), the input of the cost-model prediction in DESIGN.md section 5
with the CLI's churn settings.  Host clock around a whole generate_seeds call (host draws, PNG writing and per-seed bookkeeping included),
ending in a device synchronise.  Every setting is run once before the window: each row shape has then been through its eager calls and its HIP
graph is captured.  Reports images/s and candidate evaluations (denoiser rows) per second.  DESIGN.md section 5 holds the figures.

    python tools/bulk_search_bench.py [--case a|b|m] [--search-batch 1] [--steps 6] [--seeds 16] [--reps 3] [--lockstep-only] [out.json]

`--search-batch 1` measures the sequential setting alone and passes no search_batch keyword: that command also runs on a tree from before the
keyword, which is how the unchanged path is compared with its parent (for case m: the parent's only MCTS path).  `--lockstep-only`
measures the batched setting alone."""
import argparse, json, os, sys, tempfile, time, warnings
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings('ignore')
from diffusion_tts_amd import bulk, sampler as sm, scorers as S, ops
from diffusion_tts_amd.hashing import seed0_scale

ap = argparse.ArgumentParser()
ap.add_argument('--case', default='ab')
ap.add_argument('--search-batch', type=int, default=None, help='1: the sequential setting alone, no new keyword; default: 1 against 16')
ap.add_argument('--steps', type=int, default=6)
ap.add_argument('--seeds', type=int, default=16)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--lockstep-only', action='store_true', help='the batched setting alone')
ap.add_argument('out', nargs='?')
args = ap.parse_args()
dev = torch.device('cuda')
seeds = f'0-{args.seeds - 1}'
kw = dict(device=dev, compute_dtype=ops.F16X3, num_steps=args.steps, S_churn=40, S_min=0.05, S_max=50, S_noise=1.003)
outdir = tempfile.mkdtemp(prefix='bulk_search_bench_')


def case_a():
    net = sm.load_network('random:adm_imagenet64', device=dev, dtype=ops.F16X3)
    scorer = S.ImageNetScorer(dtype=torch.float32, device=dev, compute_dtype=ops.F16X3)
    return net, dict(sampling_method=sm.SamplingMethod.EPS_GREEDY, scale_fn=seed0_scale,
                     sampling_params=dict(scorer=scorer, N=4, K=4, lambda_param=0.15, eps=0.4))


def case_b():
    net = sm.load_network('random:ddpmpp_cifar10', device=dev, dtype=ops.F16X3)
    return net, dict(sampling_method=sm.SamplingMethod.REJECTION_SAMPLING, sampling_params=dict(scorer=S.BrightnessScorer(), N=16))


def case_m():
    net = sm.load_network('random:adm_imagenet64', device=dev, dtype=ops.F16X3)
    scorer = S.ImageNetScorer(dtype=torch.float32, device=dev, compute_dtype=ops.F16X3)
    return net, dict(sampling_method=sm.SamplingMethod.MCTS, sampling_params=dict(scorer=scorer, N=4, S=16))


class RowHistogram:
    """counts the denoiser forwards of a network by their row count (GraphCache.__call__ sees every forward, padded rows included)"""

    def __init__(self, net):
        self.rows, self.cache, self.inner = {}, net._graphs, net._graphs.__class__.__call__

    def __enter__(self):
        def counted(cache, *inputs):
            if cache is self.cache:
                self.rows[inputs[0].shape[0]] = self.rows.get(inputs[0].shape[0], 0) + 1
            return self.inner(cache, *inputs)
        self.cache.__class__.__call__ = counted
        return self

    def __exit__(self, *exc):
        self.cache.__class__.__call__ = self.inner


def timed(net, how, search_batch):
    extra = {} if search_batch is None else dict(search_batch=search_batch)
    if how['sampling_method'] == sm.SamplingMethod.MCTS and search_batch not in (None, 1):
        extra['mcts_lockstep'] = True
    torch.cuda.synchronize(); t0 = time.perf_counter()
    done = bulk.generate_seeds(net, seeds, outdir, **how, **kw, **extra)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, len(done), sum(r['net_rows'] for r in done.values())


settings = [None] if args.search_batch == 1 else [1, args.search_batch or 16]       # None: the call as it was before the keyword
if args.lockstep_only:
    settings = [args.search_batch or 16]
out = dict(steps=args.steps, seeds=args.seeds, reps=args.reps)
for name, make in (('a', case_a), ('b', case_b), ('m', case_m)):
    if name not in args.case:
        continue
    net, how = make()
    histograms = {}
    for sb in settings:                                                            # warm every row shape of every setting, capture the graphs
        with RowHistogram(net) as h:
            timed(net, how, sb)
        histograms[str(sb or 1)] = {str(k): v for k, v in sorted(h.rows.items())}
    runs = {str(sb or 1): [] for sb in settings}
    for rep in range(args.reps):
        for sb in settings:
            dt, images, rows = timed(net, how, sb)
            runs[str(sb or 1)].append(dict(s=dt, images_per_s=images / dt, evals_per_s=rows / dt))
            print(f'case {name} rep {rep} search_batch {sb or 1}: {dt:.3f} s, {images / dt:.2f} images/s, {rows / dt:.0f} candidate evaluations/s', flush=True)
    res = {}
    for sb, rs in runs.items():
        ips = [r['images_per_s'] for r in rs]
        res[sb] = dict(runs=rs, images_per_s_median=float(np.median(ips)), images_per_s_spread=[min(ips), max(ips)],
                       evals_per_s_median=float(np.median([r['evals_per_s'] for r in rs])))
    if len(res) == 2:
        lo, hi = (res[str(sb)]['images_per_s_median'] for sb in settings)
        res['ratio'] = hi / lo
        print(f'case {name}: search_batch {settings[1]} runs at {hi / lo:.2f} x the sequential run', flush=True)
    res['graphs'] = net._graphs.path_report()
    if name == 'm':
        res['forward_rows_histogram'] = histograms
        res['lockstep_pad_rows'] = sm.__dict__.get('MCTS_LOCKSTEP_PAD_ROWS')
    out[name] = res
    del net, how
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
