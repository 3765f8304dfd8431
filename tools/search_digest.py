#!/usr/bin/env python3
"""Digests of the EDM searches, for comparing two commits bit for bit: run this file on a checkout of each and diff the two outputs.

It uses the public surface only (generate_image_grid, plain.edm_sampler, bulk.generate_seeds), so the same file runs on an older tree.  Settings:
the tiny 16x16 networks of tests/golden/manifest.json, 4 sigma steps with S_churn=40, S_min=0.05, S_max=50, S_noise=1.003, hashing.seed0_scale,
the brightness scorer, float32 and f16x3, latents and labels from bulk.seed_inputs.  One JSON line per case: sha256 (first 16 hex digits) of
`x`, `image`, every tensor of `rewards`, `selected`, `beam_parents` and `best_noises`, then `net_rows`, `collectives`, `shared_steps` and the
state of torch's (and numpy's) global generator after the call.  The last line counts the cases.

    python tools/search_digest.py [out.jsonl]
"""
import hashlib, json, os, sys, tempfile, warnings
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings('ignore')
from diffusion_tts_amd import bulk, init as dinit, plain, sampler as sm, scorers as S
from diffusion_tts_amd.config import EDMConfig
from diffusion_tts_amd.hashing import seed0_scale
from diffusion_tts_amd.networks import EDMPrecond

DEV = torch.device('cuda')
STEPS = 4
CHURN = dict(S_churn=40, S_min=0.05, S_max=50, S_noise=1.003)
SEEDS = [0, 5, 7]
M = sm.SamplingMethod
LOCAL = dict(N=3, K=2, lambda_param=0.15)
METHODS = {                                  # name: (method, params, keywords, network)
    'naive': (M.NAIVE, {}, {}, 'adm_tiny'),
    'rejection': (M.REJECTION_SAMPLING, dict(N=4), {}, 'ddpmpp_tiny'),
    'eps_greedy': (M.EPS_GREEDY, dict(eps=0.4, **LOCAL), {}, 'adm_tiny'),
    'zero_order': (M.ZERO_ORDER, dict(eps=0.0, **LOCAL), {}, 'adm_tiny'),
    'beam': (M.BEAM_SEARCH, dict(B=2, N=3), dict(beam_search=True), 'adm_tiny'),
    'mcts': (M.MCTS, dict(N=2, S=2), {}, 'adm_tiny'),
}
with open(os.path.join(ROOT, 'tests', 'golden', 'manifest.json')) as f:
    MANIFEST = json.load(f)
_nets, lines = {}, []


def net_of(name, dtype):
    if (name, dtype) not in _nets:
        cfg = EDMConfig(**MANIFEST[name]['cfg'])
        sd, _ = dinit.refill_degenerate(dinit.edm_state_dict(cfg, MANIFEST['net_seed']), MANIFEST['net_seed'])
        _nets[(name, dtype)] = EDMPrecond(cfg, sd, device=DEV, dtype=dtype)
    return _nets[(name, dtype)]


def sha(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous()
        return hashlib.sha256(f'{t.dtype}{tuple(t.shape)}'.encode() + t.numpy().tobytes()).hexdigest()[:16]
    return hashlib.sha256(t).hexdigest()[:16]


def emit(case, **fields):
    fields.update(torch_rng=sha(torch.get_rng_state()), numpy_rng=sha(np.random.get_state()[1].tobytes()))
    lines.append(json.dumps(dict(case=case, **fields)))
    print(lines[-1], flush=True)


def digest(res):
    return dict(x=sha(res['x']), image=sha(res['image']), rewards=[sha(r) for r in res['rewards']], selected=[sha(s_) for s_ in res['selected']],
                beam_parents=[sha(b) for b in res['beam_parents']], best_noises={str(i): sha(v) for i, v in sorted(res['best_noises'].items())},
                net_rows=int(res['net_rows']), collectives=int(res['collectives']), shared_steps=list(res['shared_steps']))


def inputs(net, seeds):
    pairs = [bulk.seed_inputs(s, net) for s in seeds]
    return torch.cat([p[0] for p in pairs]), (None if pairs[0][1] is None else torch.cat([p[1] for p in pairs]))


def search(name, dtype, seeds, row_seeds, tag='', **extra):
    """one generate_image_grid call over the images of `seeds`: the shared stream seed=seeds[0], or row_seeds=seeds"""
    method, params, kw, netname = METHODS[name]
    net = net_of(netname, dtype)
    lat, lab = inputs(net, seeds)
    np.random.seed(0)
    how = dict(row_seeds=list(seeds)) if row_seeds else dict(seed=seeds[0])
    res = sm.generate_image_grid(net, None, lat, lab, gridw=len(seeds), gridh=1, device=DEV, num_steps=STEPS, sampling_method=method,
                                 sampling_params=dict(scorer=S.BrightnessScorer(), **params), scale_fn=seed0_scale, compute_dtype=dtype,
                                 verbose=False, **CHURN, **kw, **how, **extra)
    emit(f'{name} {dtype} {"row_seeds" if row_seeds else "seed"}={seeds}{" " + tag if tag else ""}', **digest(res))
    return res


def noise(shape, seed=11):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


for dtype in (torch.float32, 'f16x3'):
    for name in METHODS:
        for seeds, row_seeds in (([5], False), (SEEDS, False), ([5], True), (SEEDS, True)):
            if row_seeds and name == 'mcts':
                continue                                                            # refused by name
            res = search(name, dtype, seeds, row_seeds)
            if name == 'eps_greedy' and len(seeds) > 1 and not row_seeds:
                # the shared stream with winners that differ between the images: the rebuilt pivot takes a row per image
                assert any(len(set(s_.tolist())) > 1 for s_ in res['selected']), [s_.tolist() for s_ in res['selected']]
            if name in ('eps_greedy', 'zero_order'):
                for tag, extra in (('share', dict(share_identical=True)), ('chunk1', dict(candidate_chunk=1)), ('record', dict(record_noises=True)),
                                   ('reuse', dict(reuse_winner=True)), ('no-reuse', dict(reuse_winner=False)),
                                   ('share+record+reuse', dict(share_identical=True, record_noises=True, reuse_winner=True))):
                    search(name, dtype, seeds, row_seeds, tag, **extra)
                if not row_seeds:
                    pre = {1: noise((len(seeds), 2, 3, 3, 16, 16)), 'pivot_2': noise((len(seeds), 3, 16, 16), 12)}
                    search(name, dtype, seeds, False, 'precomputed', precomputed_noise=pre)
                if not row_seeds and len(seeds) == 1:
                    forced = [1, 0, 2, 1, 0, 2, 1, 0]
                    search(name, dtype, seeds, False, 'forced', forced_selections=forced)
                    search(name, dtype, seeds, False, 'forced+share+record', forced_selections=forced, share_identical=True, record_noises=True)
            if name == 'beam':
                search(name, dtype, seeds, row_seeds, 'share', share_identical=True)
                if not row_seeds:
                    search(name, dtype, seeds, False, 'precomputed', precomputed_noise={1: noise((len(seeds), 2, 3, 3, 16, 16))})
    # outside generate_image_grid: the plain sampler over per-row generators, and bulk mode in lock-step pairs with its PNG files
    net = net_of('adm_tiny', dtype)
    for churn in ({}, CHURN):
        rnd, lat, lab = bulk.batch_inputs(SEEDS, net)
        rows0 = net.evals
        x = plain.edm_sampler(net, lat, lab, randn_like=rnd.randn_like, num_steps=STEPS, **churn)
        emit(f'edm_sampler {dtype} seeds={SEEDS} churn={bool(churn)}', x=sha(x), net_rows=int(net.evals - rows0))
    with tempfile.TemporaryDirectory() as out:
        method, params, _, _ = METHODS['eps_greedy']
        done = bulk.generate_seeds(net, '0-4', out, sampling_method=method, sampling_params=dict(scorer=S.BrightnessScorer(), **params), device='cuda',
                                   compute_dtype=dtype, num_steps=STEPS, scale_fn=seed0_scale, search_batch=2, rank=0, world=1, **CHURN)
        for s in sorted(done):
            with open(os.path.join(out, f'{s:06d}.png'), 'rb') as f:
                emit(f'bulk search_batch=2 {dtype} seed {s}', png=sha(f.read()), row_seeds=done[s]['row_seeds'], **digest(done[s]))
print(json.dumps(dict(cases=len(lines))), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        f.write('\n'.join(lines) + '\n')
