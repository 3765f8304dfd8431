"""GPU: the searches of several seeds in lock-step as one batch -- `generate_image_grid(row_seeds=...)` and `bulk.generate_seeds(search_batch=...)`.

The yardstick is the reference's CPU restatement run ONE SEED AT A TIME (oracle.sampler.search(seed=s); tests/beam_reference.beam_search for the
beam), never this build's own batched run.  Settings: the tiny 16x16 networks of tests/golden/manifest.json, 4 sigma steps with S_churn=40,
S_min=0.05, S_max=50, S_noise=1.003, hashing.seed0_scale, the brightness scorer, latents and labels from bulk.seed_inputs.  Bounds are the
project's: rewards within 5e-5 of the reference and the final state within 1e-3 (tests/test_gpu_search.py); a decision is checkable when its
top-2 gap is 0 or above 4e-5 (helpers.MARGIN / check_decisions) -- the seeds used here have only such decisions (for eps-greedy N=3, K=2 each
seed has 4 exact ties, the gamma = 0 steps, and 4 gaps of 1.79e-4 or more), which is ASSERTED, so nothing passes by being skipped; the same
search under different launch forms (a row in a batch of 4 against the one-image call): rewards 2e-6, final state 1e-5
(tests/test_gpu_sharded.py); PNGs: max difference 1 on fewer than 5e-3 of the pixels (tests/test_gpu_beam.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import beam_reference as br                                                     # noqa: E402
from conftest import ROOT                                                       # noqa: E402
from helpers import tiny_edm, oracle_net, check_decisions, MARGIN               # noqa: E402
from oracle import sampler as osamp, scorers as oscore                          # noqa: E402
from diffusion_tts_amd.hashing import seed0_scale                               # noqa: E402

DEV = 'cuda'
X3 = 'f16x3'
DTYPES = [torch.float32, X3]
REWARD_ATOL, IMG_TOL = 5e-5, 1e-3            # against the reference (tests/test_gpu_search.py)
FORM_REWARD, FORM_X = 2e-6, 1e-5             # the same search under other launch forms (tests/test_gpu_sharded.py)
STEPS = 4
CHURN = dict(S_churn=40, S_min=0.05, S_max=50, S_noise=1.003)
SEEDS = [0, 5, 7, 2]
EPS = dict(N=3, K=2, lambda_param=0.15, eps=0.4)

_NETS, _ORACLE, _SOLO = {}, {}, {}


def hip_net(manifest, name, dtype):
    from diffusion_tts_amd.networks import EDMPrecond
    if (name, dtype) not in _NETS:
        cfg, sd = tiny_edm(manifest, name)
        _NETS[(name, dtype)] = EDMPrecond(cfg, sd, device=DEV, dtype=dtype)
    return _NETS[(name, dtype)]


def inputs(net, seeds):
    from diffusion_tts_amd import bulk
    pairs = [bulk.seed_inputs(s, net) for s in seeds]
    return torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])


def oracle_run(manifest, name, method, seed):
    """the reference's restatement of ONE seed's search on the CPU: computed once, shared, left unchanged; (result, denoiser rows)"""
    key = (name, method, seed)
    if key not in _ORACLE:
        cfg, sd = tiny_edm(manifest, name)
        net = oracle_net(cfg, sd)
        lat, lab = inputs(net, [seed])
        rows0 = net.evals
        if method == 'beam':
            o = br.beam_search(net, lat, lab, B=2, N=3, scorer=oscore.BrightnessOracle(), seed=seed, num_steps=STEPS, **CHURN)
        else:
            params = {'eps_greedy': EPS, 'rejection': dict(N=4), 'naive': {}}[method]
            o = osamp.search(net, lat, lab, method=method, params=dict(scorer=oscore.BrightnessOracle(), **params), seed=seed, num_steps=STEPS,
                             scale_fn=seed0_scale, **CHURN)
        _ORACLE[key] = (o, net.evals - rows0)
    return _ORACLE[key]


def hip_run(manifest, name, method, dtype, seeds=None, seed=None, **extra):
    """row_seeds=seeds (one lock-step batch) or the one-image call seed=seed"""
    from diffusion_tts_amd import sampler as sm, scorers as S
    net = hip_net(manifest, name, dtype)
    M = sm.SamplingMethod
    how = {'eps_greedy': (M.EPS_GREEDY, EPS, {}), 'rejection': (M.REJECTION_SAMPLING, dict(N=4), {}), 'naive': (M.NAIVE, {}, {}),
           'beam': (M.BEAM_SEARCH, dict(B=2, N=3), dict(beam_search=True))}[method]
    lat, lab = inputs(net, seeds if seeds is not None else [seed])
    kw = dict(row_seeds=list(seeds)) if seeds is not None else dict(seed=seed)
    return sm.generate_image_grid(net, None, lat, lab, gridw=lat.shape[0], gridh=1, device=torch.device(DEV), num_steps=STEPS,
                                  sampling_method=how[0], sampling_params=dict(scorer=S.BrightnessScorer(), **how[1]), scale_fn=seed0_scale,
                                  compute_dtype=dtype, verbose=False, **CHURN, **how[2], **kw, **extra)


def solo_run(manifest, name, method, dtype, seed):
    key = (name, method, str(dtype), seed)
    if key not in _SOLO:
        _SOLO[key] = hip_run(manifest, name, method, dtype, seed=seed)
    return _SOLO[key]


def image_rewards(res, method, b):
    """image b's rewards of every scorer call as flat vectors (eps-greedy [N, B]; rejection [B, N]; beam [S, B*N])"""
    return [(r[:, b] if method == 'eps_greedy' else r[b]).reshape(-1).float() for r in res['rewards']]


def no_unchecked(report):
    assert "'sub-noise': 0" in report and "'diverged-after': 0" in report, report


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name,method', [('adm_tiny', 'eps_greedy'), ('ddpmpp_tiny', 'rejection')])
def test_local_search_and_rejection_in_lock_step(manifest, name, method, dtype):
    res = hip_run(manifest, name, method, dtype, seeds=SEEDS)
    assert res['row_seeds'] == SEEDS and res['net_rows'] % len(SEEDS) == 0
    if method == 'eps_greedy':
        assert all(tuple(r.shape) == (3, len(SEEDS)) for r in res['rewards']) and len(res['rewards']) == STEPS * 2
    for b, s in enumerate(SEEDS):
        o, rows = oracle_run(manifest, name, method, s)
        what = f'{name} {method} {dtype} seed {s}'
        mine = image_rewards(res, method, b)
        assert len(mine) == len(o['rewards'])
        for j, (got, ref) in enumerate(zip(mine, o['rewards'])):
            dev = float((got - ref.reshape(-1).float()).abs().max())
            assert dev < REWARD_ATOL, (what, j, dev)
        same, report = check_decisions([r.reshape(-1, 1) for r in o['rewards']], o['selected'], [sel[b:b + 1] for sel in res['selected']], what)
        assert same
        no_unchecked(report)
        if method == 'eps_greedy':
            assert "'tie': 4" in report and "'safe': 4" in report, report
        x_err = float((res['x'][b].cpu() - o['x'][0]).abs().max())
        print(f'{what}: max |x - x_ref| = {x_err:.2e}')
        assert x_err < IMG_TOL, what
        assert res['net_rows'] // len(SEEDS) == rows, what
        one = solo_run(manifest, name, method, dtype, s)                            # this build's own one-image call: other launch forms only
        assert one['net_rows'] == rows
        for j, (got, ref) in enumerate(zip(mine, image_rewards(one, method, 0))):
            assert float((got - ref).abs().max()) <= FORM_REWARD, (what, j)
        assert all(torch.equal(a[b:b + 1], c) for a, c in zip(res['selected'], one['selected'])), what
        assert float((res['x'][b] - one['x'][0]).abs().max()) < FORM_X, what


@pytest.mark.parametrize('dtype', DTYPES)
def test_beam_search_in_lock_step(manifest, dtype):
    B, N = 2, 3
    res = hip_run(manifest, 'adm_tiny', 'beam', dtype, seeds=SEEDS)
    assert len(res['rewards']) == len(res['selected']) == len(res['beam_parents']) == STEPS
    for b, s in enumerate(SEEDS):
        o, rows = oracle_run(manifest, 'adm_tiny', 'beam', s)
        one = solo_run(manifest, 'adm_tiny', 'beam', dtype, s)
        what = f'beam {dtype} seed {s}'
        for i in range(STEPS):
            ref, got = o['rewards'][i].float().reshape(-1), res['rewards'][i][b].float()
            assert float((got - ref).abs().max()) < REWARD_ATOL, (what, i)
            srt = ref.sort(descending=True).values
            gaps = [float(srt[q] - srt[q + 1]) for q in range(B)]
            assert all(g == 0 or g > MARGIN for g in gaps), (what, i, gaps)         # every decision of these seeds is checkable
            assert res['selected'][i][b].tolist() == br.select(ref.reshape(1, -1), B)[0].tolist() == o['selected'][i][0].tolist(), (what, i)
            assert torch.equal(res['beam_parents'][i][b], res['selected'][i][b] // N)
            assert float((got - one['rewards'][i][0].float()).abs().max()) <= FORM_REWARD, (what, i)
            assert torch.equal(res['selected'][i][b], one['selected'][i][0]), (what, i)
        assert float((res['x'][b].cpu() - o['x'][0]).abs().max()) < IMG_TOL, what
        assert float((res['x'][b] - one['x'][0]).abs().max()) < FORM_X, what
        assert res['net_rows'] // len(SEEDS) == rows == one['net_rows'], what


@pytest.mark.parametrize('dtype', DTYPES)
def test_naive_sampler_in_lock_step(manifest, dtype):
    res = hip_run(manifest, 'adm_tiny', 'naive', dtype, seeds=SEEDS)
    for b, s in enumerate(SEEDS):
        o, rows = oracle_run(manifest, 'adm_tiny', 'naive', s)
        one = solo_run(manifest, 'adm_tiny', 'naive', dtype, s)
        assert float((res['x'][b].cpu() - o['x'][0]).abs().max()) < IMG_TOL, s
        assert float((res['final_scores'][b] - o['final_scores'][0]).abs()) < REWARD_ATOL, s
        assert float((res['x'][b] - one['x'][0]).abs().max()) < FORM_X, s
        assert res['net_rows'] // len(SEEDS) == rows == one['net_rows'], s


@pytest.mark.parametrize('dtype', DTYPES)
def test_the_naive_search_is_the_plain_sampler(manifest, dtype):
    """generate_image_grid(NAIVE, seed=s) and plain.edm_sampler under torch.manual_seed(s) with host_randn_like are one loop (plain.heun_loop)
    on one stream -- per step one float64 draw [2, ...] from the global generator -- over the same schedule (this network neither clamps nor
    rounds it): the same latents and labels give the same final x bit for bit"""
    from diffusion_tts_amd import plain, sampler as sm, scorers as S
    net = hip_net(manifest, 'adm_tiny', dtype)
    lat, lab = inputs(net, [5, 7])
    res = sm.generate_image_grid(net, None, lat, lab, seed=3, gridw=2, gridh=1, device=torch.device(DEV), num_steps=STEPS,
                                 sampling_method=sm.SamplingMethod.NAIVE, sampling_params=dict(scorer=S.BrightnessScorer()), compute_dtype=dtype,
                                 verbose=False, **CHURN)
    torch.manual_seed(3)
    x = plain.edm_sampler(net, lat, lab, randn_like=plain.host_randn_like, num_steps=STEPS, **CHURN)
    assert res['net_rows'] == 2 * (2 * STEPS - 1) and x.dtype == torch.float64
    assert torch.equal(res['x'], x)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('method', ['eps_greedy', 'beam'])
def test_streams_are_isolated(manifest, method, dtype):
    """Equal seeds with equal inputs give bit-identical rows; a seed's result does not depend on its position or on its companions' seeds
    (same batch size, so the same launch forms: rows are position-independent, tests/test_gpu_search.py
    test_denoiser_rows_independent_of_batch_position)."""
    def image(res, b):
        return ([r[b] if method == 'beam' else r[:, b] for r in res['rewards']], [s[b] for s in res['selected']], res['x'][b], res['image'][b])

    def equal(p, q):
        return all(torch.equal(a, c) for a, c in zip(p[0], q[0])) and all(torch.equal(a, c) for a, c in zip(p[1], q[1])) \
            and torch.equal(p[2], q[2]) and torch.equal(p[3], q[3])
    same = hip_run(manifest, 'adm_tiny', method, dtype, seeds=[7, 7, 7])
    assert equal(image(same, 0), image(same, 1)) and equal(image(same, 0), image(same, 2))
    a = hip_run(manifest, 'adm_tiny', method, dtype, seeds=[0, 5, 7])
    c = hip_run(manifest, 'adm_tiny', method, dtype, seeds=[7, 0, 5])
    assert equal(image(a, 2), image(c, 0)) and equal(image(a, 0), image(c, 1)) and equal(image(a, 1), image(c, 2))
    assert not equal(image(a, 0), image(a, 2))                                      # different seeds are different searches


# ---- bulk mode ---------------------------------------------------------------------------------------------------------------------------
def bulk_run(manifest, dtype, outdir, seeds, **kw):
    from diffusion_tts_amd import bulk, sampler as sm, scorers as S
    net = hip_net(manifest, 'adm_tiny', dtype)
    return bulk.generate_seeds(net, seeds, str(outdir), sampling_method=sm.SamplingMethod.EPS_GREEDY,
                               sampling_params=dict(scorer=S.BrightnessScorer(), **EPS), device=DEV, compute_dtype=dtype, num_steps=STEPS,
                               scale_fn=seed0_scale, **CHURN, **kw)


def results_equal(p, q):
    return all(torch.equal(p[k], q[k]) for k in ('x', 'image', 'final_scores')) and p['net_rows'] == q['net_rows'] \
        and len(p['rewards']) == len(q['rewards']) and all(torch.equal(a, c) for a, c in zip(p['rewards'], q['rewards'])) \
        and all(torch.equal(a, c) for a, c in zip(p['selected'], q['selected']))


def png(path):
    import PIL.Image
    return np.array(PIL.Image.open(path))


@pytest.mark.parametrize('dtype', DTYPES)
def test_bulk_batches_do_not_depend_on_the_number_of_ranks(manifest, tmp_path, dtype):
    """seeds 0-7 in lock-step pairs: one rank, and ranks 0 and 1 of 2 (no collective: the split is by argument)"""
    from diffusion_tts_amd import bulk
    whole = bulk_run(manifest, dtype, tmp_path / 'w1', '0-7', search_batch=2, rank=0, world=1)
    parts = [bulk_run(manifest, dtype, tmp_path / 'w2', '0-7', search_batch=2, rank=r, world=2) for r in (0, 1)]
    assert sorted(whole) == list(range(8)) and sorted(parts[0]) == [0, 1, 4, 5] and sorted(parts[1]) == [2, 3, 6, 7]
    one = [b.tolist() for b in bulk.rank_batches(range(8), 2, 0, 1)]
    two = sorted(b.tolist() for r in (0, 1) for b in bulk.rank_batches(range(8), 2, r, 2))
    assert one == two == [[0, 1], [2, 3], [4, 5], [6, 7]]
    for s in range(8):
        mine = parts[0][s] if s in parts[0] else parts[1][s]
        assert results_equal(whole[s], mine), s
        assert whole[s]['row_seeds'] == mine['row_seeds'] == [s - s % 2, s - s % 2 + 1]
        assert tuple(whole[s]['x'].shape) == (1, 3, 16, 16) and tuple(whole[s]['rewards'][0].shape) == (3, 1) and tuple(whole[s]['selected'][0].shape) == (1,)
        for d in ('w1', 'w2'):
            assert np.array_equal(png(tmp_path / d / f'{s:06d}.png'), whole[s]['image'][0].permute(1, 2, 0).numpy()), (d, s)


@pytest.mark.parametrize('dtype', DTYPES)
def test_bulk_search_batch_1_is_the_direct_call_and_4_is_within_the_png_bound(manifest, tmp_path, dtype):
    ones = bulk_run(manifest, dtype, tmp_path / 'b1', '0-3', search_batch=1, subdirs=True)
    for s in range(4):
        direct = solo_run(manifest, 'adm_tiny', 'eps_greedy', dtype, s)               # generate_image_grid(seed=s): bit for bit
        assert results_equal(ones[s], direct), s
        assert ones[s]['row_seeds'] == [s]
        assert np.array_equal(png(tmp_path / 'b1' / '000000' / f'{s:06d}.png'), direct['image'][0].permute(1, 2, 0).numpy())
    four = bulk_run(manifest, dtype, tmp_path / 'b4', '0-3', search_batch=4)
    for s in range(4):
        assert four[s]['row_seeds'] == [0, 1, 2, 3] and four[s]['net_rows'] == ones[s]['net_rows']
        diff = np.abs(png(tmp_path / 'b4' / f'{s:06d}.png').astype(int) - png(tmp_path / 'b1' / '000000' / f'{s:06d}.png').astype(int))
        assert diff.max() <= 1 and (diff > 0).mean() < 5e-3, (s, diff.max(), (diff > 0).mean())


def test_bulk_mcts_keeps_the_per_seed_call(manifest, tmp_path):
    """MCTS is not run in lock-step: with a search batch it is still one `seed=` call per seed (no row_seeds in the result)"""
    from diffusion_tts_amd import bulk, sampler as sm, scorers as S
    net = hip_net(manifest, 'adm_tiny', torch.float32)
    np.random.seed(0)
    done = bulk.generate_seeds(net, '3-4', str(tmp_path), sampling_method=sm.SamplingMethod.MCTS,
                               sampling_params=dict(scorer=S.BrightnessScorer(), N=2, S=2), device=DEV, compute_dtype=torch.float32, num_steps=3,
                               search_batch=2, **CHURN)
    assert sorted(done) == [3, 4] and all('row_seeds' not in r for r in done.values())
    assert all(os.path.exists(tmp_path / f'{s:06d}.png') for s in (3, 4))


def test_main_search_batch_writes_one_png_per_seed(tmp_path):
    """`main.py --seeds 0-3 --search-batch 4` end to end in a fresh process"""
    out = tmp_path / 'out'
    cmd = [sys.executable, os.path.join(ROOT, 'main.py'), '--backend', 'edm', '--method', 'eps_greedy', '--network', 'random:ddpmpp_cifar10',
           '--scorer', 'brightness', '--N', '2', '--K', '1', '--seeds', '0-3', '--search-batch', '4', '--outdir', str(out)]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert f'4 images -> {out}' in done.stdout
    for s in range(4):
        img = png(out / f'{s:06d}.png')
        assert img.shape == (32, 32, 3) and img.dtype == np.uint8
    assert len({png(out / f'{s:06d}.png').tobytes() for s in range(4)}) == 4
