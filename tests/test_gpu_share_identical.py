"""GPU: `generate_image_grid(share_identical=True)` -- the identical candidates of a sigma step without churn noise go through the denoiser and
the scorer once.

Settings are those of tests/test_gpu_lockstep.py: the tiny 16x16 networks of tests/golden/manifest.json, 4 sigma steps with S_churn=40,
S_min=0.05, S_max=50, S_noise=1.003 (sigma steps 0 and 3 lie outside the churn window: two of the four steps are shared), hashing.seed0_scale,
the brightness scorer, N=3, K=2, lambda 0.15, eps 0.4 (and eps 0: zero-order), float32 and f16x3 with reuse_winner=False.  Two yardsticks:
this build's own full run (share_identical off) -- same draws, same pivot steps, so x, image, selections and final scores are BIT-equal and only
the rewards of a shared step come from another launch form (batch B instead of N*B: FORM_REWARD) -- and the reference's restatement on the CPU,
one seed at a time (oracle.sampler.search, tests/beam_reference.beam_search), which keeps evaluating every candidate.  Bounds are the
project's: REWARD_ATOL / IMG_TOL against the oracle, FORM_REWARD / FORM_X between launch forms, helpers.check_decisions / MARGIN with the
counts of tie and safe decisions asserted (eps 0.4: 4 ties + 4 safe per seed, as tests/test_gpu_lockstep.py notes; eps 0: the 4 ties of the
shared steps + 4 safe ones, the smallest top-2 gap of the reference's restatement being 3.2e-4 over the four seeds)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

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
SHARED = [0, 3]
SEEDS = [0, 5, 7, 2]
N, K = 3, 2
BEAM_B = 2

_NETS, _ORACLE, _RUNS = {}, {}, {}


def eps_params(eps):
    return dict(N=N, K=K, lambda_param=0.15, eps=eps)


def hip_net(manifest, dtype, name='adm_tiny'):
    from diffusion_tts_amd.networks import EDMPrecond
    if (name, dtype) not in _NETS:
        cfg, sd = tiny_edm(manifest, name)
        _NETS[(name, dtype)] = EDMPrecond(cfg, sd, device=DEV, dtype=dtype)
    return _NETS[(name, dtype)]


def inputs(net, seeds):
    from diffusion_tts_amd import bulk
    pairs = [bulk.seed_inputs(s, net) for s in seeds]
    return torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])


def oracle_run(manifest, method, seed, eps=0.4):
    """the reference's restatement of ONE seed's search on the CPU, every candidate evaluated: computed once, shared, left unchanged"""
    key = (method, seed, eps)
    if key not in _ORACLE:
        cfg, sd = tiny_edm(manifest, 'adm_tiny')
        net = oracle_net(cfg, sd)
        lat, lab = inputs(net, [seed])
        rows0 = net.evals
        if method == 'beam':
            o = br.beam_search(net, lat, lab, B=BEAM_B, N=N, scorer=oscore.BrightnessOracle(), seed=seed, num_steps=STEPS, **CHURN)
        else:
            o = osamp.search(net, lat, lab, method='eps_greedy', params=dict(scorer=oscore.BrightnessOracle(), **eps_params(eps)), seed=seed,
                             num_steps=STEPS, scale_fn=seed0_scale, **CHURN)
        _ORACLE[key] = (o, net.evals - rows0)
    return _ORACLE[key]


CASES = {'one': dict(lat=[0], kw=dict(seed=0)), 'pair': dict(lat=[0, 5], kw=dict(seed=3)), 'rows': dict(lat=SEEDS, kw=dict(row_seeds=SEEDS))}


def hip_run(manifest, dtype, case, eps=0.4, beam=False, cache=False, **extra):
    from diffusion_tts_amd import sampler as sm, scorers as S
    key = (str(dtype), case, eps, beam)
    if cache and key in _RUNS:
        return _RUNS[key]
    net = hip_net(manifest, dtype)
    lat, lab = inputs(net, CASES[case]['lat'])
    if beam:
        how = dict(sampling_method=sm.SamplingMethod.BEAM_SEARCH, sampling_params=dict(scorer=S.BrightnessScorer(), B=BEAM_B, N=N), beam_search=True)
    else:
        method = sm.SamplingMethod.EPS_GREEDY if eps else sm.SamplingMethod.ZERO_ORDER
        how = dict(sampling_method=method, sampling_params=dict(scorer=S.BrightnessScorer(), **eps_params(eps)), reuse_winner=False)
    res = sm.generate_image_grid(net, None, lat, lab, gridw=lat.shape[0], gridh=1, device=torch.device(DEV), num_steps=STEPS, scale_fn=seed0_scale,
                                 compute_dtype=dtype, verbose=False, **CHURN, **how, **CASES[case]['kw'], **extra)
    if cache:
        _RUNS[key] = res
    return res


def full_run(manifest, dtype, case, eps=0.4, beam=False):
    """this build's run with the keyword off: computed once per setting, shared, left unchanged"""
    return hip_run(manifest, dtype, case, eps, beam, cache=True)


def schedule_steps(res, net):
    from diffusion_tts_amd import sampler as sm
    return sm.identical_steps(res['t_steps'], STEPS, CHURN['S_churn'], CHURN['S_min'], CHURN['S_max'], CHURN['S_noise'], net.round_sigma)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('eps', [0.4, 0])
@pytest.mark.parametrize('case', ['one', 'pair', 'rows'])
def test_local_search_shares_the_steps_without_noise(manifest, case, eps, dtype):
    from diffusion_tts_amd import sampler as sm
    full = full_run(manifest, dtype, case, eps)
    res = hip_run(manifest, dtype, case, eps, share_identical=True)
    B = len(CASES[case]['lat'])
    what = f'{case} eps={eps} {dtype}'
    assert full['shared_steps'] == [] and res['shared_steps'] == SHARED == schedule_steps(res, hip_net(manifest, dtype))
    # the shared run takes exactly the full run's pivot steps
    for key in ('x', 'image', 'final_scores'):
        assert torch.equal(res[key], full[key]), (what, key)
    assert len(res['selected']) == len(full['selected']) == len(res['rewards']) == len(full['rewards']) == STEPS * K
    assert all(torch.equal(a, c) and a.dtype == c.dtype for a, c in zip(res['selected'], full['selected'])), what
    for d, (got, ref) in enumerate(zip(res['rewards'], full['rewards'])):
        assert got.shape == ref.shape == (N, B) and got.dtype == ref.dtype, (what, d)
        if d // K in SHARED:
            assert all(torch.equal(got[n], got[0]) for n in range(N)), (what, d)     # one value per image
            assert res['selected'][d].tolist() == [0] * B, (what, d)
            dev = float((got - ref).abs().max())
            print(f'{what} decision {d} (shared): max |reward - full run\'s| = {dev:.2e}')
            assert dev <= FORM_REWARD, (what, d, dev)
        else:
            assert torch.equal(got, ref), (what, d)
    saved = sm.shared_rows_saved(SHARED, STEPS, N, K, B)
    assert saved == K * N * B * 3 and res['net_rows'] == full['net_rows'] - saved, (what, res['net_rows'], full['net_rows'])
    assert res['collectives'] == full['collectives'] == 0
    if case == 'pair':
        return
    # against the reference's restatement, one seed at a time
    for b, s in enumerate(CASES[case]['lat']):
        o, rows = oracle_run(manifest, 'eps_greedy', s, eps)
        assert full['net_rows'] // B == rows
        mine = [r[:, b].reshape(-1).float() for r in res['rewards']]
        for d, (got, ref) in enumerate(zip(mine, o['rewards'])):
            dev = float((got - ref.reshape(-1).float()).abs().max())
            assert dev < REWARD_ATOL, (what, s, d, dev)
        same, report = check_decisions([r.reshape(-1, 1) for r in o['rewards']], o['selected'], [sel[b:b + 1] for sel in res['selected']], f'{what} seed {s}')
        assert same and "'sub-noise': 0" in report and "'diverged-after': 0" in report, report
        assert "'tie': 4" in report and "'safe': 4" in report, report                # nothing passes by being skipped
        x_err = float((res['x'][b].cpu() - o['x'][0]).abs().max())
        print(f'{what} seed {s}: max |x - x_ref| = {x_err:.2e}')
        assert x_err < IMG_TOL, (what, s)


@pytest.mark.parametrize('dtype', DTYPES)
def test_forced_selections_move_the_pivot_at_shared_steps_too(manifest, dtype):
    """a walk whose decisions at the SHARED steps (0, 1 and 6, 7) are not candidate 0: the pivot is rebuilt from the forced candidate's noise as
    the full run rebuilds it, so the recorded winning noises and the state are the full run's bit for bit; `selected` stays the run's own
    argmax, 0 at an exact tie"""
    forced = [1, 2, 0, 1, 2, 0, 2, 1]
    assert all(forced[d] != 0 for d in range(STEPS * K) if d // K in SHARED)
    full = hip_run(manifest, dtype, 'one', forced_selections=forced, record_noises=True)
    res = hip_run(manifest, dtype, 'one', forced_selections=forced, record_noises=True, share_identical=True)
    assert sorted(res['best_noises']) == sorted(full['best_noises']) == list(range(STEPS))
    for i in range(STEPS):
        assert res['best_noises'][i].shape == full['best_noises'][i].shape == (K, 1, 3, 16, 16)
        assert torch.equal(res['best_noises'][i], full['best_noises'][i]), i
    assert torch.equal(res['x'], full['x']) and torch.equal(res['image'], full['image'])
    assert all(torch.equal(a, c) for a, c in zip(res['selected'], full['selected']))
    assert [int(s[0]) for d, s in enumerate(res['selected']) if d // K in SHARED] == [0] * 4
    free = full_run(manifest, dtype, 'one')
    assert not torch.equal(res['x'], free['x'])                                     # the forced walk is another trajectory
    # without forced selections the recorded noises are the full run's as well
    a, c = hip_run(manifest, dtype, 'rows', record_noises=True), hip_run(manifest, dtype, 'rows', record_noises=True, share_identical=True)
    assert all(torch.equal(a['best_noises'][i], c['best_noises'][i]) for i in range(STEPS))


@pytest.mark.parametrize('dtype', DTYPES)
def test_beam_search_evaluates_one_row_per_class(manifest, dtype):
    """B=2 beams x N=3 candidates, the four seeds in lock-step.  Class rule: the B beam rows of an image start as one class; the survivors of a
    shared step inherit their parents' classes; after any other step every survivor is a class of its own.  Here sigma step 0 is shared
    with ONE class per image (1 row, two Heun stages), steps 1 and 2 are full (B*N rows, two stages each) and step 3 is shared after a
    noisy step (B classes; the last step has one stage): 1*2 + 2*(B*N*2) + B*1 = 28 rows per image against the full run's 3*(B*N*2) + B*N = 42."""
    B = BEAM_B
    full = full_run(manifest, dtype, 'rows', beam=True)
    res = hip_run(manifest, dtype, 'rows', beam=True, share_identical=True)
    assert res['shared_steps'] == SHARED and full['shared_steps'] == []
    assert len(res['rewards']) == len(res['selected']) == len(res['beam_parents']) == STEPS
    per_image = 1 * 2 + 2 * (B * N * 2) + B * 1
    assert full['net_rows'] == len(SEEDS) * (3 * (B * N * 2) + B * N) and res['net_rows'] == len(SEEDS) * per_image == len(SEEDS) * 28
    for i in range(STEPS):
        assert res['rewards'][i].shape == full['rewards'][i].shape == (len(SEEDS), B * N) and res['rewards'][i].dtype == full['rewards'][i].dtype
        assert torch.equal(res['selected'][i], full['selected'][i]) and torch.equal(res['beam_parents'][i], full['beam_parents'][i]), i
        assert torch.equal(res['beam_parents'][i], res['selected'][i] // N)
        dev = float((res['rewards'][i] - full['rewards'][i]).abs().max())
        print(f'beam {dtype} step {i}: max |reward - full run\'s| = {dev:.2e}')
        assert dev <= FORM_REWARD, (i, dev)
    assert all(torch.equal(res['rewards'][0][b], res['rewards'][0][b, :1].expand(B * N)) for b in range(len(SEEDS)))   # one class: one value
    x_dev = float((res['x'] - full['x']).abs().max())
    print(f'beam {dtype}: max |x - full run\'s x| = {x_dev:.2e}')
    assert x_dev < FORM_X
    for b, s in enumerate(SEEDS):
        o, rows = oracle_run(manifest, 'beam', s)
        what = f'beam {dtype} seed {s}'
        assert rows == 42
        for i in range(STEPS):
            ref, got = o['rewards'][i].float().reshape(-1), res['rewards'][i][b].float()
            assert float((got - ref).abs().max()) < REWARD_ATOL, (what, i)
            srt = ref.sort(descending=True).values
            gaps = [float(srt[q] - srt[q + 1]) for q in range(B)]
            assert all(g == 0 or g > MARGIN for g in gaps), (what, i, gaps)         # every decision of these seeds is checkable
            assert res['selected'][i][b].tolist() == br.select(ref.reshape(1, -1), B)[0].tolist() == o['selected'][i][0].tolist(), (what, i)
            assert res['beam_parents'][i][b].tolist() == o['beam_parents'][i][0].tolist(), (what, i)
        assert float((res['x'][b].cpu() - o['x'][0]).abs().max()) < IMG_TOL, what


def test_beam_rows_stay_one_class_without_churn(manifest):
    """S_churn = 0: every step is shared.  The B rows of an image stay ONE class throughout (all survivors of a one-class step are copies of
    its one row): one row per image and stage, 2*STEPS - 1 rows per image; every reward row is one value and every selection is the first B
    flat indices."""
    from diffusion_tts_amd import sampler as sm, scorers as S
    net = hip_net(manifest, torch.float32)
    lat, lab = inputs(net, SEEDS[:2])
    kw = dict(gridw=2, gridh=1, device=torch.device(DEV), num_steps=STEPS, sampling_method=sm.SamplingMethod.BEAM_SEARCH,
              sampling_params=dict(scorer=S.BrightnessScorer(), B=3, N=2), beam_search=True, compute_dtype=torch.float32, verbose=False, seed=1)
    full = sm.generate_image_grid(net, None, lat, lab, **kw)
    res = sm.generate_image_grid(net, None, lat, lab, share_identical=True, **kw)
    assert res['shared_steps'] == list(range(STEPS))
    assert res['net_rows'] == 2 * (2 * STEPS - 1) and full['net_rows'] == 2 * 3 * 2 * (2 * STEPS - 1)
    for i in range(STEPS):
        assert res['selected'][i].tolist() == full['selected'][i].tolist() == [[0, 1, 2]] * 2
        assert all(torch.equal(r, r[:1].expand(6)) for r in res['rewards'][i])
        assert float((res['rewards'][i] - full['rewards'][i]).abs().max()) <= FORM_REWARD
    assert float((res['x'] - full['x']).abs().max()) < FORM_X


@pytest.mark.parametrize('dtype', DTYPES)
def test_iddpm_network_shares_by_its_own_round_sigma(dtype):
    """a tiny iDDPM network (tests/test_gpu_precond.py's fixtures): round_sigma snaps every level and every t_hat to the network's table, so
    which steps add no noise is decided by the coefficient the loop computes with THIS network's round_sigma, not by gamma"""
    import precond_helpers as ph
    from diffusion_tts_amd import sampler as sm, scorers as S
    from diffusion_tts_amd.networks import EDMPrecond
    man = ph.manifest()
    cfg, sd = ph.tiny_weights(man, 'iddpm')
    net = EDMPrecond(cfg, sd, device=DEV, dtype=dtype)
    steps = 6
    lat = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(4))
    lab = torch.eye(10)[torch.tensor([3, 8])]
    kw = dict(seed=2, gridw=2, gridh=1, device=torch.device(DEV), num_steps=steps, sigma_min=max(0.002, net.sigma_min), sigma_max=min(80, net.sigma_max),
              sampling_method=sm.SamplingMethod.EPS_GREEDY, sampling_params=dict(scorer=S.BrightnessScorer(), **eps_params(0.4)), scale_fn=seed0_scale,
              compute_dtype=dtype, verbose=False, reuse_winner=False, **man['S'])
    full = sm.generate_image_grid(net, None, lat, lab, **kw)
    res = sm.generate_image_grid(net, None, lat, lab, share_identical=True, **kw)
    c = man['S']
    want = sm.identical_steps(res['t_steps'], steps, c['S_churn'], c['S_min'], c['S_max'], c['S_noise'], net.round_sigma)
    print(f'iddpm {dtype}: sigma levels {[round(float(t), 5) for t in res["t_steps"]]}, shared steps {want}')
    assert res['shared_steps'] == want and 0 < len(want) < steps
    assert torch.equal(res['t_steps'][:-1], net.round_sigma(res['t_steps'][:-1]))   # the levels are table entries
    assert torch.equal(res['x'], full['x']) and torch.equal(res['image'], full['image'])
    assert all(torch.equal(a, b) for a, b in zip(res['selected'], full['selected']))
    assert res['net_rows'] == full['net_rows'] - sm.shared_rows_saved(want, steps, N, K, 2)


# ---- sharded over two ranks ------------------------------------------------------------------------------------------------------------------
SHARD_N = 4


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _shard_runs(manifest, golden_path):
    """eps-greedy N=4, K=2 on one image, full and shared, float32 and f16x3; numpy results (plain pickling through the queue)"""
    from diffusion_tts_amd.networks import EDMPrecond
    from diffusion_tts_amd.sampler import SamplingMethod, generate_image_grid
    from diffusion_tts_amd.scorers import BrightnessScorer
    g = np.load(golden_path)
    cfg, sd = tiny_edm(manifest, 'adm_tiny')
    lat, lab = torch.from_numpy(g['search_latents1']), torch.from_numpy(g['search_lab1'])
    out = {}
    for dtype in DTYPES:
        net = EDMPrecond(cfg, sd, device='cuda', dtype=dtype)
        for share in (False, True):
            res = generate_image_grid(net, None, lat, lab, seed=3, gridw=1, gridh=1, device=torch.device('cuda'), num_steps=STEPS,
                                      sampling_method=SamplingMethod.EPS_GREEDY, scale_fn=seed0_scale, compute_dtype=dtype, verbose=False,
                                      sampling_params=dict(scorer=BrightnessScorer(), N=SHARD_N, K=K, lambda_param=0.15, eps=0.4),
                                      reuse_winner=False, share_identical=share, **CHURN)
            out[(str(dtype), share)] = dict(x=res['x'].cpu().numpy(), selected=[s.numpy().copy() for s in res['selected']],
                                            rewards=[r.float().numpy().copy() for r in res['rewards']], collectives=res['collectives'],
                                            rows=res['net_rows'], shared=res['shared_steps'])
    return out


def _shard_worker(rank, world, port, manifest, golden_path, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        q.put((rank, _shard_runs(manifest, golden_path)))
    finally:
        dist.destroy_process_group()


def test_sharded_search_makes_no_collective_at_a_shared_step(manifest):
    """two gloo ranks on the one GPU (the pattern of tests/test_gpu_sharded.py): at a shared step every rank computes the one row itself, so the
    K reward all-gathers of that sigma step do not take place"""
    gp = os.path.join(ROOT, 'tests', 'golden', 'edm_golden.npz')
    solo = _shard_runs(manifest, gp)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, manifest, gp, q)) for r in range(2)]
    try:
        for p in procs:
            p.start()
        got = dict(q.get(timeout=240) for _ in procs)
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    for dtype in DTYPES:
        one, one_full = solo[(str(dtype), True)], solo[(str(dtype), False)]
        assert one['shared'] == SHARED and one['collectives'] == 0 and one['rows'] == one_full['rows'] - K * SHARD_N * 3
        for r in (0, 1):
            full, me = got[r][(str(dtype), False)], got[r][(str(dtype), True)]
            what = f'{dtype} rank {r}'
            assert me['shared'] == SHARED and full['collectives'] == STEPS * K, what
            assert me['collectives'] == full['collectives'] - len(SHARED) * K, (what, me['collectives'])
            assert me['rows'] == full['rows'] - K * (SHARD_N // 2) * 3, (what, me['rows'], full['rows'])   # this rank's share of the candidates
            assert all(np.array_equal(a, c) for a, c in zip(me['selected'], got[0][(str(dtype), True)]['selected'])), what
            assert all(np.array_equal(a, c) for a, c in zip(me['selected'], one['selected'])), what
            assert all(np.abs(a - c).max() <= FORM_REWARD for a, c in zip(me['rewards'], one['rewards'])), what
            assert np.abs(me['x'] - one['x']).max() < FORM_X, what


# ---- bulk mode and the default -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_bulk_pngs_do_not_change(manifest, tmp_path, dtype):
    from diffusion_tts_amd import bulk, sampler as sm, scorers as S
    net = hip_net(manifest, dtype)

    def run(outdir, **kw):
        return bulk.generate_seeds(net, '0-3', str(outdir), sampling_method=sm.SamplingMethod.EPS_GREEDY,
                                   sampling_params=dict(scorer=S.BrightnessScorer(), **eps_params(0.4)), device=DEV, compute_dtype=dtype, num_steps=STEPS,
                                   scale_fn=seed0_scale, search_batch=2, **CHURN, **kw)
    full, res = run(tmp_path / 'full'), run(tmp_path / 'shared', share_identical=True)
    assert sorted(full) == sorted(res) == [0, 1, 2, 3]
    for s in range(4):
        with open(tmp_path / 'full' / f'{s:06d}.png', 'rb') as f, open(tmp_path / 'shared' / f'{s:06d}.png', 'rb') as h:
            assert f.read() == h.read(), s
        assert res[s]['shared_steps'] == SHARED and full[s]['shared_steps'] == []
        assert res[s]['net_rows'] == full[s]['net_rows'] - K * N * 3
        assert torch.equal(res[s]['x'], full[s]['x']) and all(torch.equal(a, c) for a, c in zip(res[s]['selected'], full[s]['selected']))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('beam', [False, True])
def test_the_keyword_is_off_by_default(manifest, beam, dtype):
    """share_identical=False and no keyword at all: the same launches -- every field bit-equal, the reference's row count, no shared step"""
    without = full_run(manifest, dtype, 'rows', beam=beam)
    off = hip_run(manifest, dtype, 'rows', beam=beam, share_identical=False)
    assert sorted(off) == sorted(without)
    for key in ('x', 'image', 'final_scores', 't_steps'):
        assert torch.equal(off[key], without[key]), key
    for key in ('rewards', 'selected', 'beam_parents'):
        assert len(off[key]) == len(without[key]) and all(torch.equal(a, c) for a, c in zip(off[key], without[key])), key
    for key in ('avg_score', 'net_rows', 'collectives', 'row_seeds', 'shared_steps', 'best_noises'):
        assert off[key] == without[key], key
    assert off['shared_steps'] == [] and off['best_noises'] == {}
    rows = [oracle_run(manifest, 'beam' if beam else 'eps_greedy', s)[1] for s in SEEDS]
    assert off['net_rows'] == sum(rows) and len(set(rows)) == 1


def test_the_keyword_is_refused_where_nothing_is_shared(manifest):
    from diffusion_tts_amd import sampler as sm, scorers as S
    net = hip_net(manifest, torch.float32)
    lat, lab = inputs(net, [0])
    for method in (sm.SamplingMethod.NAIVE, sm.SamplingMethod.REJECTION_SAMPLING, sm.SamplingMethod.MCTS):
        with pytest.raises(ValueError, match='share_identical'):
            sm.generate_image_grid(net, None, lat, lab, device=torch.device(DEV), num_steps=STEPS, sampling_method=method,
                                   sampling_params=dict(scorer=S.BrightnessScorer(), N=2, S=2), compute_dtype=torch.float32, verbose=False,
                                   share_identical=True)
