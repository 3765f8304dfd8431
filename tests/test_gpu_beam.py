"""GPU: the EDM beam search, `generate_image_grid(..., sampling_method=BEAM_SEARCH, beam_search=True)`: B beams per image x N candidates
per beam.  Against the runs of the reference's own branch (k = 1: tests/golden/beam_golden.npz, make_golden_beam.py), against the CPU
restatement (tests/beam_reference.py) where the reference's branch is wrong (k > 1), sharded over two gloo ranks, the refusals, and the
command line.  Comparisons and bounds are those of tests/test_gpu_search.py (rewards atol 5e-5 in float32 and f16x3, a selection checked
wherever the reference's gap exceeds 4 x the reward deviation, final state within 1e-3, PNG within 1 LSB) and of
tests/test_gpu_sharded.py (sharded against solo: rewards 2e-6, equal selections, final state 1e-5)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

import beam_reference as br                                                     # noqa: E402
from conftest import ROOT                                                       # noqa: E402
from helpers import tiny_edm, oracle_net, T                                     # noqa: E402
from oracle import scorers as oscore                                            # noqa: E402

DEV = 'cuda'
X3 = 'f16x3'
REWARD_ATOL, IMG_TOL = 5e-5, 1e-3            # tests/test_gpu_search.py
CHURN = dict(S_churn=40, S_min=0.05, S_max=50, S_noise=1.003)
STEPS = 6
BN_SEED = 1        # B = 2, N = 3, two images: the first seed whose decisions all have a gap of 0 or >= 4e-5 AND whose noisy steps hold both a
                   # pair of survivors with one parent and a pair with two (scanned on the CPU with tests/beam_reference.py; asserted below)


@pytest.fixture(scope='module')
def beam_golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'beam_manifest.json')) as f:
        return np.load(os.path.join(ROOT, 'tests', 'golden', 'beam_golden.npz')), json.load(f)


_NETS, _REST = {}, {}


def hip_net(manifest, name, dtype):
    from diffusion_tts_amd.networks import EDMPrecond
    if (name, dtype) not in _NETS:
        cfg, sd = tiny_edm(manifest, name)
        _NETS[(name, dtype)] = EDMPrecond(cfg, sd, device=DEV, dtype=dtype)
    return _NETS[(name, dtype)]


def run_hip(manifest, golden, netname, batch, B, N, seed, dtype=torch.float32, method='BEAM_SEARCH', num_steps=STEPS, **extra):
    from diffusion_tts_amd import sampler as sm, scorers as S
    lat, lab = T(golden[f'search_latents{batch}']), T(golden[f'search_lab{batch}'])
    extra.setdefault('beam_search', True)
    params = dict(scorer=S.BrightnessScorer(), B=B, N=N)
    params.update(extra.pop('params', {}))
    return sm.generate_image_grid(hip_net(manifest, netname, dtype), None, lat, lab, seed=seed, gridw=batch, gridh=1, device=torch.device(DEV),
                                  num_steps=num_steps, sampling_method=getattr(sm.SamplingMethod, method), sampling_params=params,
                                  compute_dtype=dtype, verbose=False, **CHURN, **extra)


def restatement(manifest, golden, key, netname, batch, B, N, seed, pre=None):
    """the CPU restatement of one case: computed once, shared by the tests that need it, left unchanged"""
    if key not in _REST:
        cfg, sd = tiny_edm(manifest, netname)
        lat, lab = T(golden[f'search_latents{batch}']), T(golden[f'search_lab{batch}'])
        _REST[key] = br.beam_search(oracle_net(cfg, sd), lat, lab, B=B, N=N, scorer=oscore.BrightnessOracle(), seed=seed, num_steps=STEPS,
                                    precomputed_noise=pre, **CHURN)
    return _REST[key]


def compare_trace(res, ref_rewards, B, what, max_skipped):
    """tests/test_gpu_search.py's comparison of a free-running search: every step's rewards within REWARD_ATOL; a decision (the gaps between
    neighbours among the best B + 1 of an image) is an exact tie (ours must tie too, lower index first), decidable (gap > 4 x this step's
    reward deviation: the selection must equal the stable top-B of the reference's rewards), or skipped; at most `max_skipped` are skipped."""
    skipped = checked = 0
    assert len(res['rewards']) == len(res['selected']) == len(res['beam_parents']) == len(ref_rewards)
    for i, ref in enumerate(ref_rewards):
        ref = T(np.asarray(ref)).float()
        got = res['rewards'][i].float()
        assert got.shape == ref.shape and res['selected'][i].shape == (ref.shape[0], B) and res['selected'][i].dtype == torch.int64
        dev = float((got - ref).abs().max())
        print(f'{what} step {i}: max reward deviation {dev:.2e}')
        assert dev < REWARD_ATOL, (what, i, dev)
        want = br.select(ref, B)
        srt = ref.sort(dim=1, descending=True).values
        for s in range(ref.shape[0]):
            gaps = [float(srt[s, q] - srt[s, q + 1]) for q in range(min(B, ref.shape[1] - 1))]
            if any(0 < g <= 4 * dev for g in gaps):
                skipped += 1
                continue
            checked += 1
            assert res['selected'][i][s].tolist() == want[s].tolist(), (what, i, s, gaps, dev)
            if all(g == 0 for g in gaps) and bool((ref[s] == ref[s, 0]).all()):        # identical candidates (gamma = 0): our rewards tie exactly too
                assert bool((got[s] == got[s, 0]).all()) and res['selected'][i][s].tolist() == list(range(B)), (what, i, s)
        N = ref.shape[1] // B
        assert torch.equal(res['beam_parents'][i], res['selected'][i] // N)
    print(f'{what}: {checked} decisions checked, {skipped} skipped as undecidable')
    assert skipped <= max_skipped and checked > 0, (what, skipped)


@pytest.mark.parametrize('dtype', [torch.float32, X3])
@pytest.mark.parametrize('case', ['beam_k1_adm', 'beam_k1_ddpmpp'])
def test_beam_k1_against_the_reference_run(golden, manifest, beam_golden, case, dtype):
    """k = 1 (B = 1): the reference's own greedy best-of-b-per-step runs, one image on ADM (b = 4) and two on DDPM++ (b = 3, odd, two label
    rows).  Rewards of every step, selections, denoiser rows, final state and PNG; at most one decision may be skipped as undecidable."""
    g, m = beam_golden
    meta = m['cases'][case]
    S, N = meta['batch'], meta['N']
    assert meta['B'] == 1 and meta['num_steps'] == STEPS and all(meta[k] == v for k, v in CHURN.items())
    res = run_hip(manifest, golden, meta['net'], S, 1, N, meta['seed'], dtype)
    # the schedule, from t_steps: a leading gamma = 0 step, >= 2 noisy steps, a trailing step below S_min which is also the Euler-only last step
    t = res['t_steps']
    gam = br.gammas(t, STEPS, CHURN['S_churn'], CHURN['S_min'], CHURN['S_max'])
    assert gam[0] == 0 and sum(1 for v in gam if v > 0) >= 2 and gam[-1] == 0 and float(t[STEPS - 1]) < CHURN['S_min'] and float(t[STEPS]) == 0
    assert res['net_rows'] == meta['net_rows'] == S * N * (2 * STEPS - 1)
    assert res['collectives'] == 0
    compare_trace(res, g[f'{case}_rewards'], 1, f'{case} {dtype}', max_skipped=1)
    x_err = float((res['x'].cpu() - T(g[f'{case}_x_final'])).abs().max())
    print(f'{case} {dtype}: max |x - x_ref| = {x_err:.2e}')
    assert x_err < IMG_TOL
    ref_img = g[f'{case}_image']
    mine = res['image'].permute(2, 0, 3, 1).reshape(ref_img.shape[0], -1, 3).numpy()
    diff = np.abs(mine.astype(int) - ref_img.astype(int))
    assert diff.max() <= 1 and (diff > 0).mean() < 5e-3, (case, diff.max(), (diff > 0).mean())
    assert np.allclose(res['final_scores'].float().numpy(), g[f'{case}_final_score'], atol=REWARD_ATOL)


def test_beam_k2_prefix_against_the_reference_run(golden, manifest, beam_golden):
    """k = 2, b = 2: the steps before the reference's wrong survivor gather can matter -- draw order across beams, row layout, all k*b rewards."""
    g, m = beam_golden
    meta = m['cases']['beam_k2_prefix']
    keep = meta['steps_stored']
    res = run_hip(manifest, golden, meta['net'], 1, 2, 2, meta['seed'])
    cut = dict(rewards=res['rewards'][:keep], selected=res['selected'][:keep], beam_parents=res['beam_parents'][:keep])
    compare_trace(cut, g['beam_k2_prefix_rewards'], 2, 'beam_k2_prefix', max_skipped=0)
    assert res['net_rows'] == 1 * 2 * 2 * (2 * STEPS - 1)


def test_beam_b2_n3_two_images_against_the_restatement(golden, manifest):
    """B = 2, N = 3, two images (more than one beam, N odd, two label rows): where the reference's gather is wrong, the restatement is the
    yardstick.  The seed's trace holds survivors of one image that share a parent and survivors that do not, at noisy steps."""
    o = restatement(manifest, golden, 'b2n3', 'adm_tiny', 2, 2, 3, BN_SEED)
    par = [p.tolist() for p in o['beam_parents']]
    gam = br.gammas(o['t_steps'], STEPS, CHURN['S_churn'], CHURN['S_min'], CHURN['S_max'])
    noisy_after_first = [i for i in range(STEPS) if gam[i] > 0][1:]              # the beams of an image differ from here on
    assert any(par[i][s][0] == par[i][s][1] for i in noisy_after_first for s in range(2))
    assert any(par[i][s][0] != par[i][s][1] for i in noisy_after_first for s in range(2))
    res = run_hip(manifest, golden, 'adm_tiny', 2, 2, 3, BN_SEED)
    compare_trace(res, [r.numpy() for r in o['rewards']], 2, 'B=2 N=3', max_skipped=1)
    assert [p.tolist() for p in res['beam_parents']] == par
    assert res['net_rows'] == 2 * 2 * 3 * (2 * STEPS - 1)
    assert float((res['x'].cpu() - o['x']).abs().max()) < IMG_TOL
    assert (res['image'].int() - o['image'].int()).abs().max().item() <= 1
    assert tuple(res['x'].shape) == (2, 3, 16, 16)


def test_precomputed_noise_replaces_exactly_the_draws_of_its_step(golden, manifest):
    """precomputed_noise[i] [S, B, N, C, H, W] stands in for the S*B draws of step i, which are then NOT made: later steps take the draws
    that would have followed.  Checked two ways: against the restatement with the same hook, and against a run that is handed EVERY step's
    noise -- the seed's stream with step i's draws left out, written down here."""
    S, B, N, i_pre = 2, 2, 3, 2
    shape = (S, B, N, 3, 16, 16)
    pre = {i_pre: torch.randn(shape, generator=torch.Generator().manual_seed(123), dtype=torch.float64)}
    o = restatement(manifest, golden, 'b2n3_pre', 'adm_tiny', 2, B, N, BN_SEED, pre=pre)
    res = run_hip(manifest, golden, 'adm_tiny', 2, B, N, BN_SEED, precomputed_noise=pre)
    compare_trace(res, [r.numpy() for r in o['rewards']], B, 'precomputed step 2', max_skipped=1)
    assert float((res['x'].cpu() - o['x']).abs().max()) < IMG_TOL
    plain = run_hip(manifest, golden, 'adm_tiny', 2, B, N, BN_SEED)
    for i in range(i_pre):                                                         # nothing before step i changes ...
        assert torch.equal(plain['rewards'][i], res['rewards'][i]) and torch.equal(plain['selected'][i], res['selected'][i])
    assert not torch.equal(plain['rewards'][i_pre], res['rewards'][i_pre])         # ... step i takes the given noise
    torch.manual_seed(BN_SEED)
    every = {}
    for i in range(STEPS):
        every[i] = pre[i] if i in pre else torch.stack([torch.randn((N, 3, 16, 16), dtype=torch.float64) for _ in range(S * B)]).reshape(shape)
    full = run_hip(manifest, golden, 'adm_tiny', 2, B, N, BN_SEED + 1000, precomputed_noise=every)        # no draw left for its own seed to matter
    for i in range(STEPS):
        assert torch.equal(full['rewards'][i], res['rewards'][i]) and torch.equal(full['selected'][i], res['selected'][i]), i
    assert torch.equal(full['x'], res['x'])
    with pytest.raises(ValueError, match='precomputed_noise'):
        run_hip(manifest, golden, 'adm_tiny', 2, B, N, BN_SEED, precomputed_noise={0: torch.zeros(S, B * N, 3, 16, 16)})


def test_refusals_and_the_unchanged_default(golden, manifest):
    """Without the keyword, and with beam_search=False, BEAM_SEARCH is the reference's branch: AttributeError on `p.b`.  The keyword goes with
    BEAM_SEARCH only, and not with forced_selections / candidate_chunk / record_noises; B and N must be at least 1."""
    from diffusion_tts_amd import sampler as sm, scorers as S
    net = hip_net(manifest, 'adm_tiny', torch.float32)
    lat, lab = T(golden['search_latents1']), T(golden['search_lab1'])
    kw = dict(seed=0, gridw=1, gridh=1, device=torch.device(DEV), num_steps=STEPS, sampling_method=sm.SamplingMethod.BEAM_SEARCH,
              sampling_params=dict(scorer=S.BrightnessScorer(), B=2, N=2), compute_dtype=torch.float32, verbose=False, **CHURN)
    with pytest.raises(AttributeError):
        sm.generate_image_grid(net, None, lat, lab, **kw)
    with pytest.raises(AttributeError):
        sm.generate_image_grid(net, None, lat, lab, beam_search=False, **kw)
    with pytest.raises(ValueError, match='BEAM_SEARCH'):
        run_hip(manifest, golden, 'adm_tiny', 1, 2, 2, 0, method='EPS_GREEDY')
    with pytest.raises(ValueError, match='BEAM_SEARCH'):
        run_hip(manifest, golden, 'adm_tiny', 1, 2, 2, 0, method='NAIVE')
    with pytest.raises(ValueError, match='forced_selections'):
        run_hip(manifest, golden, 'adm_tiny', 1, 2, 2, 0, forced_selections=[0] * STEPS)
    with pytest.raises(ValueError, match='candidate_chunk'):
        run_hip(manifest, golden, 'adm_tiny', 1, 2, 2, 0, candidate_chunk=1)
    with pytest.raises(ValueError, match='record_noises'):
        run_hip(manifest, golden, 'adm_tiny', 1, 2, 2, 0, record_noises=True)
    with pytest.raises(ValueError, match='B >= 1'):
        run_hip(manifest, golden, 'adm_tiny', 1, 0, 2, 0)
    with pytest.raises(ValueError, match='N >= 1'):
        run_hip(manifest, golden, 'adm_tiny', 1, 2, 0, 0)


# ---- two gloo ranks on the one GPU ----------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _pack(res):
    return dict(x=res['x'].cpu().numpy(), rewards=[r.float().numpy().copy() for r in res['rewards']], selected=[s.numpy().copy() for s in res['selected']],
                parents=[s.numpy().copy() for s in res['beam_parents']], collectives=int(res['collectives']), rows=int(res['net_rows']))


def _shard_worker(rank, world, port, manifest, q):
    import torch.distributed as dist
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        dist.init_process_group('gloo', rank=rank, world_size=world)
        try:
            golden = np.load(os.path.join(ROOT, 'tests', 'golden', 'edm_golden.npz'))
            q.put((rank, _pack(run_hip(manifest, golden, 'adm_tiny', 2, 2, 3, BN_SEED))))
        finally:
            dist.destroy_process_group()
    except Exception as e:                                   # on the queue: the parent must not wait for a worker that failed
        q.put((rank, repr(e)))
        raise


def test_sharded_beam_equals_single_process(golden, manifest):
    """B = 2, N = 3, two images over two ranks (rank 0 owns candidates 0-1 of every beam, rank 1 candidate 2): the solo run's selections
    and rewards, its final state, and 2 collectives per sigma step -- the reward all-gather and the survivor exchange."""
    solo = _pack(run_hip(manifest, golden, 'adm_tiny', 2, 2, 3, BN_SEED))
    assert solo['collectives'] == 0
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, manifest, q)) for r in range(2)]
    try:
        for p in procs:
            p.start()
        got = []
        for _ in procs:
            item = q.get(timeout=300)
            assert not isinstance(item[1], str), item
            got.append(item)
        for p in procs:
            p.join(timeout=120)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    assert all(p.exitcode == 0 for p in procs)
    got = dict(got)
    for r in (0, 1):
        me = got[r]
        assert len(me['rewards']) == STEPS
        for a, c in zip(me['rewards'], solo['rewards']):
            assert np.allclose(a, c, atol=2e-6), r
        assert all(np.array_equal(a, c) for a, c in zip(me['selected'], solo['selected'])), r
        assert all(np.array_equal(a, c) for a, c in zip(me['parents'], solo['parents'])), r
        assert np.abs(me['x'] - solo['x']).max() < 1e-5, r
        assert me['collectives'] == 2 * STEPS
        assert me['rows'] < solo['rows']
    assert got[0]['rows'] + got[1]['rows'] == solo['rows']
    assert np.array_equal(got[0]['x'], got[1]['x'])                                # replicas agree bit for bit


def test_bulk_generation_passes_the_keyword_through(manifest, tmp_path):
    """bulk.generate_seeds forwards keyword extras to generate_image_grid: a seed's beam-search image is the direct call's."""
    from diffusion_tts_amd import bulk, sampler as sm, scorers as S
    net = hip_net(manifest, 'adm_tiny', torch.float32)
    params = dict(scorer=S.BrightnessScorer(), B=2, N=3)
    kw = dict(num_steps=STEPS, sampling_method=sm.SamplingMethod.BEAM_SEARCH, sampling_params=params, compute_dtype=torch.float32, **CHURN)
    done = bulk.generate_seeds(net, '7', str(tmp_path), device=DEV, beam_search=True, **kw)
    assert sorted(done) == [7] and os.path.exists(tmp_path / '000007.png') and len(done[7]['beam_parents']) == STEPS
    lat, lab = bulk.seed_inputs(7, net)
    one = sm.generate_image_grid(net, None, lat, lab, seed=7, gridw=1, gridh=1, device=torch.device(DEV), verbose=False, beam_search=True, **kw)
    assert torch.equal(one['image'], done[7]['image']) and torch.equal(one['x'], done[7]['x'])
    with pytest.raises(AttributeError):
        bulk.generate_seeds(net, '7', str(tmp_path), device=DEV, **kw)


def test_main_beam_run_writes_its_png(tmp_path):
    """`main.py --backend edm --method beam --beam run` end to end in a fresh process; without `--beam run` the same command line is the
    reference's AttributeError (tests/test_gpu_search.py::test_beam_raises_like_the_reference holds that at the API)."""
    out = tmp_path / 'beam.png'
    cmd = [sys.executable, os.path.join(ROOT, 'main.py'), '--backend', 'edm', '--method', 'beam', '--beam', 'run', '--network', 'random:ddpmpp_cifar10',
           '--scorer', 'brightness', '--B', '2', '--N', '2', '--output', str(out)]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    import PIL.Image
    img = np.array(PIL.Image.open(out))
    assert img.shape == (32, 32, 3) and img.dtype == np.uint8
    assert f'denoiser rows: {2 * 2 * 35}' in done.stdout
