"""CPU: the restatement of the EDM beam search (tests/beam_reference.py, over the oracle's networks) against the runs of the reference's
own BEAM_SEARCH branch (tests/golden/make_golden_beam.py -> beam_golden.npz); the tie rule; the survivor exchange of the sharded search
over two gloo ranks.  Bounds are those tests/test_oracle_golden.py holds the eps-greedy traces to: rewards atol 2e-6, equal selections,
PNG within 1 LSB at < 1e-3 of the pixels, final state within 1e-3."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import beam_reference as br
from conftest import ROOT
from helpers import tiny_edm, oracle_net, T
from oracle import scorers as oscore

torch.set_num_threads(4)
REWARD_ATOL, X_TOL = 2e-6, 1e-3          # tests/test_oracle_golden.py


@pytest.fixture(scope='module')
def beam_golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'beam_manifest.json')) as f:
        return np.load(os.path.join(ROOT, 'tests', 'golden', 'beam_golden.npz')), json.load(f)


def _inputs(golden, meta):
    b = meta['batch']
    return T(golden[f'search_latents{b}']), T(golden[f'search_lab{b}'])


def _churn(meta):
    return {k: meta[k] for k in ('S_churn', 'S_min', 'S_max', 'S_noise')}


_RUNS = {}


def _restatement(golden, manifest, meta, case, stop_after=None):
    if case not in _RUNS:                                    # computed once, shared, left unchanged
        cfg, sd = tiny_edm(manifest, meta['net'])
        net = oracle_net(cfg, sd)
        lat, lab = _inputs(golden, meta)
        res = br.beam_search(net, lat, lab, B=meta['B'], N=meta['N'], scorer=oscore.BrightnessOracle(), seed=meta['seed'],
                             num_steps=meta['num_steps'], stop_after=stop_after, **_churn(meta))
        _RUNS[case] = (net, res)
    return _RUNS[case]


@pytest.mark.parametrize('case', ['beam_k1_adm', 'beam_k1_ddpmpp', 'beam_k2_prefix'])
def test_schedule_has_every_kind_of_step(golden, manifest, beam_golden, case):
    """asserted from t_steps: a leading gamma = 0 step, at least two noisy steps, a trailing step below S_min, and the last step (no Heun)"""
    g, m = beam_golden
    meta = m['cases'][case]
    cfg, sd = tiny_edm(manifest, meta['net'])
    t = br.osamp.sigma_schedule(oracle_net(cfg, sd), meta['num_steps'])
    gam = br.gammas(t, meta['num_steps'], meta['S_churn'], meta['S_min'], meta['S_max'])
    assert len(t) == meta['num_steps'] + 1 and float(t[-1]) == 0.0 and np.allclose(t.numpy(), meta['sigmas'], rtol=1e-12)
    assert gam[0] == 0 and float(t[0]) > meta['S_max']
    assert sum(1 for v in gam if v > 0) >= 2
    assert gam[-1] == 0 and float(t[meta['num_steps'] - 1]) < meta['S_min']
    assert meta['first_noisy_step'] == next(i for i, v in enumerate(gam) if v > 0) >= 1


@pytest.mark.parametrize('case', ['beam_k1_adm', 'beam_k1_ddpmpp'])
def test_restatement_matches_the_reference_run_k1(golden, manifest, beam_golden, case):
    """k = 1: the reference's branch is a correct greedy best-of-b-per-step search, for one image and for two.  Rewards of every step,
    selections, denoiser rows, the final state and the PNG."""
    g, m = beam_golden
    meta = m['cases'][case]
    net, res = _restatement(golden, manifest, meta, case)
    S, N, steps = meta['batch'], meta['N'], meta['num_steps']
    ref = g[f'{case}_rewards']
    assert ref.shape == (steps, S, N) and ref.dtype == np.float32 and len(res['rewards']) == steps
    assert net.evals == meta['net_rows'] == S * N * (2 * steps - 1)
    for i in range(steps):
        got = res['rewards'][i].numpy()
        assert np.allclose(got, ref[i], atol=REWARD_ATOL), (case, i, np.abs(got - ref[i]).max())
        assert torch.equal(res['selected'][i], br.select(T(ref[i]), 1)), (case, i)      # the reference's own rewards, the stated tie rule
        assert torch.equal(res['selected'][i], T(ref[i]).argmax(dim=1, keepdim=True))     # k = 1: its top-1 is the first maximum
        assert torch.equal(res['beam_parents'][i], torch.zeros(S, 1, dtype=torch.int64))
        if meta['gammas'][i] == 0:                                                        # identical candidates: exact ties, index 0
            assert np.all(ref[i] == ref[i][:, :1]) and np.all(got == got[:, :1]) and res['selected'][i].abs().sum() == 0
    x_err = float((res['x'] - T(g[f'{case}_x_final'])).abs().max())
    print(f'{case}: max |x - x_ref| = {x_err:.2e}')
    assert x_err < X_TOL
    assert np.allclose(res['final_scores'].numpy(), g[f'{case}_final_score'], atol=REWARD_ATOL)
    ref_img = g[f'{case}_image']
    mine = res['image'].permute(2, 0, 3, 1).reshape(ref_img.shape[0], -1, 3).numpy()
    diff = np.abs(mine.astype(int) - ref_img.astype(int))
    assert diff.max() <= 1 and (diff > 0).mean() < 1e-3, (case, diff.max(), (diff > 0).mean())


def test_restatement_matches_the_reference_prefix_k2(golden, manifest, beam_golden):
    """k = 2, b = 2: the sigma steps up to and including the first noisy one, before the reference's survivor gather can matter -- the draw
    order across beams, the row layout and all k*b rewards of a step."""
    g, m = beam_golden
    meta = m['cases']['beam_k2_prefix']
    keep = meta['steps_stored']
    assert keep == meta['first_noisy_step'] + 1 and meta['B'] == meta['k'] == 2 and meta['N'] == meta['b'] == 2
    net, res = _restatement(golden, manifest, meta, 'beam_k2_prefix', stop_after=keep)
    ref = g['beam_k2_prefix_rewards']
    assert ref.shape == (keep, 1, 4) and len(res['rewards']) == keep
    for i in range(keep):
        got = res['rewards'][i].numpy()
        assert np.allclose(got, ref[i], atol=REWARD_ATOL), (i, np.abs(got - ref[i]).max())
        assert torch.equal(res['selected'][i], br.select(T(ref[i]), 2)), i
    assert np.all(ref[:keep - 1] == ref[:keep - 1, :, :1])                       # until noise enters, every row of an image is the same row
    assert res['selected'][0].tolist() == [[0, 1]] and len(set(ref[keep - 1].reshape(-1).tolist())) == 4


def _selectors():
    from diffusion_tts_amd.sampler import beam_select
    return [('restatement', br.select), ('package', beam_select)]


@pytest.mark.parametrize('which', [0, 1])
def test_tie_rule(which):
    """Top B of B*N in descending order, exact ties to the lower flat index j*N + n -- across beams, and with more beams than candidates."""
    name, select = _selectors()[which]
    # B = 2, N = 3: the maximum is shared by candidate 2 of beam 0 and candidate 0 of beam 1 (flat 2 and 3), and by flat 5
    r = torch.tensor([[0.1, 0.2, 0.7, 0.7, 0.3, 0.7]])
    assert select(r, 2).tolist() == [[2, 3]], name
    assert select(r, 3).tolist() == [[2, 3, 5]], name
    # B = 3 > N = 2, all six equal (a gamma = 0 step): flat 0, 1, 2 = beam 0's two candidates, then beam 1's first
    r = torch.full((2, 6), 0.5)
    sel = select(r, 3)
    assert sel.tolist() == [[0, 1, 2], [0, 1, 2]] and (sel // 2).tolist() == [[0, 0, 1], [0, 0, 1]], name
    # B = 3 > N = 1: every candidate survives, in rank order, ties in index order
    assert select(torch.tensor([[0.2, 0.9, 0.2]]), 3).tolist() == [[1, 0, 2]], name
    # a tie below the maximum decides the LAST survivor; float32 is what is compared (two float64 values that round to one float32 tie)
    assert select(torch.tensor([[0.3, 0.9, 0.3, 0.1]]), 2).tolist() == [[1, 0]], name
    assert select(torch.tensor([[0.5 + 1e-12, 0.5, 0.25]], dtype=torch.float64), 1).tolist() == [[0]], name
    assert select(torch.tensor([[0.5, 0.5 + 1e-12, 0.25]], dtype=torch.float64), 1).tolist() == [[0]], name
    # two images are independent rows
    assert select(torch.tensor([[1.0, 2.0, 3.0, 4.0], [4.0, 3.0, 2.0, 1.0]]), 2).tolist() == [[3, 2], [0, 1]], name
    assert select(r, 3).dtype == torch.int64 and tuple(select(r, 3).shape) == (2, 3)


def test_command_line_flag_and_keyword_defaults():
    """`--beam {reference,run}`, default reference; generate_image_grid's keyword-only `beam_search`, default False."""
    import inspect
    import importlib.util
    spec = importlib.util.spec_from_file_location('dts_main_cli', os.path.join(ROOT, 'main.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ['--backend', 'edm', '--scorer', 'brightness', '--method', 'beam']
    assert cli.build_parser().parse_args(base).beam == 'reference'
    assert cli.build_parser().parse_args(base + ['--beam', 'run']).beam == 'run'
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ['--beam', 'fixed'])
    from diffusion_tts_amd.sampler import generate_image_grid
    par = inspect.signature(generate_image_grid).parameters['beam_search']
    assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY


# ---- the survivor exchange over two gloo ranks-----------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _exchange_worker(rank, world, port, q):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        try:
            from diffusion_tts_amd.parallel import CandidateShards
            sh = CandidateShards()
            g = torch.Generator().manual_seed(7)                                    # replicated
            S, B, N, steps = 2, 3, 5, 4
            out = []
            for i in range(steps):
                truth = torch.randn(S * B, 3, 4, 4, generator=g, dtype=torch.float64)
                truth[0, 0, 0, 0], truth[1, 0, 0, 1], truth[S * B - 1, 2, 3, 3] = -0.0, 0.0, -0.0
                truth[2, 1, 1, 1] = float('inf')
                cand = torch.randint(0, N, (S * B,), generator=g).tolist()
                if i == 1:
                    cand = [0] * (S * B)                                            # every survivor is rank 0's
                if i == 2:
                    cand = [N - 1] * (S * B)                                        # every survivor is rank 1's
                owners = [sh.owner(n, N) for n in cand]
                assert all(sh.span(N, o)[0] <= n < sh.span(N, o)[1] for n, o in zip(cand, owners))
                local = torch.full_like(truth, float('nan'))                        # what a rank does not own must never arrive
                for r_, o in enumerate(owners):
                    if o == rank:
                        local[r_] = truth[r_]
                lo, hi = sh.span(N)
                rew = torch.rand(N, S * B, generator=g)
                before = sh.collectives
                allr = sh.gather_rewards(rew[lo:hi].reshape(-1).clone(), N, S * B)
                got = sh.exchange_rows(local, owners)
                assert sh.collectives == before + 2                                 # one reward all-gather + one survivor exchange per sigma step
                assert torch.equal(allr.reshape(N, S * B), rew)
                same_bits = torch.equal(got.view(torch.int64), truth.view(torch.int64))     # bit for bit: -0.0 stays -0.0
                out.append((same_bits, bool(torch.signbit(got[0, 0, 0, 0])), bool(torch.signbit(got[1, 0, 0, 1])), got.dtype == torch.float64))
            bad = None
            try:
                sh.exchange_rows(torch.zeros(2, 3), [0])
            except ValueError as e:
                bad = str(e)
            q.put((rank, out, sh.collectives, bad))
        finally:
            dist.destroy_process_group()
    except Exception as e:                                                          # a failed worker must not leave the parent waiting
        q.put((rank, repr(e), -1, None))
        raise


def test_survivor_exchange_world2_gloo():
    """parallel.CandidateShards.exchange_rows: every rank ends with the S*B survivor rows bit for bit (-0.0 and inf included), whoever owns
    them -- mixed owners, all on rank 0, all on rank 1 -- in ONE collective per call; with the reward all-gather, 2 per sigma step."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_exchange_worker, args=(r, 2, port, q)) for r in range(2)]
    try:
        for p in procs:
            p.start()
        res = [q.get(timeout=120) for _ in procs]
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    assert all(p.exitcode == 0 for p in procs), res
    got = {r[0]: r[1:] for r in res}
    steps = 4
    for rank in (0, 1):
        out, collectives, bad = got[rank]
        assert out == [(True, True, False, True)] * steps, (rank, out)
        assert collectives == 2 * steps and 'owners' in bad


def test_survivor_exchange_single_process_is_a_noop():
    from diffusion_tts_amd.parallel import CandidateShards
    sh = CandidateShards()
    x = torch.randn(4, 3, dtype=torch.float64)
    assert sh.exchange_rows(x, [0, 0, 0, 0]) is x and sh.collectives == 0 and sh.owner(3, 5) == 0
