"""CPU: the MCTS searches of several seeds in lock-step (`generate_image_grid(row_seeds=..., mcts_lockstep=True)`), without a device.

The keyword's refusals by name and the old refusal without it; the numpy stream of a search (RandomState(s) against the seeded global
generator); the whole loop on a stub step -- `_mcts_lockstep` against `_mcts` run one seed at a time after torch.manual_seed(s) and
numpy.random.seed(s), with an element-wise stand-in for the Heun step and the scorer, so that trees, rewards, selections, row counts and
every draw must agree exactly; and bulk.generate_seeds(mcts_lockstep=True): its batches, its rank split and its file names on a stub."""
import os

import numpy as np
import pytest
import torch

from diffusion_tts_amd import bulk, sampler as sm
from diffusion_tts_amd.parallel import CandidateShards

SHAPE1 = (3, 4, 4)
STEPS = 5
CHURN = dict(S_churn=40, S_min=0.05, S_max=50, S_noise=1.003)
SEEDS, SHUFFLED = [0, 5, 7, 2], [7, 2, 0, 5]


class StubNet:
    img_resolution, img_channels, label_dim = 4, 3, 0
    dtype = torch.float32

    def __init__(self):
        self.evals = 0

    def round_sigma(self, sigma):
        return torch.as_tensor(sigma)

    def __call__(self, *a):
        raise AssertionError('a refused call must not reach the denoiser')


class StubLoop(sm._Loop):
    """_Loop on the host: the step is an element-wise function of a row, its noise and ITS OWN sigma step's scalars (a row computed with
    another row's scalars, or another search's noise, changes every reward), the reward the row's mean"""

    def __init__(self):
        super().__init__(StubNet(), 'cpu', STEPS, CHURN['S_churn'], CHURN['S_min'], CHURN['S_max'], CHURN['S_noise'], None,
                         CandidateShards(enabled=False))
        self.calls = []                                                             # (kind, rows, live rows, distinct sigma steps)

    @staticmethod
    def _row(x, eps, t_hat, coef, t_next):
        return (x + coef * eps.to(torch.float64)) * (t_next + 0.25) / (t_hat + 0.25) + 0.125 * t_hat

    def step(self, x_cur, t_cur, t_next, i, eps, labels, nb=None, interleave=False, live=None, first_denoised=False):
        nb = eps.shape[0] if nb is None else nb
        rep = nb // x_cur.shape[0]
        x = x_cur.repeat_interleave(rep, dim=0) if interleave else x_cur.repeat(rep, 1, 1, 1)
        t_hat, coef = self.churn(t_cur)
        self.net.evals += (nb if live is None else live) * (1 if i >= self.num_steps - 1 else 2)
        self.calls.append(('root' if interleave else 'step', nb, nb if live is None else live, 1))
        out = self._row(x, eps, t_hat, coef, float(t_next))
        return out, out

    def step_rows(self, x_cur, t_hat, coef, t_next, eps, labels, live=None):
        nb = eps.shape[0]
        assert len(t_hat) == len(coef) == len(t_next) == nb and all(float(t) != 0.0 for t in t_next)
        x = x_cur.repeat_interleave(nb // x_cur.shape[0], dim=0)
        col = lambda v: torch.tensor([float(a) for a in v], dtype=torch.float64).reshape(nb, 1, 1, 1)
        self.net.evals += (nb if live is None else live) * 2
        self.calls.append(('rows', nb, nb if live is None else live, len(set(float(t) for t in t_hat[:nb if live is None else live]))))
        return self._row(x, eps, col(t_hat), col(coef), col(t_next))

    def score(self, scorer, x, labels):
        return x.mean(dim=(1, 2, 3)).to(torch.float32)


class RecordingSource(sm._Source):
    def __init__(self, seeds):
        super().__init__(seeds)
        self.log = {b: [] for b in range(len(seeds))}

    def randn(self, image, shape, dtype=torch.float64):
        self.log[image].append((tuple(shape), dtype))
        return super().randn(image, shape, dtype)


def schedule():
    return sm.grid_schedule(StubNet(), STEPS, 0.002, 80, 7)


def start(seed):
    return torch.randn((1,) + SHAPE1, dtype=torch.float64, generator=torch.Generator().manual_seed(1000 + seed)) * 80


def solo(seed, params, monkeypatch):
    """`_mcts` for one image after torch.manual_seed(seed) and numpy.random.seed(seed): (x, rewards, selected, rows, draws, next numbers)"""
    L = StubLoop()
    draws = []
    real = torch.randn

    def recording(*size, **kw):
        if kw.get('generator') is None:
            draws.append((tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size), kw.get('dtype', torch.float32)))
        return real(*size, **kw)
    torch.manual_seed(seed)
    np.random.seed(seed)
    with monkeypatch.context() as m:
        m.setattr(torch, 'randn', recording)
        x = sm._mcts(L, schedule(), start(seed), None, params, None)
    return dict(x=x, rewards=L.rewards, selected=L.selected, rows=L.net.evals, draws=draws, next_torch=real(5))


@pytest.mark.parametrize('N,S', [(2, 6), (3, 6), (4, 20), (2, 40)])
def test_the_lock_step_loop_is_each_seeds_own_search(N, S, monkeypatch):
    """S = 20 and 40 take two and three groups of simulations per sigma step (16 + 4, 16 + 16 + 8); rollout batches above 16 rows are padded,
    which no count may show.  With S <= 16 the tree statistics do not move inside a sigma step and every search expands one level below its
    previous simulation: no launch can hold two sigma steps; with several groups the stub's rewards (means of states of magnitude 80) tell
    the trees apart."""
    from types import SimpleNamespace
    params = SimpleNamespace(N=N, S=S, scorer=None)
    ones = {s: solo(s, params, monkeypatch) for s in SEEDS}
    mixed = 0
    for order in (SEEDS, SHUFFLED):
        L = StubLoop()
        L.src, L.row_seeds = RecordingSource(order), list(order)
        before = np.random.get_state()
        np.random.seed(99)
        state = np.random.get_state()
        x = sm._mcts_lockstep(L, schedule(), torch.cat([start(s) for s in order]), None, params, None)
        after = np.random.get_state()
        assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]      # the global generator: not advanced
        np.random.set_state(before)
        groups = [min(16, S - g0) for g0 in range(0, S, 16)]
        assert [tuple(r.shape) for r in L.rewards] == [(len(order), g) for _ in range(STEPS) for g in groups]
        assert len(L.selected) == STEPS and all(tuple(sel.shape) == (len(order),) for sel in L.selected)
        for b, s in enumerate(order):
            one = ones[s]
            assert len(one['rewards']) == len(L.rewards)
            assert all(torch.equal(r[b], r1) for r, r1 in zip(L.rewards, one['rewards'])), s
            assert all(torch.equal(sel[b:b + 1], s1) for sel, s1 in zip(L.selected, one['selected'])), s
            assert torch.equal(x[b:b + 1], one['x']), s
            assert L.search_rows[b] == one['rows'], s
            # the lane's draws: the num_steps float32 [1, N, C, H, W] up front, then N discarded [1, C, H, W] per expanding simulation
            log = L.src.log[b]
            assert log == one['draws'], s
            assert log[:STEPS] == [((1, N) + SHAPE1, torch.float32)] * STEPS and set(log[STEPS:]) <= {((1,) + SHAPE1, torch.float32)}
            assert len(log) > STEPS and (len(log) - STEPS) % N == 0
            assert torch.equal(torch.randn(5, generator=L.src.gens[b]), one['next_torch']), s
        assert L.net.evals == sum(L.search_rows) == sum(ones[s]['rows'] for s in order)           # padding rows are not counted
        rows_calls = [c for c in L.calls if c[0] == 'rows']
        assert L.mcts_ragged_launches == len(rows_calls) and L.mcts_mixed_launches == sum(c[3] > 1 for c in rows_calls)
        assert all(c[2] <= len(order) * N for c in rows_calls)                                     # one launch per simulation index: <= S * b rows
        assert len(rows_calls) <= STEPS * S
        G = sm.MCTS_LOCKSTEP_PAD_ROWS
        for kind, rows, live, _ in L.calls:                                         # above 16 rows: whole granules (expansions: whole nodes)
            assert live <= rows and (rows == live if rows <= 16 else rows % (G if kind == 'step' else max(1, G // N) * N) == 0), (kind, rows, live)
        mixed += L.mcts_mixed_launches
    if S <= 16:
        assert mixed == 0
    if S == 40:
        assert mixed >= 1                                                           # trees of different depths did meet in one launch


@pytest.mark.parametrize('n', [2, 3, 4])
def test_a_random_state_replays_the_seeded_global_generator(n):
    before = np.random.get_state()
    try:
        for s in (0, 5, 7, 2, 2 ** 31 + 5):
            np.random.seed(s)
            want = [np.random.randint(0, n) for _ in range(200)]
            rs = np.random.RandomState(s)
            assert [rs.randint(0, n) for _ in range(200)] == want, s
    finally:
        np.random.set_state(before)


def grid(method=sm.SamplingMethod.MCTS, images=3, **kw):
    lat = torch.zeros((images,) + (3, 16, 16))

    class Net(StubNet):
        img_resolution = 16
    return sm.generate_image_grid(Net(), None, lat, None, num_steps=4, sampling_method=method, sampling_params=dict(scorer=None, N=3, K=2),
                                  verbose=False, **kw)


def test_refusals_by_name(monkeypatch):
    M = sm.SamplingMethod

    def no_load(*a, **k):
        raise AssertionError('a refused bulk call must not load a network')
    monkeypatch.setattr(bulk, 'load_network', no_load)
    with pytest.raises(ValueError, match=r'row_seeds: SamplingMethod.MCTS is not supported \(its numpy child draw and its ragged trees are per search\)'):
        grid(row_seeds=[0, 5, 7])                                                   # without the keyword: the old message, verbatim
    with pytest.raises(ValueError, match='mcts_lockstep=True: SamplingMethod.MCTS only, got EPS_GREEDY'):
        grid(M.EPS_GREEDY, row_seeds=[0, 5, 7], mcts_lockstep=True)
    with pytest.raises(ValueError, match='mcts_lockstep=True: needs row_seeds'):
        grid(mcts_lockstep=True)
    with pytest.raises(ValueError, match='mcts_lockstep=True: forced_selections is not supported'):
        grid(row_seeds=[0, 5, 7], mcts_lockstep=True, forced_selections=[0] * 8)
    with pytest.raises(ValueError, match='mcts_lockstep=True: precomputed_noise is not supported'):
        grid(row_seeds=[0, 5, 7], mcts_lockstep=True, precomputed_noise={0: torch.zeros(3, 3, 3, 16, 16)})
    with pytest.raises(ValueError, match='row_seeds: need one seed per image, got 2 seeds for 3 images'):
        grid(row_seeds=[0, 5], mcts_lockstep=True)
    with pytest.raises(ValueError, match='mcts_lockstep=True: SamplingMethod.MCTS only, got EPS_GREEDY'):
        bulk.generate_seeds(StubNet(), '0-3', '.', sampling_method=M.EPS_GREEDY, search_batch=2, mcts_lockstep=True)
    with pytest.raises(ValueError, match='mcts_lockstep=True: forced_selections / precomputed_noise'):
        bulk.generate_seeds(StubNet(), '0-3', '.', sampling_method=M.MCTS, search_batch=2, mcts_lockstep=True, precomputed_noise={})


def test_candidate_sharding_is_refused(monkeypatch):
    class TwoRanks:
        solo, rank, collectives = False, 0, 0

        def __init__(self, enabled=True):
            pass
    monkeypatch.setattr(sm, 'CandidateShards', TwoRanks)
    with pytest.raises(ValueError, match='mcts_lockstep=True: candidate sharding over more than one rank is not supported'):
        grid(images=2, row_seeds=[1, 2], mcts_lockstep=True)


def test_main_refuses_the_flag_where_it_does_not_apply():
    import main as cli
    parse = lambda extra: cli.build_parser().parse_args(['--backend', 'edm', '--scorer', 'brightness'] + extra)
    ok = parse(['--method', 'mcts', '--seeds', '0-3', '--search-batch', '4', '--mcts-lockstep'])
    assert ok.mcts_lockstep is True and parse(['--method', 'mcts']).mcts_lockstep is False
    cli.check_bulk_args(ok)
    with pytest.raises(ValueError, match='--mcts-lockstep is an EDM option of --method mcts'):
        cli.check_bulk_args(parse(['--method', 'eps_greedy', '--seeds', '0-3', '--mcts-lockstep']))
    with pytest.raises(ValueError, match='--mcts-lockstep goes with --seeds'):
        cli.check_bulk_args(parse(['--method', 'mcts', '--mcts-lockstep']))


def test_bulk_batches_file_names_and_rank_split_on_a_stub(tmp_path, monkeypatch):
    calls = []

    def fake_grid(net, dest_path, latents, labels, **kw):
        calls.append(dict(kw, dest_path=dest_path, images=latents.shape[0]))
        n = latents.shape[0]
        if dest_path is not None:
            bulk.save_image(np.zeros((4, 4, 3), dtype=np.uint8), dest_path)
        seeds = kw.get('row_seeds', [kw.get('seed')])
        res = dict(x=torch.zeros((n,) + SHAPE1), image=torch.tensor([s % 256 for s in seeds], dtype=torch.uint8).reshape(n, 1, 1, 1).expand(n, 3, 4, 4).contiguous(),
                   final_scores=torch.zeros(n), avg_score=0.0, rewards=[torch.arange(n * 6.).reshape(n, 6)], selected=[torch.arange(n)],
                   beam_parents=[], best_noises={}, net_rows=sum(10 + s for s in seeds))
        if 'row_seeds' in kw:
            res.update(row_seeds=list(seeds), search_rows=[10 + s for s in seeds], mcts_ragged_launches=3, mcts_mixed_launches=1)
        return res
    monkeypatch.setattr(bulk, 'generate_image_grid', fake_grid)
    monkeypatch.setattr(bulk, 'load_network', lambda net, **kw: net)
    run = lambda out, **kw: bulk.generate_seeds(StubNet(), '0-6', str(tmp_path / out), sampling_method=sm.SamplingMethod.MCTS,
                                                sampling_params=dict(N=2, S=6), search_batch=2, num_steps=4, **kw)
    whole = run('w1', mcts_lockstep=True, rank=0, world=1)
    assert sorted(whole) == list(range(7))
    assert [c['row_seeds'] for c in calls] == [b.tolist() for b in bulk.rank_batches(range(7), 2, 0, 1)] == [[0, 1], [2, 3], [4, 5], [6]]
    assert all(c['mcts_lockstep'] is True and c['dest_path'] is None and c['shard_candidates'] is False and 'seed' not in c for c in calls)
    for s in range(7):
        path = tmp_path / 'w1' / f'{s:06d}.png'
        assert os.path.exists(path)
        import PIL.Image
        assert int(np.array(PIL.Image.open(path))[0, 0, 0]) == s                   # the seed's own row of the batch went into its file
        b = s % 2
        assert whole[s]['net_rows'] == 10 + s and tuple(whole[s]['rewards'][0].shape) == (6,) and whole[s]['selected'][0].tolist() == [b]
        assert torch.equal(whole[s]['rewards'][0], torch.arange(6.) + 6 * b)
        assert whole[s]['mcts_ragged_launches'] == 3
    del calls[:]
    parts = [run('w2', mcts_lockstep=True, rank=r, world=2) for r in (0, 1)]
    assert sorted(parts[0]) == [0, 1, 4, 5] and sorted(parts[1]) == [2, 3, 6]     # dealt out in turn, no collective
    assert sorted(os.listdir(tmp_path / 'w2')) == [f'{s:06d}.png' for s in range(7)]
    del calls[:]
    plain = run('w3')                                                                # without the flag: one `seed=` call per seed, as ever
    assert sorted(plain) == list(range(7)) and [c['seed'] for c in calls] == list(range(7))
    assert all('row_seeds' not in c and 'mcts_lockstep' not in c and c['images'] == 1 for c in calls)
    sub = bulk.generate_seeds(StubNet(), '999-1000', str(tmp_path / 'w4'), sampling_method=sm.SamplingMethod.MCTS, search_batch=2,
                              mcts_lockstep=True, subdirs=True)
    assert sorted(sub) == [999, 1000] and os.path.exists(tmp_path / 'w4' / '000000' / '000999.png') and os.path.exists(tmp_path / 'w4' / '001000' / '001000.png')
