"""GPU: the MCTS searches of several seeds in lock-step -- `generate_image_grid(row_seeds=..., mcts_lockstep=True)` and
`bulk.generate_seeds(search_batch=..., mcts_lockstep=True)`.

The yardstick is the reference's CPU restatement run ONE SEED AT A TIME: numpy.random.seed(s), then oracle.sampler.search(method='mcts',
seed=s) -- never this build's own batched run.  Settings (the frame of tests/test_gpu_lockstep.py): the tiny 16x16 adm_tiny of
tests/golden/manifest.json, the brightness scorer, hashing.seed0_scale, latents and labels from bulk.seed_inputs, S_churn=40, S_min=0.05,
S_max=50, S_noise=1.003, four seeds, float32 and f16x3.  Bounds are the project's: rewards within 5e-5 of the reference call by call and the
final state within 1e-3; against this build's own one-image call (numpy.random.seed(s); seed=s: other launch forms only) rewards within
2e-6 and the state within 1e-5 (tests/test_gpu_sharded.py).

Two settings (CONFIGS):
  s6    N = 3 children, S = 6 simulations, 5 sigma steps.  With S <= 16 all simulations of a sigma step are ONE group, the tree statistics
        move only between groups, and a fresh node's children are all unvisited (UCB = inf, first maximum): simulation k of EVERY search
        follows the chain the simulations before it built and expands one level below simulation k - 1, whatever the rewards are -- every
        seed of a scan of 0 .. 39 grows [1, 2, 3], [2, 3], [3], [], [] at N = 2 and at N = 3, and more sigma steps only lengthen the chains
        (8 steps: [1..6], [2..6], ...).  The expansions of one simulation index therefore stand at ONE sigma step in every launch of this
        setting: mcts_mixed_launches is 0 by construction and cannot be made >= 1 at S = 6; the per-row launches themselves are made and
        counted.
  s36   N = 2, S = 36 (groups of 16, 16 and 4: the statistics do move inside a sigma step), 6 sigma steps: at sigma step 1 the trees of
        seeds 0, 1 expand at steps 2, 3, 4 where those of seeds 4, 6 expand at 3, 4: launches that hold rows of two sigma steps.  Here
        mcts_mixed_launches >= 1 is asserted, so the per-row path cannot go untested.

An MCTS run is comparable only while the trees agree, and a UCB or best-child comparison closer than helpers.MARGIN (4e-5) can flip
legitimately.  `replay` walks the reference's search again on the host from its recorded rewards alone (the tree statistics are sums of
those rewards; the child draws are RandomState(s)'s) and returns every decision's top-2 gap; that it IS the reference's search is asserted
(its selections and its number of scorer calls are the recorded ones).  The seeds were chosen on the CPU from the reference alone, by that
replay: a seed is kept when every one of its UCB argmaxes and best-child choices has a top-2 gap of exactly 0 (equal values, among them
the several unvisited children of a fresh node: the first maximum on both sides) or above MARGIN.  s6: seeds 0 .. 39 scanned in order,
all 40 kept (61 decisions each), the first four taken.  s36: seeds 0 .. 23 scanned in order, all 24 kept (smallest gap above 0:
6.1e-5, seed 22); 0 .. 3 share one tree shape, so the first two of each of the two shapes were taken: 0, 1 and 4, 6.  The test
re-computes and ASSERTS the property for every decision: nothing passes by being skipped, no decision is excused.
Measured on an MI355X: rewards within 1.2e-5 of the reference (float32: 1.1e-5), final state within 3.5e-5, in both settings."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import tiny_edm, oracle_net, MARGIN                                # noqa: E402
from oracle import sampler as osamp, scorers as oscore                          # noqa: E402
from diffusion_tts_amd.hashing import seed0_scale                               # noqa: E402

DEV = 'cuda'
X3 = 'f16x3'
DTYPES = [torch.float32, X3]
REWARD_ATOL, IMG_TOL = 5e-5, 1e-3            # against the reference (tests/test_gpu_lockstep.py)
FORM_REWARD, FORM_X = 2e-6, 1e-5             # the same search under other launch forms (tests/test_gpu_sharded.py)
CONFIGS = {'s6': dict(N=3, S=6, steps=5, seeds=[0, 1, 2, 3]), 's36': dict(N=2, S=36, steps=6, seeds=[0, 1, 4, 6])}
CHURN = dict(S_churn=40, S_min=0.05, S_max=50, S_noise=1.003)
NAME = 'adm_tiny'

_NETS, _ORACLE, _SOLO, _LOCK = {}, {}, {}, {}


class _Stat:
    __slots__ = ('children', 'reward', 'visit')

    def __init__(self, visit=0):
        self.children, self.reward, self.visit = [], 0, visit


def top2_gap(values):
    """gap between the two largest of `values`: 0.0 for an exact tie (two infinities included), inf for a single candidate"""
    v = sorted((float(a) for a in values), reverse=True)
    if len(v) < 2:
        return float('inf')
    return 0.0 if v[0] == v[1] else v[0] - v[1]


def replay(rewards, seed, b, sims, ns):
    """The reference's one-image MCTS (oracle.sampler._mcts, m = 1) on its tree statistics alone: UCB1 descent, expansion while the leaf
    is above the last sigma step, the child draw from RandomState(seed), back-propagation of the recorded `rewards` (one tensor per
    group of min(16, S) simulations).  Returns (selected per sigma step, [(kind, top-2 gap)] of every decision, and per sigma step and
    simulation index the sigma step the simulation expanded at, or None)."""
    rng = np.random.RandomState(seed)
    root, selected, gaps, grew, call = _Stat(1), [], [], [], 0
    for i in range(ns):
        if not root.children:
            root.children = [_Stat() for _ in range(b)]
        group = min(16, sims)
        grew.append([])
        for g0 in range(0, sims, group):
            paths = []
            for sim in range(g0, min(g0 + group, sims)):
                node, it, path = root, i, [root]
                while node.children:
                    ucb = [float('inf') if c.visit == 0 else c.reward / c.visit + np.sqrt(2 * np.log(node.visit) / c.visit) for c in node.children]
                    gaps.append(('ucb', top2_gap(ucb)))
                    node = node.children[int(np.argmax(ucb))]
                    it += 1
                    path.append(node)
                grew[i].append(it if it < ns - 1 else None)
                if it < ns - 1:
                    node.children = [_Stat() for _ in range(b)]
                    node = node.children[rng.randint(0, b)]
                    path.append(node)
                paths.append(path)
            rew = rewards[call]
            call += 1
            assert len(rew) == len(paths)
            for path, r in zip(paths, rew):
                for nd in path:
                    nd.reward += r.item()
                    nd.visit += 1
        means = [c.reward / c.visit for c in root.children if c.visit > 0]
        gaps.append(('best', top2_gap(means)))
        best, best_r, best_j = None, -float('inf'), -1
        for j, c in enumerate(root.children):
            if c.visit > 0 and c.reward / c.visit > best_r:
                best, best_r, best_j = c, c.reward / c.visit, j
        selected.append(best_j)
        root = best
    assert call == len(rewards)
    return selected, gaps, grew


def hip_net(manifest, dtype):
    from diffusion_tts_amd.networks import EDMPrecond
    if dtype not in _NETS:
        cfg, sd = tiny_edm(manifest, NAME)
        _NETS[dtype] = EDMPrecond(cfg, sd, device=DEV, dtype=dtype)
    return _NETS[dtype]


def inputs(net, seeds):
    from diffusion_tts_amd import bulk
    pairs = [bulk.seed_inputs(s, net) for s in seeds]
    return torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])


def oracle_run(manifest, cfg_name, seed):
    """the reference's restatement of ONE seed's search on the CPU after numpy.random.seed(seed): computed once, shared, left unchanged;
    (result, denoiser rows)"""
    c = CONFIGS[cfg_name]
    if (cfg_name, seed) not in _ORACLE:
        cfg, sd = tiny_edm(manifest, NAME)
        net = oracle_net(cfg, sd)
        lat, lab = inputs(net, [seed])
        rows0 = net.evals
        state = np.random.get_state()
        np.random.seed(seed)
        try:
            o = osamp.search(net, lat, lab, method='mcts', params=dict(scorer=oscore.BrightnessOracle(), N=c['N'], S=c['S']), seed=seed,
                             num_steps=c['steps'],
                             scale_fn=seed0_scale, **CHURN)
        finally:
            np.random.set_state(state)
        _ORACLE[(cfg_name, seed)] = (o, net.evals - rows0)
    return _ORACLE[(cfg_name, seed)]


def hip_run(manifest, cfg_name, dtype, seeds=None, seed=None):
    """row_seeds=seeds, mcts_lockstep=True (one lock-step batch), or the one-image call seed=seed after numpy.random.seed(seed)"""
    from diffusion_tts_amd import sampler as sm, scorers as Sc
    c = CONFIGS[cfg_name]
    net = hip_net(manifest, dtype)
    lat, lab = inputs(net, seeds if seeds is not None else [seed])
    kw = dict(row_seeds=list(seeds), mcts_lockstep=True) if seeds is not None else dict(seed=seed)
    if seeds is None:
        np.random.seed(seed)
    return sm.generate_image_grid(net, None, lat, lab, gridw=lat.shape[0], gridh=1, device=torch.device(DEV), num_steps=c['steps'],
                                  sampling_method=sm.SamplingMethod.MCTS, sampling_params=dict(scorer=Sc.BrightnessScorer(), N=c['N'], S=c['S']),
                                  scale_fn=seed0_scale, compute_dtype=dtype, verbose=False, **CHURN, **kw)


def solo_run(manifest, cfg_name, dtype, seed):
    key = (cfg_name, str(dtype), seed)
    if key not in _SOLO:
        state = np.random.get_state()
        try:
            _SOLO[key] = hip_run(manifest, cfg_name, dtype, seed=seed)
        finally:
            np.random.set_state(state)
    return _SOLO[key]


def lock_run(manifest, cfg_name, dtype, seeds):
    """the lock-step call over `seeds`, made once per (dtype, order); numpy's global generator must come out of it as it went in"""
    key = (cfg_name, str(dtype), tuple(seeds))
    if key not in _LOCK:
        before = np.random.get_state()
        res = hip_run(manifest, cfg_name, dtype, seeds=seeds)
        after = np.random.get_state()
        assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:], 'numpy\'s global generator moved'
        _LOCK[key] = res
    return _LOCK[key]


def grown(manifest, cfg_name):
    """per seed of the setting, `replay`'s third result: the sigma step every simulation expanded at"""
    c = CONFIGS[cfg_name]
    return [replay(oracle_run(manifest, cfg_name, s)[0]['rewards'], s, c['N'], c['S'], c['steps'])[2] for s in c['seeds']]


def mixed_indices(manifest, cfg_name):
    """(sigma step, simulation index) pairs at which the expanding searches of the setting stand at two or more sigma steps"""
    c, g = CONFIGS[cfg_name], grown(manifest, cfg_name)
    return [(i, k) for i in range(c['steps']) for k in range(c['S']) if len({t[i][k] for t in g} - {None}) > 1]


@pytest.mark.parametrize('cfg_name', sorted(CONFIGS))
def test_every_decision_of_the_chosen_seeds_is_checkable(manifest, cfg_name):
    """from the reference alone: every UCB argmax and best-child choice of the four searches is an exact tie or wider than MARGIN"""
    c = CONFIGS[cfg_name]
    groups = [min(16, c['S'] - g0) for g0 in range(0, c['S'], 16)]
    for s in c['seeds']:
        o, _ = oracle_run(manifest, cfg_name, s)
        selected, gaps, _ = replay(o['rewards'], s, c['N'], c['S'], c['steps'])
        assert selected == [int(v) for v in o['selected']], s                   # the replay is the reference's search
        assert [len(r) for r in o['rewards']] == groups * c['steps']
        bad = [(kind, g) for kind, g in gaps if not (g == 0.0 or g > MARGIN)]
        ties, safe = sum(g == 0.0 for _, g in gaps), sum(g > MARGIN for _, g in gaps)
        print(f'{cfg_name} seed {s}: {len(gaps)} decisions, {ties} exact ties, {safe} above {MARGIN}, smallest gap above 0: '
              f'{min(g for _, g in gaps if g > 0):.3e}')
        assert not bad and ties + safe == len(gaps) and safe > 0, (s, bad)
    # s6: one group per sigma step -- every search expands at the same sigma step at every simulation index; s36: they differ
    assert (len(mixed_indices(manifest, cfg_name)) >= 1) == (cfg_name == 's36')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cfg_name', sorted(CONFIGS))
def test_mcts_in_lock_step_is_each_seeds_own_search(manifest, cfg_name, dtype):
    c = CONFIGS[cfg_name]
    seeds, n, steps, S = c['seeds'], len(c['seeds']), c['steps'], c['S']
    groups = [min(16, S - g0) for g0 in range(0, S, 16)]
    res = lock_run(manifest, cfg_name, dtype, seeds)
    assert res['row_seeds'] == seeds
    assert len(res['selected']) == steps and all(tuple(sel.shape) == (n,) for sel in res['selected'])
    assert [tuple(r.shape) for r in res['rewards']] == [(n, g) for _ in range(steps) for g in groups]
    # one per-row launch per simulation index at which any search expands; those whose searches stand at two sigma steps, from the reference's trees
    g = grown(manifest, cfg_name)
    assert res['mcts_ragged_launches'] == sum(any(t[i][k] is not None for t in g) for i in range(steps) for k in range(S)) >= 1
    assert res['mcts_mixed_launches'] == len(mixed_indices(manifest, cfg_name))
    if cfg_name == 's36':
        assert res['mcts_mixed_launches'] >= 1                                      # the per-row path did carry rows of two sigma steps
    total = 0
    for b, s in enumerate(seeds):
        o, rows = oracle_run(manifest, cfg_name, s)
        what = f'mcts {cfg_name} {dtype} seed {s}'
        worst = 0.0
        for j, ref in enumerate(o['rewards']):
            dev = float((res['rewards'][j][b].float() - ref.reshape(-1).float()).abs().max())
            worst = max(worst, dev)
            assert dev < REWARD_ATOL, (what, j, dev)
        assert [int(sel[b]) for sel in res['selected']] == [int(v) for v in o['selected']], what
        assert res['search_rows'][b] == rows, what
        total += rows
        x_err = float((res['x'][b].cpu() - o['x'][0]).abs().max())
        print(f'{what}: max |reward - ref| = {worst:.2e}, max |x - x_ref| = {x_err:.2e}')
        assert x_err < IMG_TOL, what
        one = solo_run(manifest, cfg_name, dtype, s)                                # this build's own one-image call: other launch forms only
        assert one['net_rows'] == rows and len(one['rewards']) == len(res['rewards'])
        for j, ref in enumerate(one['rewards']):
            dev = float((res['rewards'][j][b].float() - ref.float()).abs().max())
            assert ref.shape == res['rewards'][j][b].shape and dev <= FORM_REWARD, (what, j, dev)
        assert all(torch.equal(sel[b:b + 1], s1) for sel, s1 in zip(res['selected'], one['selected'])), what
        assert float((res['x'][b] - one['x'][0]).abs().max()) < FORM_X, what
    assert res['net_rows'] == total                                                 # the sum of the solo runs' rows: no padding row is counted


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('cfg_name', sorted(CONFIGS))
def test_a_seeds_search_does_not_depend_on_its_position(manifest, cfg_name, dtype):
    """s36: the launches that hold rows of two sigma steps hold them in another order"""
    seeds = CONFIGS[cfg_name]['seeds']
    a = lock_run(manifest, cfg_name, dtype, seeds)
    order = [seeds[2], seeds[0], seeds[3], seeds[1]]
    c = lock_run(manifest, cfg_name, dtype, order)
    assert c['net_rows'] == a['net_rows'] and c['mcts_mixed_launches'] == a['mcts_mixed_launches']
    for s in seeds:
        p, q = seeds.index(s), order.index(s)
        assert all(int(u[p]) == int(v[q]) for u, v in zip(a['selected'], c['selected'])), s
        assert a['search_rows'][p] == c['search_rows'][q], s
        for j, (u, v) in enumerate(zip(a['rewards'], c['rewards'])):
            assert float((u[p] - v[q]).abs().max()) <= FORM_REWARD, (s, j)
        assert float((a['x'][p] - c['x'][q]).abs().max()) < FORM_X, s


def test_bulk_mcts_lockstep_writes_each_seeds_own_search(manifest, tmp_path):
    """bulk.generate_seeds(search_batch=4, mcts_lockstep=True): one lock-step call, each seed's slice shaped like its one-image call's"""
    import PIL.Image
    from diffusion_tts_amd import bulk, sampler as sm, scorers as Sc
    c = CONFIGS['s6']
    seeds = c['seeds']
    net = hip_net(manifest, torch.float32)
    before = np.random.get_state()
    done = bulk.generate_seeds(net, seeds, str(tmp_path), sampling_method=sm.SamplingMethod.MCTS,
                               sampling_params=dict(scorer=Sc.BrightnessScorer(), N=c['N'], S=c['S']), device=DEV, compute_dtype=torch.float32,
                               num_steps=c['steps'], search_batch=4, mcts_lockstep=True, scale_fn=seed0_scale, **CHURN)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    ref = lock_run(manifest, 's6', torch.float32, seeds)
    assert sorted(done) == sorted(seeds)
    for b, s in enumerate(seeds):
        r = done[s]
        assert r['row_seeds'] == seeds and r['net_rows'] == ref['search_rows'][b] == oracle_run(manifest, 's6', s)[1]
        assert tuple(r['x'].shape) == (1, 3, 16, 16) and torch.equal(r['x'][0], ref['x'][b])
        assert all(tuple(q.shape) == (c['S'],) and torch.equal(q, w[b]) for q, w in zip(r['rewards'], ref['rewards']))
        assert all(tuple(q.shape) == (1,) and int(q) == int(w[b]) for q, w in zip(r['selected'], ref['selected']))
        img = np.array(PIL.Image.open(os.path.join(str(tmp_path), f'{s:06d}.png')))
        assert np.array_equal(img, r['image'][0].permute(1, 2, 0).numpy())
