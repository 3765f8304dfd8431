"""GPU: the VP, VE and iDDPM preconditioners -- dts_precond_in against the float64 references and derived bounds of tests/precond_reference.py,
and tiny networks of the three wrappers against the reference's own forwards and searches (tests/golden/make_golden_preconds.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import precond_helpers as ph                                           # noqa: E402
import precond_reference as pr                                         # noqa: E402
from helpers import check_decisions                                    # noqa: E402

DEV = 'cuda'
X3 = 'f16x3'
KINDS = ph.KINDS


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


@pytest.fixture(scope='module')
def gold():
    return ph.golden()


@pytest.fixture(scope='module')
def man():
    return ph.manifest()


@pytest.fixture(scope='module')
def table(gold):
    return torch.from_numpy(gold['iddpm_u']).to(DEV)


def run(ops, kind, x, sigma, table):
    """ops.precond_in on float64 numpy inputs -> (xin, coef) numpy"""
    xin, coef = ops.precond_in(kind, torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(np.ascontiguousarray(sigma)).to(DEV),
                               ops.precond_params(kind), table if kind == 'iddpm' else None)
    assert xin.dtype == torch.float32 and coef.dtype == torch.float32 and coef.shape == (x.shape[0], 4) and xin.shape == x.shape
    return xin.cpu().numpy(), coef.cpu().numpy()


def held(name, got, ref, bound):
    ex, i = pr.check(got, ref, bound)
    print(f'{name}: largest excess over the bound {ex:.3e} (element {i}: got {got.reshape(-1)[i]!r}, reference {ref.reshape(-1)[i]!r}, '
          f'bound {bound.reshape(-1)[i]:.3e})')
    assert ex <= 0, (name, i)


ROW_SIGMAS = np.array([0.013, 2.7, 75.0])


@pytest.mark.parametrize('chw', [1, 192, 257])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('kind', KINDS)
def test_precond_in_matches_float64(ops, gold, table, kind, n, chw):
    """coefficients and c_in * x, scalar sigma (broadcast to the rows) and per-row sigma"""
    u = gold['iddpm_u']
    x = np.random.default_rng(100 * n + chw).standard_normal((n, chw)) * 30
    for sigma in (ROW_SIGMAS[1:2], ROW_SIGMAS[:n]):
        rows = np.broadcast_to(sigma, (n,)) if sigma.size == 1 else sigma
        xin, coef = run(ops, kind, x, sigma, table)
        held(f'{kind} coef n={n} chw={chw} nsigma={sigma.size}', coef, *pr.coef_ref(kind, rows, u=u))
        held(f'{kind} xin n={n} chw={chw} nsigma={sigma.size}', xin, *pr.xin_ref(kind, x, rows, u=u))


@pytest.mark.parametrize('kind', KINDS)
def test_precond_in_second_trip_of_the_grid_stride_loop(ops, gold, table, kind):
    """n * chw > 2048 blocks of 256 threads: the scaling pass goes round its loop twice, and row 2 starts beyond the first trip"""
    n, chw = 3, pr.WRAP_CHW
    assert n * chw > 2048 * 256
    x = np.random.default_rng(7).standard_normal((n, chw)) * 10
    xin, coef = run(ops, kind, x, ROW_SIGMAS, table)
    held(f'{kind} coef wrap', coef, *pr.coef_ref(kind, ROW_SIGMAS, u=gold['iddpm_u']))
    held(f'{kind} xin wrap', xin, *pr.xin_ref(kind, x, ROW_SIGMAS, u=gold['iddpm_u']))


@pytest.mark.parametrize('kind', ['vp', 've'])
def test_coefficients_over_the_sigma_range(ops, gold, table, kind):
    """257 rows in one call, 1e-4 .. 3e4: past both ends of either network's range (VP's bound is absolute at the small end)"""
    sig = pr.sigma_sweep(1e-4, 3e4)
    _, coef = run(ops, kind, np.ones((len(sig), 1)), sig, table)
    held(f'{kind} sweep', coef, *pr.coef_ref(kind, sig))


def test_iddpm_index(ops, gold, table):
    """every table entry, the exactly representable midpoints (first index wins), above u[0], below u[M-1], 0 -- 1 781 rows in one call, so
    a block's four waves work on four different rows -- and the sigma sweep"""
    u = gold['iddpm_u']
    cases = pr.index_cases(u)
    mids, lower = pr.table_midpoints(u)
    sig = np.concatenate([cases, pr.sigma_sweep(1e-4, 3e4)])
    _, coef = run(ops, 'iddpm', np.ones((len(sig), 1)), sig, table)
    ref, bound = pr.coef_ref('iddpm', sig, u=u)
    held('iddpm index cases', coef, ref, bound)
    idx = (999 - coef[:, 3]).astype(np.int64)
    M1 = len(u)
    assert np.array_equal(idx[:M1], np.arange(M1))                                   # every entry is its own nearest
    assert len(mids) >= 50 and np.array_equal(idx[M1:M1 + len(mids)], lower)         # exact ties: the first index
    assert list(idx[M1 + len(mids):len(cases)]) == [0, 0, 0, 999, 999, 1000, 1000, 1000, 1000]
    # one row, and a table shorter than a wavefront (lanes without an entry)
    _, c1 = run(ops, 'iddpm', np.ones((1, 1)), np.array([float(u[37])]), table)
    assert c1[0, 3] == 999 - 37
    short = torch.from_numpy(u[-5:].copy()).to(DEV)
    _, c2 = run(ops, 'iddpm', np.ones((3, 1)), np.array([1.0, float(u[-3]), 0.0]), short)
    assert list(999 - c2[:, 3]) == [0, 2, 4]


@pytest.mark.parametrize('kind', KINDS)
def test_golden_c_noise_sweep(ops, gold, table, kind):
    """c_noise of the reference module's own float32 expression on 64 log-spaced sigmas across its range: the kernel inside the float64
    bound, hence within two bounds of the reference's value; iDDPM: equal wherever the reference's matrix-product cdist is decided (two
    nearest entries >= 5 % apart), and the exact nearest entry everywhere"""
    sig, cn = gold[f'{kind}_sweep_sigma'].astype(np.float64), gold[f'{kind}_sweep_c_noise']
    _, coef = run(ops, kind, np.ones((len(sig), 1)), sig, table)
    ref, bound = pr.coef_ref(kind, sig, u=gold['iddpm_u'])
    held(f'{kind} golden sweep', coef, ref, bound)
    ok = gold['iddpm_sweep_decided'] if kind == 'iddpm' else np.ones(len(sig), bool)
    d = np.abs(coef[:, 3].astype(np.float64) - cn.astype(np.float64))
    print(f'{kind}: max |c_noise - reference module| {d[ok].max():.3e} on {int(ok.sum())} sigmas')
    assert ok.sum() >= 48 and np.all(d[ok] <= 2 * bound[ok, 3])


def test_precond_in_refuses_bad_arguments(ops, table):
    x, s = torch.zeros(2, 4, dtype=torch.float64, device=DEV), torch.ones(2, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        ops.precond_in('edm', x, s)
    with pytest.raises(ValueError):
        ops.precond_in('iddpm', x, s, ops.precond_params('iddpm'))
    with pytest.raises(RuntimeError):
        ops.precond_in('vp', x, torch.ones(3, dtype=torch.float64, device=DEV), ops.precond_params('vp'))


# ---- networks ----------------------------------------------------------------------------------------------------------------------
_NETS = {}


def _net(man, kind, dtype):
    from diffusion_tts_amd.networks import EDMPrecond
    if (kind, dtype) not in _NETS:
        cfg, sd = ph.tiny_weights(man, kind)
        _NETS[(kind, dtype)] = EDMPrecond(cfg, sd, device=DEV, dtype=dtype)
    return _NETS[(kind, dtype)]


def _fwd_inputs(g, kind):
    x, sigma, D, D64 = (torch.from_numpy(g[f'{kind}_{k}']) for k in ('x', 'sigma', 'D', 'D64'))
    return x, sigma, torch.eye(10)[torch.from_numpy(g[f'{kind}_label_idx'])], D, D64


@pytest.mark.parametrize('dtype', [torch.float32, X3])
@pytest.mark.parametrize('kind', KINDS)
def test_forward_matches_the_reference(gold, man, kind, dtype):
    """the reference wrapper's D on 2 rows with per-row sigma.  Bound: max(3e-6, 4 x the reference's own fp32-vs-float64 distance on this
    network, from the manifest) of max(1, max|D|) -- the rule of test_gpu_ncsnpp.py.  Four calls: eager launches, capture and HIP-graph
    replay.  iDDPM: also against the float64 forward that computes all six output channels and reads three (the same bound: 4 x the
    reference's own distance to it), so dropping the variance rows of the last convolution at load changes nothing."""
    x, sigma, lab, D, D64 = _fwd_inputs(gold, kind)
    net = _net(man, kind, dtype)
    assert net.precond == kind and (net.sigma_min, net.sigma_max) == (man[kind]['sigma_min'], man[kind]['sigma_max'])
    bound = max(3e-6, 4 * man[kind]['ref_f32_vs_f64'])
    scale = max(1.0, float(D.abs().max()))
    for call in range(4):                               # graphs.SIGHTINGS: the third call of a shape is captured, the fourth replayed
        got = net(x, sigma, lab).cpu()
        assert got.dtype == torch.float32 and got.shape == D.shape
        err = float((got - D).abs().max()) / scale
        e64 = float((got.double() - D64).abs().max()) / scale
        print(f'{kind} forward vs the reference, {dtype}, call {call}: err {err:.3e} (bound {bound:.3e}; vs float64 {e64:.3e}; reference vs '
              f'float64 {man[kind]["ref_f32_vs_f64"]:.3e})')
        assert err <= bound, (call, err, bound)
        if kind == 'iddpm':
            assert e64 <= bound, (call, e64, bound)
    assert net._graphs.replays >= 1


def test_iddpm_network_drops_the_variance_rows(man):
    net = _net(man, 'iddpm', torch.float32)
    assert net.out_w.shape[0] == 3 and net.out_cb.shape[0] == 3 and net.u_dev.numel() == 1001
    u = net.u
    assert torch.equal(net.round_sigma(u), u) and torch.equal(net.round_sigma(u, return_index=True), torch.arange(1001))
    s = torch.tensor([0.002, 80.0, 1.0], dtype=torch.float64)
    r = net.round_sigma(s)
    assert r.dtype == torch.float64 and float(r[0]) == 0.0 and float(r[1]) == float(u[np.abs(u.numpy() - 80.0).argmin()])


def test_load_network_carries_the_preconditioner_and_auto_mode(man, tmp_path):
    """a .pkl of the iDDPM wrapper and a .pt bundle of the VP one through sampler.load_network; dtype='auto' follows the recorded use_fp16"""
    import dataclasses
    from diffusion_tts_amd import ops as o, sampler as sm
    cfg, sd = ph.tiny_weights(man, 'iddpm')
    p = tmp_path / 'iddpm.pkl'
    p.write_bytes(ph.precond_pickle(cfg, sd))
    net = sm.load_network(str(p), device=DEV, dtype='auto')
    assert net.precond == 'iddpm' and net.dtype == o.F16X3 and torch.equal(net.u, sd['u']) and net.sigma_max == cfg.sigma_max
    cfg, sd = ph.tiny_weights(man, 'vp')
    p = tmp_path / 'vp.pt'
    torch.save(dict(cfg=dataclasses.asdict(dataclasses.replace(cfg, use_fp16=True)), state_dict=sd), p)
    net = sm.load_network(str(p), device=DEV, dtype='auto')
    assert net.precond == 'vp' and net.dtype == torch.float16 and net.cfg.use_fp16
    assert sm.load_network(str(p), device=DEV).dtype == o.F16X3                     # the default does not act on the flag


@pytest.mark.parametrize('dtype,tol', [(torch.float16, 1e-2), (torch.bfloat16, 6e-2)])
@pytest.mark.parametrize('kind', KINDS)
def test_throughput_modes_smoke(gold, man, kind, dtype, tol):
    """bf16 / f16: finite, and within the tolerances of test_gpu_ncsnpp.py::test_throughput_modes_smoke"""
    x, sigma, lab, D, _ = _fwd_inputs(gold, kind)
    got = _net(man, kind, dtype)(x, sigma, lab).cpu()
    err = float((got - D).abs().max())
    print(f'{kind} forward, {dtype}: max err {err:.3e}')
    assert bool(torch.isfinite(got).all()) and err < tol * max(1.0, float(D.abs().max()))


@pytest.mark.parametrize('dtype', [X3, torch.float32])
@pytest.mark.parametrize('kind', KINDS)
def test_searches_against_the_reference_runs(gold, man, kind, dtype):
    """NAIVE (35 rows) and REJECTION N = 4 with the brightness scorer (140 rows) against the reference's generate_image_grid runs, schedule
    clamped to the network's range: the criteria of test_gpu_ncsnpp.py::test_searches_against_the_reference_runs -- row counts, final state
    within 1e-3, uint8 image within 1 LSB, the rewards within 5e-5, and the kept trajectory where the top-2 margin decides it."""
    from diffusion_tts_amd import sampler as sm, scorers as S
    from diffusion_tts_amd.hashing import seed0_scale
    g, m = gold, man[kind]
    net = _net(man, kind, dtype)
    lab = torch.eye(10)[torch.tensor([m['naive']['label']])]

    def kw(rec, seed):
        assert (rec['sigma_min'], rec['sigma_max']) == (max(0.002, net.sigma_min), min(80, net.sigma_max))
        return dict(seed=seed, num_steps=man['num_steps'], gridw=1, gridh=1, device=torch.device(DEV), scale_fn=seed0_scale, compute_dtype=dtype,
                    verbose=False, sigma_min=rec['sigma_min'], sigma_max=rec['sigma_max'], **man['S'])

    def image_ok(h, ref):
        diff = np.abs(h['image'][0].permute(1, 2, 0).numpy().astype(np.int32) - ref.astype(np.int32))
        return diff.max() <= 1 and (diff > 0).mean() < 0.005
    lat = torch.randn(1, 3, 16, 16, generator=torch.Generator().manual_seed(m['naive']['latent_seed']))
    assert np.array_equal(lat.numpy(), g[f'{kind}_naive_latents'])
    h = sm.generate_image_grid(net, None, lat, lab, sampling_method=sm.SamplingMethod.NAIVE, sampling_params=dict(scorer=S.BrightnessScorer()),
                               **kw(m['naive'], man['seed']))
    e0 = float((h['x'].cpu() - torch.from_numpy(g[f'{kind}_naive_x_final'])).abs().max())
    print(f'{kind} naive vs the reference run, {dtype}: max |x - x_ref| {e0:.2e}')
    assert h['net_rows'] == m['naive']['net_rows'] == 35 and e0 < 1e-3 and image_ok(h, g[f'{kind}_naive_image'])
    assert abs(float(h['final_scores'][0]) - float(g[f'{kind}_naive_final_score'][0])) < 5e-5
    rj = m['rejection']
    lat = torch.randn(1, 3, 16, 16, generator=torch.Generator().manual_seed(rj['latent_seed']))
    assert np.array_equal(lat.numpy(), g[f'{kind}_rej_latents'])
    h = sm.generate_image_grid(net, None, lat, lab, sampling_method=sm.SamplingMethod.REJECTION_SAMPLING,
                               sampling_params=dict(scorer=S.BrightnessScorer(), **rj['params']), **kw(rj, rj['seed']))
    rew = h['rewards'][0].reshape(-1).numpy()
    e_r = float(np.abs(rew - g[f'{kind}_rej_rewards']).max())
    e1 = float((h['x'].cpu() - torch.from_numpy(g[f'{kind}_rej_x_final'])).abs().max())
    print(f'{kind} rejection vs the reference run, {dtype}: reward err {e_r:.2e} (top-2 gap {rj["top2_gap"]:.1e}), '
          f'kept {int(h["selected"][0][0])} (reference {rj["kept"]}), max |x - x_ref| {e1:.2e}')
    assert h['net_rows'] == rj['net_rows'] == 140 and e_r < 5e-5
    same, _ = check_decisions([torch.from_numpy(g[f'{kind}_rej_rewards']).reshape(-1, 1)], [torch.from_numpy(g[f'{kind}_rej_kept'])],
                              [h['selected'][0].reshape(-1)], f'{kind} rejection ({dtype})')
    assert same and int(h['selected'][0][0]) == rj['kept'] == int(g[f'{kind}_rej_kept'][0])
    assert e1 < 1e-3 and image_ok(h, g[f'{kind}_rej_image'])
