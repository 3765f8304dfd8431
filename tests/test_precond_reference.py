"""Pins tests/precond_reference.py: the float32 model of the kernel's own steps sits inside every bound, each planted mistake falls outside
one, the Fraction index agrees with a brute-force scan, and the references agree with the reference module's own float32 expression
(tests/golden/make_golden_preconds.py) to those bounds.  No GPU."""
import numpy as np
import pytest

import precond_helpers as ph
import precond_reference as pr

KINDS = ph.KINDS


@pytest.fixture(scope='module')
def gold():
    return ph.golden()


def _sigmas(kind, u):
    """what tests/test_gpu_precond.py feeds the kernel: the network's range, beyond both ends, and for iDDPM the index cases"""
    sw = pr.sigma_sweep(1e-4, 3e4)
    return np.concatenate([sw, pr.index_cases(u)]) if kind == 'iddpm' else sw


@pytest.mark.parametrize('kind', KINDS)
def test_model_of_the_kernel_is_inside_the_bounds(kind, gold):
    u = gold['iddpm_u']
    sig = _sigmas(kind, u)
    ref, bound = pr.coef_ref(kind, sig, u=u)
    got = pr.coef_model(kind, sig, u=u)
    ex, i = pr.check(got, ref, bound)
    print(f'{kind}: {len(sig)} sigmas, largest excess over the bound {ex:.3e} at element {i}')
    assert ex <= 0, (kind, i, got.reshape(-1)[i], ref.reshape(-1)[i], bound.reshape(-1)[i])
    assert np.all(bound[:, :2] == 0)                                   # c_skip, c_out: exact


def test_vp_bound_is_absolute_at_small_sigma():
    """c_noise -> 0 with sigma while its bound does not: a flat relative tolerance would either reject the kernel or admit anything"""
    ref, bound = pr.coef_ref('vp', np.array([1e-4, 1e-3, 1e-2, 1.0, 100.0]))
    # (at 1e-4, 1 + s^2 rounds to 1 and c_noise is what f32(beta_min^2) and f32(beta_min) leave of zero: -1.3e-7)
    assert abs(ref[0, 3]) < 1e-3 and 1e-6 < bound[0, 3] < 3e-6 and bound[0, 3] > abs(ref[0, 3])
    assert bound[1, 3] > 0.9 * bound[0, 3]                             # the floor: 3 ulp of beta_min through (M-1) / beta_d
    assert bound[4, 3] < 1e-5 * ref[4, 3]                              # relative again once d >> beta_min's ulp


# (VE has no M; only iDDPM has ties)
@pytest.mark.parametrize('kind,mistake', [(k, m) for k in KINDS for m in pr.MISTAKES
                                          if not (m == 'last_tie' and k != 'iddpm') and not (m == 'M_not_M1' and k == 've')])
def test_planted_mistakes_are_caught(kind, mistake, gold):
    u = gold['iddpm_u']
    sig = _sigmas(kind, u)
    ref, bound = pr.coef_ref(kind, sig, u=u)
    ex, i = pr.check(pr.coef_model(kind, sig, u=u, mistake=mistake), ref, bound)
    print(f'{kind}, {mistake}: excess {ex:.3e} at element {i} (column {i % 4})')
    assert ex > 0
    assert i % 4 == {'c_out_sign': 1, 'M_not_M1': 3, 'last_tie': 3}.get(mistake, i % 4)


def test_fraction_index_is_the_brute_force_index(gold):
    u = gold['iddpm_u']
    sig = pr.f32_sigma(_sigmas('iddpm', u))
    d = np.abs(sig.astype(np.float64)[:, None] - u.astype(np.float64)[None, :])
    assert np.array_equal(pr.nearest_index(sig, u), d.argmin(1))
    mids, lower = pr.table_midpoints(u)
    assert len(mids) >= 50                                              # enough exact ties to mean something
    assert np.array_equal(pr.nearest_index(pr.f32_sigma(mids), u), lower)
    assert np.array_equal(pr.nearest_index(u, u), np.arange(len(u)))
    assert list(pr.nearest_index(pr.f32_sigma([0.0, 1e-30, 1e18, float(u[-2]) * 0.5, float(u[-2]) * 0.49]), u)) == [1000, 1000, 0, 999, 1000]


def test_index_reference_against_the_reference_module(gold):
    """round_sigma(return_index=True) of the reference on sigmas whose two nearest entries are >= 5 % apart (where its cdist route is decided)"""
    got = pr.nearest_index(gold['iddpm_round_sigma'], gold['iddpm_u'])
    assert len(got) > 3000 and np.array_equal(got, gold['iddpm_round_index'].astype(np.int64))


@pytest.mark.parametrize('kind', KINDS)
def test_c_noise_reference_against_the_reference_module(kind, gold):
    """the reference module's own float32 c_noise on 64 log-spaced sigmas across its range lies inside the bound as well (it is another
    float32 evaluation of the same expression, with the host library's logf)"""
    sig, cn = gold[f'{kind}_sweep_sigma'], gold[f'{kind}_sweep_c_noise']
    ref, bound = pr.coef_ref(kind, sig, u=gold['iddpm_u'])
    ok = gold['iddpm_sweep_decided'] if kind == 'iddpm' else np.ones(len(sig), bool)
    ex = np.abs(cn.astype(np.float64) - ref[:, 3]) - bound[:, 3]
    print(f'{kind}: reference c_noise vs float64, largest excess {ex[ok].max():.3e}; {int(ok.sum())} of {len(sig)} sigmas compared')
    assert ok.sum() >= 48 and ex[ok].max() <= 0


def test_xin_reference():
    g = np.random.default_rng(5)
    x = g.standard_normal((3, 7)) * 40
    sig = np.array([0.01, 2.0, 70.0])
    for kind in ('vp', 've'):
        want, bound = pr.xin_ref(kind, x, sig)
        cm = pr.coef_model(kind, sig)
        got = cm[:, 2:3] * x.astype(np.float32)
        assert got.dtype == np.float32 and pr.check(got, want, bound)[0] <= 0
        bad = pr.coef_model(kind, sig, mistake='row0_sigma')[:, 2:3] * x.astype(np.float32)
        assert (pr.check(bad, want, bound)[0] > 0) == (kind == 'vp')     # VE's c_in is 1 whatever the row
