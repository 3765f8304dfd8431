"""Pins tests/gn_reference.py on the CPU: gn_ref64 against torch's float64 group_norm, and every statistics regime's condition --
the error of the reference's OWN float32 arithmetic (oracle.edm_nets.group_norm on float32 input) against gn_ref64 stays under the
regime's limit, which is what makes the inputs fair for the kernels (tests/test_gpu_groupnorm.py)."""
import pytest
import torch
import torch.nn.functional as F

from gn_reference import REGIMES, err, gn_ref64, groups_of, ref32, regime_input

SHAPES = [(192, 8), (192, 64), (1344, 8), (256, 16)]


@pytest.mark.parametrize('n,c1,c2,h,w', [(2, 192, 0, 8, 8), (3, 64, 0, 5, 7), (2, 768, 576, 4, 4)])
def test_gn_ref64_is_float64_group_norm(n, c1, c2, h, w):
    gen = torch.Generator().manual_seed(7)
    c = c1 + c2
    x1 = torch.randn(n, c1, h, w, generator=gen) * 2 + 0.5
    x2 = torch.randn(n, c2, h, w, generator=gen) if c2 else None
    gamma, beta = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    ss = torch.randn(n, 2 * c, generator=gen) * 0.3
    x = (x1 if x2 is None else torch.cat([x1, x2], 1)).double()
    want = F.group_norm(x, groups_of(c), gamma.double(), beta.double(), 1e-5)
    y, a, b = gn_ref64(x1, x2, groups_of(c), 1e-5, gamma, beta)
    assert err(y, want) < 1e-13
    assert err(x * a[:, :, None, None] + b[:, :, None, None], want) < 1e-13
    want = want * (1 + ss.double()[:, :c, None, None]) + ss.double()[:, c:, None, None]
    y, a, b = gn_ref64(x1, x2, groups_of(c), 1e-5, gamma, beta, ss)
    assert err(y, want) < 1e-13 and err(x * a[:, :, None, None] + b[:, :, None, None], want) < 1e-13
    if h % 2 == 0:
        want = F.avg_pool2d(F.silu(want), 2)
        assert err(gn_ref64(x1, x2, groups_of(c), 1e-5, gamma, beta, ss, silu=True, pool=True)[0], want) < 1e-13


@pytest.mark.parametrize('eps', [1e-5, 1e-6])
@pytest.mark.parametrize('c,res', SHAPES)
@pytest.mark.parametrize('regime', list(REGIMES))
def test_regime_is_fair_to_float32(regime, c, res, eps):
    """e_ref32 of every regime stays under its limit (a condition on the inputs, not a tolerance on a kernel)."""
    x, r = regime_input(regime, 2, c, res, res, seed=1000 + c + res)
    gen = torch.Generator().manual_seed(c)
    gamma, beta = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    ref64 = gn_ref64(x, None, groups_of(c), eps, gamma, beta)[0]
    e = err(ref32(x, None, eps, gamma, beta), ref64)
    xg = x.double().reshape(2, groups_of(c), -1)
    r_meas = float((xg.mean(2).abs() / xg.std(2)).max())
    print(f'{regime} ({c},{res}) eps={eps:g}: e_ref32 = {e:.2e} (limit {REGIMES[regime][2]:.0e}), measured |mean|/std <= {r_meas:.2f}')
    assert e < REGIMES[regime][2]
    assert abs(r_meas - r) < 0.25 * max(1.0, r)        # (sampling noise of mean / std over >= 384 elements, worst of 64 groups)


def test_exact_cases_are_finite_in_the_reference():
    """a constant group (3.0, and 3000.0 at eps = 1e-6) and an all-zero sample: the float64 reference is finite and the zero
    sample's affine part is exactly beta"""
    c = 192
    gen = torch.Generator().manual_seed(3)
    gamma, beta = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    for value, eps in ((3.0, 1e-5), (3000.0, 1e-6)):
        x, _ = regime_input('centred', 2, c, 8, 8, seed=5)
        x[1, 18:24] = value
        y, a, b = gn_ref64(x, None, 32, eps, gamma, beta)
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(ref32(x, None, eps, gamma, beta)).all())
        assert float((y[1, 18:24] - beta.double()[18:24, None, None]).abs().max()) < 1e-9 * value / eps ** 0.5
    x, _ = regime_input('centred', 2, c, 8, 8, seed=5)
    x[1] = 0
    y, a, b = gn_ref64(x, None, 32, 1e-5, gamma, beta)
    assert torch.equal(y[1], beta.double()[:, None, None].expand(c, 8, 8)) and torch.equal(b[1], beta.double()) and bool(torch.isfinite(a).all())
