"""GPU: the per-row forms of the Heun step kernels (ops.heun_xhat_rows / heun_euler_rows / heun_correct_rows: the step's scalars as one
float64 per row on the device), which carry the MCTS expansions of several searches -- each at the sigma step of its own leaf -- in one launch.

Held per case to
  (a) the scalar entry point: row i is BIT-EQUAL to ops.heun_xhat / heun_euler / heun_correct launched on that row alone with the row's
      scalars (one body per op; the scalar kernel is its broadcast case);
  (b) the float64 reference and bound of tests/elementwise_reference.py for the scalar kernel (8 e64 times the terms of each expression),
      applied row by row;
  (c) a row whose noise coefficient is exactly 0.0: x_hat is its source row of x_cur, bit for bit;
  (d) a HOST array holding t_hat == 0 (euler) or t_next == 0 (correct) is refused by name before any launch -- the entry points cannot
      check a device array without reading it.
Shapes: chw = 105 (3 * 5 * 7: no multiple of any vector width) and 768 (3 * 16 * 16); one chw at which nb * chw passes the 2048 blocks of
256 threads that grid1d() caps an element-wise launch at (elementwise_reference.WRAP restates that rule), so the grid-stride loop -- the
only size-driven loop of the three kernels -- takes its second trip, with the row index and the per-row scalars changing inside it;
nb = 6 rows over xb = 3 sources in both broadcast forms, and nb = 1; eps float32 and float64.  The six rows stand at six different steps
of the 18-step schedule: one outside the churn range (noise coefficient exactly 0.0) and one whose t_next is set to its t_hat (dt = 0)."""
import pytest
import torch

import elementwise_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BIG_CHW = R.WRAP // 6 + 1                      # 6 rows of it: a few elements past one full trip of the capped grid
STEPS6 = (3, 0, 9, 12, 6, 14)                 # step 0 (sigma 80 > S_max = 50): no churn, coefficient exactly 0.0
SAME_T = 4                                     # the row whose t_next is its t_hat


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


def scalars(nb):
    t = R.sigma_schedule()
    t_hat, coef, t_next = [], [], []
    for r in range(nb):
        th, c = R.churned(float(t[STEPS6[r]]))
        t_hat.append(th)
        coef.append(c)
        t_next.append(th if r == SAME_T else float(t[STEPS6[r] + 1]))
    return t_hat, coef, t_next


def inputs(xb, nb, chw, eps_dtype, seed):
    g_ = R.gen(seed)
    x = 10.0 * torch.arange(1, xb + 1, dtype=torch.float64)[:, None] + 0.25 * torch.rand(xb, chw, generator=g_, dtype=torch.float64)
    eps = torch.randn(nb, chw, generator=g_, dtype=torch.float64).to(eps_dtype)
    return x, eps


CASES = [(xb, nb, interleave, chw, eps_dtype)
         for xb, nb, interleave in ((3, 6, False), (3, 6, True), (1, 1, False))
         for chw in (105, 768, BIG_CHW)
         for eps_dtype in (torch.float32, torch.float64)]


def test_the_large_case_takes_the_second_trip_of_the_grid_stride_loop():
    assert R.WRAP > 2048 * 256 and 6 * BIG_CHW > 2048 * 256 and BIG_CHW % 2 == 1 and 6 * BIG_CHW < 2 * 2048 * 256


@pytest.mark.parametrize('xb,nb,interleave,chw,eps_dtype', CASES, ids=lambda v: str(v).split('.')[-1])
def test_rows_equal_the_scalar_kernels_and_the_reference(ops, xb, nb, interleave, chw, eps_dtype):
    t_hat, coef, t_next = scalars(nb)
    assert len(set(coef)) == len(set(t_hat)) == len(set(t_next)) == nb and (nb == 1 or (coef[1] == 0.0 and t_next[SAME_T] == t_hat[SAME_T]))
    x, eps = inputs(xb, nb, chw, eps_dtype, 700 + chw % 97 + nb)
    xd, ed = x.to(DEV), eps.to(DEV)
    src = R.row_map(nb, xb, interleave)
    what = f'xb={xb} nb={nb} interleave={interleave} chw={chw} eps={eps_dtype}'

    def held(name, got, ref, bound, r):
        ratio, err = R.worst(got, ref, bound)
        assert ratio <= 1.0, f'{name} {what} row {r}: err/bound {ratio:.3f} (max err {err:.3e})'
        return ratio

    x_hat = ops.heun_xhat_rows(xd, ed, coef, nb, interleave=interleave)
    xh = x_hat.cpu()
    assert bool(torch.isfinite(xh).all())
    D = xh.float() * 0.3 + 0.1
    Dd = D.to(DEV)
    d_cur, x_next = ops.heun_euler_rows(x_hat, Dd, t_hat, t_next)
    dc, xn = d_cur.cpu(), x_next.cpu()
    D2 = xn.float() * 0.3 + 0.1
    D2d = D2.to(DEV)
    out = ops.heun_correct_rows(x_hat, D2d, d_cur, t_hat, t_next, x_next.clone()).cpu()
    worst = 0.0
    for r in range(nb):
        s = int(src[r])
        # (a) the scalar entry points on this row alone
        one = ops.heun_xhat(xd[s:s + 1].contiguous(), ed[r:r + 1].contiguous(), coef[r], 1)
        assert torch.equal(one.cpu(), xh[r:r + 1]), f'heun_xhat_rows {what} row {r}: not the scalar kernel\'s bits'
        d1, n1 = ops.heun_euler(x_hat[r:r + 1].contiguous(), Dd[r:r + 1].contiguous(), t_hat[r], t_next[r])
        assert torch.equal(d1.cpu(), dc[r:r + 1]) and torch.equal(n1.cpu(), xn[r:r + 1]), f'heun_euler_rows {what} row {r}'
        o1 = ops.heun_correct(x_hat[r:r + 1].contiguous(), D2d[r:r + 1].contiguous(), d_cur[r:r + 1].contiguous(), t_hat[r], t_next[r],
                              x_next[r:r + 1].clone())
        assert torch.equal(o1.cpu(), out[r:r + 1]), f'heun_correct_rows {what} row {r}'
        # (b) the float64 reference of the scalar kernel, with this row's scalars
        ref, bound = R.heun_xhat_ref(x[s:s + 1], eps[r:r + 1], coef[r], 1, False)
        worst = max(worst, held('heun_xhat_rows', xh[r:r + 1], ref, bound, r))
        (d, bd), (n, bn) = R.heun_euler_ref(xh[r:r + 1], D[r:r + 1], t_hat[r], t_next[r])
        worst = max(worst, held('heun_euler_rows d_cur', dc[r:r + 1], d, bd, r), held('heun_euler_rows x_next', xn[r:r + 1], n, bn, r))
        o, bo = R.heun_correct_ref(xh[r:r + 1], D2[r:r + 1], dc[r:r + 1], t_hat[r], t_next[r], xn[r:r + 1])
        worst = max(worst, held('heun_correct_rows', out[r:r + 1], o, bo, r))
        # (c) no noise: the source row itself
        if coef[r] == 0.0:
            assert torch.equal(xh[r], x[s]), f'{what} row {r}: noise_coef == 0 must return x_cur bit for bit'
        if t_next[r] == t_hat[r]:
            assert torch.equal(xn[r], xh[r]) and torch.equal(out[r], xh[r]), f'{what} row {r}: t_next == t_hat leaves x_hat'
    # the row mapping on its own: row r of x_cur is 10 (r + 1) + [0, 0.25)
    c = torch.tensor(coef, dtype=torch.float64)[:, None]
    assert torch.equal(((xh - c * eps.double()) / 10).round().long()[:, 0] - 1, src), what
    print(f'heun_*_rows {what}: worst err/bound {worst:.3f}')


def test_device_coefficients_are_taken_as_they_are(ops):
    """float64 device tensors (checked and uploaded once by the caller, plain.heun_step_rows) give the bits of the host sequences"""
    t_hat, coef, t_next = scalars(6)
    x, eps = inputs(3, 6, 105, torch.float32, 731)
    xd, ed = x.to(DEV), eps.to(DEV)
    dev = lambda v: torch.tensor(v, dtype=torch.float64, device=DEV)
    a = ops.heun_xhat_rows(xd, ed, coef, 6, interleave=True)
    b = ops.heun_xhat_rows(xd, ed, dev(coef), 6, interleave=True)
    assert torch.equal(a, b)
    D = (a.float() * 0.3 + 0.1)
    (d1, n1), (d2, n2) = ops.heun_euler_rows(a, D, t_hat, t_next), ops.heun_euler_rows(a, D, dev(t_hat), dev(t_next))
    assert torch.equal(d1, d2) and torch.equal(n1, n2)
    with pytest.raises(ValueError, match=r'heun_xhat_rows: noise_coef: a device tensor must be float64 \[6\]'):
        ops.heun_xhat_rows(xd, ed, dev(coef).float(), 6)
    with pytest.raises(ValueError, match='heun_xhat_rows: noise_coef: need one value per row, got 5 values for 6 rows'):
        ops.heun_xhat_rows(xd, ed, coef[:5], 6)


def test_a_zero_time_in_a_host_array_is_refused_by_name_before_any_launch(ops, monkeypatch):
    t_hat, coef, t_next = scalars(6)
    x, eps = inputs(3, 6, 105, torch.float64, 733)
    x_hat = ops.heun_xhat_rows(x.to(DEV), eps.to(DEV), coef, 6)
    D = (x_hat.float() * 0.3 + 0.1)
    d_cur, x_next = ops.heun_euler_rows(x_hat, D, t_hat, t_next)

    def no_launch(*a, **k):
        raise AssertionError('a refused call reached the library')
    monkeypatch.setattr(ops, '_call', no_launch)
    zero = lambda v, r: v[:r] + [0.0] + v[r + 1:]
    with pytest.raises(ValueError, match=r'heun_euler_rows: t_hat == 0 in row 2'):
        ops.heun_euler_rows(x_hat, D, zero(t_hat, 2), t_next)
    with pytest.raises(ValueError, match=r'heun_euler_rows: t_hat == 0 in row 5'):
        ops.heun_euler_rows(x_hat, D, torch.tensor(zero(t_hat, 5)), t_next)
    with pytest.raises(ValueError, match=r'heun_correct_rows: t_next == 0 in row 3'):
        ops.heun_correct_rows(x_hat, D, d_cur, t_hat, zero(t_next, 3), x_next)
    with pytest.raises(ValueError, match=r'heun_correct_rows: t_next == 0 in row 0'):
        ops.heun_correct_rows(x_hat, D, d_cur, t_hat, torch.tensor(zero(t_next, 0), dtype=torch.float64), x_next)
    from diffusion_tts_amd import plain
    with pytest.raises(ValueError, match=r'heun_step_rows: t_next == 0 in row 1'):
        plain.heun_step_rows(None, x.to(DEV), eps.to(DEV), t_hat, coef, zero(t_next, 1), None)
