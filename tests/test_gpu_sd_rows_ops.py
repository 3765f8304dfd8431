"""GPU: the two kernel forms of the SD backend's lock-step searches.

`dts_candidate_noise_sd_rows` (S searches x N candidate rows; row s*N + n reads pivot[s], mode[row], scale[row]) is held to the reference's
own expression evaluated by torch on the CPU in the latents' dtype, row by row against pivot[s] -- the construction of
tests/test_gpu_sd.py::test_candidate_noise_sd_rounds_like_the_reference_expression: float16 bit for bit, float32 within that test's bound
(2^-22 of the largest value: one ulp of the norm) -- and, with S = 1, to `ops.candidate_noise_sd` bit for bit (one body, two forms).

`dts_ddim_candidates_groups` (G independent (x, e) pairs x ncand candidates, group-major) is held per group to
elementwise_reference.ddim_ref with its derived bound plus the storage rounding, and bit for bit to G separate `ops.ddim_candidates` calls.
One case has G * count beyond the 2048 x 256 threads of a launch, so the grid-stride loop takes its second trip.

Every output sits in the middle of a NaN-filled buffer; the guard bands must stay NaN."""
import numpy as np
import pytest
import torch

import elementwise_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD = 1024


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


def guarded(shape, dtype):
    """an output tensor in the middle of a NaN-filled buffer: (buffer, view)"""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), float('nan'), dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + numel].view(shape)


def assert_guards(buf, what):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), f'{what}: wrote outside the output'
    assert not bool(torch.isnan(buf[GUARD:-GUARD]).any()), f'{what}: left part of the output unwritten'


# ---- candidate_noise_sd_rows -------------------------------------------------------------------------------------------------------------------
S_, N_ = 3, 4
MODE = [1, 0, 1, 1,   0, 0, 0, 0,   0, 1, 1, 0]          # mixed; search 1 all fresh (a plain copy)
COUNTS = (1, 255, 256, 4 * 64 * 64)                       # the single-thread row, a ragged tail, one full trip, 64 trips


def sd_rows_case(count, dtype, searches=S_):
    g = torch.Generator().manual_seed(700 + count)
    shape = (4, 64, 64) if count == 4 * 64 * 64 else (1, 1, count)
    pivot = torch.randn((searches,) + shape, generator=g).to(dtype)
    u = torch.randn((searches * N_,) + shape, generator=g).to(dtype)
    mode = torch.tensor(MODE[:searches * N_], dtype=torch.int32)
    rands = torch.rand(searches * N_, generator=g).tolist()
    lam, root = 0.15, float(np.sqrt(count))
    scale = torch.tensor([[r, lam, root] if m else [0.0, 0.0, 0.0] for r, m in zip(rands, mode.tolist())], dtype=torch.float32)
    want = []
    for r in range(searches * N_):
        if mode[r] == 0:
            want.append(u[r])
        else:
            to_add = u[r] / torch.norm(u[r])                                              # pipeline_stable_diffusion.py:1377
            want.append(pivot[r // N_] + to_add * rands[r] * lam * root)                  # :1379, left to right
    return pivot, u, mode, scale, torch.stack(want)


@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['float16', 'float32'])
def test_candidate_noise_sd_rows_rounds_like_the_reference_expression(ops, dtype, count):
    pivot, u, mode, scale, want = sd_rows_case(count, dtype)
    buf, out = guarded(tuple(u.shape), dtype)
    got = ops.candidate_noise_sd_rows(pivot.to(DEV), u.to(DEV), mode.to(DEV), scale.to(DEV), out=out)
    assert got.data_ptr() == out.data_ptr()
    assert_guards(buf, f'candidate_noise_sd_rows count={count}')
    got = got.cpu()
    fresh = mode == 0
    assert torch.equal(got[fresh], u[fresh])                                             # mode 0: a copy, bit for bit
    assert torch.equal(got[N_:2 * N_], u[N_:2 * N_])                                     # the all-fresh search
    if dtype == torch.float16:
        bad = got != want
        print(f'candidate_noise_sd_rows float16 count={count}: {int(bad.sum())} of {bad.numel()} values differ')
        assert not bool(bad.any()), (count, bad.reshape(S_ * N_, -1).sum(dim=1).tolist())
    else:
        err, bound = float((got - want).abs().max()), 2 ** -22 * float(want.abs().max())
        print(f'candidate_noise_sd_rows float32 count={count}: max err {err:.3e}, bound {bound:.3e}')
        assert err <= bound


@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32], ids=['float16', 'bfloat16', 'float32'])
def test_candidate_noise_sd_rows_one_search_equals_candidate_noise_sd(ops, dtype, count):
    pivot, u, mode, scale, _ = sd_rows_case(count, dtype, searches=1)
    want = ops.candidate_noise_sd(pivot.to(DEV), u.unsqueeze(1).contiguous().to(DEV), mode.to(DEV), scale.to(DEV))
    got = ops.candidate_noise_sd_rows(pivot.to(DEV), u.to(DEV), mode.to(DEV), scale.to(DEV))
    assert torch.equal(got.cpu().view(torch.int16 if dtype != torch.float32 else torch.int32),
                       want.cpu().reshape(got.shape).view(torch.int16 if dtype != torch.float32 else torch.int32))


def test_candidate_noise_sd_rows_each_search_equals_its_own_call(ops):
    """S searches in one launch == S single-search launches, bit for bit: a row reads its own search's pivot and nothing else"""
    pivot, u, mode, scale, _ = sd_rows_case(255, torch.float16)
    got = ops.candidate_noise_sd_rows(pivot.to(DEV), u.to(DEV), mode.to(DEV), scale.to(DEV)).cpu()
    for s in range(S_):
        rows = slice(s * N_, (s + 1) * N_)
        one = ops.candidate_noise_sd(pivot[s:s + 1].to(DEV), u[rows].unsqueeze(1).contiguous().to(DEV), mode[rows].to(DEV), scale[rows].contiguous().to(DEV))
        assert torch.equal(got[rows].view(torch.int16), one.cpu().reshape(got[rows].shape).view(torch.int16)), s


def test_candidate_noise_sd_rows_refuses_bad_arguments(ops):
    from diffusion_tts_amd import _lib
    pivot, u, mode, scale, _ = (t.to(DEV) for t in sd_rows_case(255, torch.float16))
    out = torch.empty_like(u)
    with pytest.raises(RuntimeError, match='dts_candidate_noise_sd_rows: null pointer'):
        ops._call('dts_candidate_noise_sd_rows', pivot.data_ptr(), u.data_ptr(), None, scale.data_ptr(), out.data_ptr(), ops.dt_code(torch.float16), S_, N_, 255)
    for searches, per in ((0, 4), (3, 0), (-1, 4)):
        with pytest.raises(RuntimeError, match=f'dts_candidate_noise_sd_rows: searches={searches} per={per}'):
            ops._call('dts_candidate_noise_sd_rows', pivot.data_ptr(), u.data_ptr(), mode.data_ptr(), scale.data_ptr(), out.data_ptr(), ops.dt_code(torch.float16), searches, per, 255)
        assert f'searches={searches} per={per}'.encode() in _lib.load().dts_last_error()
    with pytest.raises(ValueError, match='candidate_noise_sd_rows'):
        ops.candidate_noise_sd_rows(pivot, u[:S_ * N_ - 1].contiguous(), mode, scale)                 # not a whole number of rows per search
    with pytest.raises(ValueError, match='candidate_noise_sd_rows'):
        ops.candidate_noise_sd_rows(pivot, u, mode[:2].contiguous(), scale)
    with pytest.raises(ValueError, match='candidate_noise_sd_rows: out'):
        ops.candidate_noise_sd_rows(pivot, u, mode, scale, out=torch.empty(3, device=DEV, dtype=torch.float16))


# ---- ddim_candidates_groups ----------------------------------------------------------------------------------------------------------------------
def ddim_group_cases(dtype):
    """(x, e [G, count], z [G, ncand, count] or None, alpha_t, alpha_prev, sigma_t, ncand, want_x0): G in {1, 3} x ncand in {1, 3} x
    count in {1, 255, 4*64*64} over the alpha pairs; eta = 0 with z NULL, eta = 1 with z; x0_out NULL in every third case"""
    k = 0
    for at, ap in R.ALPHAS:
        for groups in (1, 3):
            for ncand in (1, 3):
                for count in (1, 255, 4 * 64 * 64):
                    for eta in (0.0, 1.0):
                        k += 1
                        g = R.gen(4000 + k)
                        x, e = torch.randn(groups, count, generator=g).to(dtype), torch.randn(groups, count, generator=g).to(dtype)
                        z = None if eta == 0.0 else torch.randn(groups, ncand, count, generator=g).to(dtype)
                        yield x, e, z, at, ap, R.ddim_sigma(at, ap, eta), ncand, k % 3 != 0


def run_groups(ops, x, e, z, at, ap, st, ncand, want_x0):
    """the launch with both outputs in guard-banded NaN-filled buffers"""
    groups, count = x.shape
    pbuf, pout = guarded((groups, ncand, count), x.dtype)
    xbuf, xout = guarded((groups, count), x.dtype)
    gp, g0 = ops.ddim_candidates_groups(x.to(DEV), e.to(DEV), None if z is None else z.to(DEV), at, ap, st, ncand=ncand, want_x0=want_x0,
                                        out=pout, x0_out=xout if want_x0 else None)
    what = f'ddim_candidates_groups G={groups} ncand={ncand} count={count}'
    assert gp.data_ptr() == pout.data_ptr() and (g0 is None) == (not want_x0)
    assert_guards(pbuf, what)
    if want_x0:
        assert g0.data_ptr() == xout.data_ptr()
        assert_guards(xbuf, what + ' x0')
    else:
        torch.cuda.synchronize()
        assert bool(torch.isnan(xbuf).all()), what + ': x0_out NULL, yet something was written'
    return gp, g0


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize('dtype', R.STORAGE, ids=[str(d).split('.')[-1] for d in R.STORAGE])
def test_ddim_candidates_groups(ops, dtype):
    worst_p = worst_0 = 0.0
    cases = 0
    for x, e, z, at, ap, st, ncand, want_x0 in ddim_group_cases(dtype):
        groups, count = x.shape
        gp, g0 = run_groups(ops, x, e, z, at, ap, st, ncand, want_x0)
        case = f'a_t={at} a_prev={ap} sigma_t={st:.4f} G={groups} ncand={ncand} count={count} z={"NULL" if z is None else "given"}'
        for g_ in range(groups):
            # every group against the float64 reference of ITS (x, e, z) ... (z NULL: prev [1, count], which every one of the ncand equal candidates must meet)
            zg = None if z is None else z[g_]
            (prev, bprev), (x0, bx0) = R.ddim_ref(x[g_], e[g_], zg, at, ap, st)
            ratio, err = R.worst(gp[g_].cpu(), prev, R.rounded_bound(prev, bprev, dtype))
            assert ratio <= 1.0, f'{case} group {g_} prev: err/bound {ratio:.3f} (max err {err:.3e})'
            worst_p = max(worst_p, ratio)
            if want_x0:
                ratio, err = R.worst(g0[g_].cpu(), x0, R.rounded_bound(x0, bx0, dtype))
                assert ratio <= 1.0, f'{case} group {g_} x0: err/bound {ratio:.3f} (max err {err:.3e})'
                worst_0 = max(worst_0, ratio)
            # ... and bit for bit against its own single-pair launch
            zd = None if zg is None else zg.to(DEV)
            sp, s0 = ops.ddim_candidates(x[g_].to(DEV), e[g_].to(DEV), zd, at, ap, st, want_x0=want_x0)
            for c in range(ncand):
                assert torch.equal(bits(gp[g_, c]), bits(sp[c if zd is not None else 0])), f'{case} group {g_} candidate {c}: bits differ from ddim_candidates'
            if want_x0:
                assert torch.equal(bits(g0[g_]), bits(s0)), f'{case} group {g_}: x0 bits differ from ddim_candidates'
        cases += 1
    print(f'ddim_candidates_groups {dtype}: {cases} cases, worst err/bound prev {worst_p:.3f}, x0 {worst_0:.3f}')


def test_ddim_candidates_groups_second_trip_of_the_grid_stride_loop(ops):
    """G * count = 33 * 16384 = 540 672 elements > the 2048 x 256 = 524 288 threads of a launch: the last 16 384 elements (group 32) are the
    loop's second trip"""
    dtype, groups, ncand, count = torch.float16, 33, 2, 4 * 64 * 64
    assert groups * count > 2048 * 256
    g = R.gen(4999)
    x, e = torch.randn(groups, count, generator=g).to(dtype), torch.randn(groups, count, generator=g).to(dtype)
    z = torch.randn(groups, ncand, count, generator=g).to(dtype)
    at, ap = R.ALPHAS[1]
    st = R.ddim_sigma(at, ap, 1.0)
    gp, g0 = run_groups(ops, x, e, z, at, ap, st, ncand, True)
    for g_ in (0, 31, 32):
        (prev, bprev), (x0, bx0) = R.ddim_ref(x[g_], e[g_], z[g_], at, ap, st)
        assert R.worst(gp[g_].cpu(), prev, R.rounded_bound(prev, bprev, dtype))[0] <= 1.0, g_
        assert R.worst(g0[g_].cpu(), x0, R.rounded_bound(x0, bx0, dtype))[0] <= 1.0, g_
        sp, s0 = ops.ddim_candidates(x[g_].to(DEV), e[g_].to(DEV), z[g_].to(DEV), at, ap, st)
        assert torch.equal(bits(gp[g_]), bits(sp)) and torch.equal(bits(g0[g_]), bits(s0)), g_


def test_ddim_candidates_groups_refuses_bad_arguments(ops):
    x = torch.randn(2, 64, device=DEV)
    prev = torch.empty(2, 1, 64, device=DEV)

    def call(groups=2, ncand=1, count=64, at=0.3, ap=0.45, st=0.0, xp=x.data_ptr()):
        ops._call('dts_ddim_candidates_groups', xp, x.data_ptr(), None, prev.data_ptr(), None, ops.dt_code(torch.float32), at, ap, st, groups, ncand, count)
    call()
    with pytest.raises(RuntimeError, match='dts_ddim_candidates_groups: groups=0'):
        call(groups=0)
    with pytest.raises(RuntimeError, match='dts_ddim_candidates_groups: bad args'):
        call(ncand=0)
    with pytest.raises(RuntimeError, match='dts_ddim_candidates_groups: bad args'):
        call(xp=None)
    with pytest.raises(RuntimeError, match='dts_ddim_candidates_groups: alphas out of range'):
        call(at=1.5)
    with pytest.raises(RuntimeError, match='dts_ddim_candidates_groups: sigma_t too large'):
        call(st=0.9)
    with pytest.raises(ValueError, match='ddim_candidates_groups: z'):
        ops.ddim_candidates_groups(x, x, torch.randn(3, 1, 64, device=DEV), 0.3, 0.45, 0.1)
    with pytest.raises(ValueError, match='ddim_candidates_groups: out'):
        ops.ddim_candidates_groups(x, x, None, 0.3, 0.45, 0.0, out=torch.empty(2, 64, device=DEV))
