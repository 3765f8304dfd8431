"""Pins tests/resample_reference.py on the CPU.  The float64 operations against torch's float64 convolutions in the reference project's
formulation (Conv2d.forward, networks.py:64-90: conv2d / conv_transpose2d with the [1,3,3,1] filter, the one place F.conv2d is allowed near
them) and against oracle.edm_nets; the exactness of every launch of the table on its lattice input (two float32 models with different
summation orders equal the float64 result, which survives the storage type); the bit models of the split images against the format's
definition and the comment in csrc/dts_common.h; and the teeth of the net -- each indexing / rounding mistake a kernel could make, made
on the REFERENCE's own steps, changes the result of every case it applies to (which cases those are is asserted, not skipped)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_reference as R
from resample_reference import CASES, INSTANCES, MODES

KINDS = ('fir_down', 'fir_up', 'box_down', 'box_up', 's2d')


def _nchw(x):
    return torch.from_numpy(np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2))))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _rand(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape)


# ---- the references -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 2, 2, 3), (1, 2, 6, 4), (3, 6, 2, 5), (2, 4, 10, 3), (2, 8, 12, 2)])
def test_fir_down_is_the_reference_projects_conv2d(shape):
    from diffusion_tts_amd import init
    x = _rand(shape, 1)
    c = shape[-1]
    f2 = init.resample_filter_2d([1, 3, 3, 1]).double().tile([c, 1, 1, 1])
    want = _nhwc(F.conv2d(_nchw(x), f2, stride=2, padding=1, groups=c))
    got, s = R.fir_down(x, want_s=True)
    assert got.shape == want.shape and float(np.abs(got - want).max()) <= 1e-13
    assert bool((s >= np.abs(got) - 1e-15).all())


@pytest.mark.parametrize('shape', [(2, 1, 1, 3), (1, 1, 3, 4), (3, 3, 1, 5), (2, 3, 5, 3), (2, 4, 2, 2), (1, 7, 6, 2)])
def test_fir_up_is_the_reference_projects_conv_transpose2d(shape):
    from diffusion_tts_amd import init
    x = _rand(shape, 2)
    c = shape[-1]
    f2 = init.resample_filter_2d([1, 3, 3, 1]).double().tile([c, 1, 1, 1])
    want = _nhwc(F.conv_transpose2d(_nchw(x), 4 * f2, stride=2, padding=1, groups=c))
    got, s = R.fir_up(x, want_s=True)
    assert got.shape == want.shape and float(np.abs(got - want).max()) <= 1e-13
    assert bool((s >= np.abs(got) - 1e-15).all())


@pytest.mark.parametrize('shape', [(2, 2, 2, 3), (1, 2, 6, 4), (3, 6, 2, 5), (2, 4, 10, 3)])
def test_mean2x2_and_nearest_are_the_oracles(shape):
    from oracle import edm_nets
    x = _rand(shape, 3)
    assert float(np.abs(R.mean2x2_down(x) - _nhwc(edm_nets.resample_down(_nchw(x)))).max()) <= 1e-13
    up = R.nearest_up(x)
    assert np.array_equal(up, _nhwc(edm_nets.resample_up(_nchw(x))))
    assert np.array_equal(up, _nhwc(F.interpolate(_nchw(x), scale_factor=2, mode='nearest')))
    y = _rand((2, 3, 5, 3), 4)                                  # odd sizes go up too
    assert np.array_equal(R.nearest_up(y), _nhwc(edm_nets.resample_up(_nchw(y))))


@pytest.mark.parametrize('c,cpad', [(3, 12), (3, 32), (5, 64), (8, 32), (12, 96)])
def test_space_to_depth2_is_the_view_permute_expression(c, cpad):
    n, h, w = 2, 12, 8
    x = torch.from_numpy(_rand((n, c, h, w), 5))
    want = torch.zeros(n, cpad, h // 2, w // 2, dtype=torch.float64)
    want[:, :4 * c] = x.view(n, c, h // 2, 2, w // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(n, 4 * c, h // 2, w // 2)
    want = _nhwc(want)
    assert np.array_equal(R.space_to_depth2(x.numpy(), cpad, nchw=True), want)
    assert np.array_equal(R.space_to_depth2(_nhwc(x), cpad), want)


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def test_every_instantiation_has_a_case_and_every_absent_cell_a_reason():
    named = {c.kernel for c in CASES.values()}
    assert named == set(INSTANCES), set(INSTANCES) ^ named
    elem = [k for k in INSTANCES if k.startswith('space_to_depth2_kernel') and k.endswith('false, false>')]
    assert len(elem) == 4 and all(any(c.kernel == k and c.layout == 'elem' for c in CASES.values()) for k in elem)
    for k in INSTANCES:
        ns = {c.n for c in CASES.values() if c.kernel == k}
        hw = {(c.h, c.w) for c in CASES.values() if c.kernel == k}
        assert ns == {1, 3}, (k, ns)
        assert any(h != w for h, w in hw) and any(h > w for h, w in hw) and any(h < w for h, w in hw)
    for c in CASES.values():
        assert c.mode in MODES and c.kind in KINDS
        if c.kind != 's2d':
            assert c.c % R.EPV[c.mode] == 0
        else:
            assert c.cpad >= 4 * c.c and c.cpad % (32 if c.mode == 'split' else R.EPV[c.mode]) == 0
            assert (c.layout == 'vec') == (c.c % R.EPV[c.mode] == 0 and c.layout != 'nchw')
        if c.mode == 'split' and c.kind != 's2d':
            assert c.c % 32 == 0
        assert R.threads(c) * 16 * (2 if c.mode == 'split' else 1) < 2 ** 20            # well under a megabyte of output
    assert any(c.kind == 's2d' and c.cpad > R._round_up(4 * c.c, R.GRANULE[c.mode]) for c in CASES.values())
    assert all(isinstance(v, str) and len(v) > 20 for v in R.ABSENT.values())
    assert {k.kernel for k in R.ROUNDING} == set(INSTANCES)


def test_grid_stride_cases_pass_the_cap_by_less_than_a_block():
    for name, cap, c in R.GRID_STRIDE:
        t = R.threads(c) if isinstance(c, R.Case) else c[3] * ((c[1] + c[2]) // 8)
        assert 0 < t - cap < 256, (name, t - cap)
        if isinstance(c, R.Case):
            assert c.h != c.w


# ---- exactness on the lattices ------------------------------------------------------------------------------------------------------
def _f32_model(case, x, order):
    """the case in float32 arithmetic.  order 'kernel': the kernels' own order (per source row a row sum over the columns, then the rows);
    'other': the 2-D weights applied directly, taps in the reverse order"""
    f = np.float32
    x = x.astype(f)
    n, h, w, c = x.shape
    if case.kind in ('fir_down', 'fir_up'):
        if case.kind == 'fir_down':
            i, j = np.arange(h // 2), np.arange(w // 2)
            ys = [(2 * i - 1 + a, f(0.375 if a in (1, 2) else 0.125)) for a in range(4)]
            xs = [(2 * j - 1 + b, f(0.375 if b in (1, 2) else 0.125)) for b in range(4)]
        else:
            yo, xo = np.arange(2 * h), np.arange(2 * w)
            ys = [(yo >> 1, f(0.75)), (np.where(yo & 1, (yo >> 1) + 1, (yo >> 1) - 1), f(0.25))]
            xs = [(xo >> 1, f(0.75)), (np.where(xo & 1, (xo >> 1) + 1, (xo >> 1) - 1), f(0.25))]
        r = np.zeros((n, len(ys[0][0]), len(xs[0][0]), c), f)
        if order == 'kernel':
            for yy, ka in ys:
                row = np.zeros_like(r)
                for xx, kb in xs:
                    row = row + kb * R._gather(x, yy, xx, h, w)[0]
                r = r + ka * row
        else:
            for xx, kb in reversed(xs):
                for yy, ka in reversed(ys):
                    r = r + (ka * kb) * R._gather(x, yy, xx, h, w)[0]
        assert r.dtype == f
        return r
    assert case.kind == 'box_down'
    i, j = np.arange(h // 2), np.arange(w // 2)
    taps = [(dy, dx) for dy in range(2) for dx in range(2)]
    r = np.zeros((n, h // 2, w // 2, c), f)
    for dy, dx in (taps if order == 'kernel' else reversed(taps)):
        r = r + f(0.25) * R._gather(x, 2 * i + dy, 2 * j + dx, h, w)[0]
    assert r.dtype == f
    return r


@pytest.mark.parametrize('kernel', INSTANCES)
def test_lattice_inputs_make_every_launch_exact(kernel):
    """for every case of the table: the input is representable in the storage type, two float32 models with different summation orders
    equal the float64 reference, and the result survives the storage type (for the split form: hi + lo / 2048 gives it back)"""
    count = 0
    for name, variant in R.launches():
        case = CASES[name]
        if case.kernel != kernel:
            continue
        count += 1
        x = R.case_input(case, variant)
        assert np.array_equal(R.from_bits(R.to_bits(x, case.mode), case.mode), x)
        ref = R.reference(case, x)
        assert float(np.abs(ref).max()) <= 257.0 and np.array_equal(ref * 4096.0, np.rint(ref * 4096.0))
        if variant == 'lat':
            assert np.array_equal(ref, np.rint(ref))
        if R.ROUNDINGS[case.kind]:
            for order in ('kernel', 'other'):
                assert np.array_equal(_f32_model(case, x, order).astype(np.float64), ref), (name, order)
        if case.mode == 'split':
            img = R.x3_image(ref.astype(np.float32))
            assert np.array_equal(R.x3_decode(img), ref)
            if variant == 'lo':
                lo = img.reshape(-1, 2, 32)[:, 1, :]
                assert bool((lo & 0x7FFF).any()), 'the lo variant must reach the lo half'
        else:
            assert np.array_equal(R.from_bits(R.to_bits(ref, case.mode), case.mode), ref)
    assert count > 0


def test_the_rounding_bound_holds_for_a_float32_model():
    """the derived bound against the float32 models above on Gaussian inputs (both orders) -- a check of the derivation's arithmetic on the
    CPU, not its source"""
    for case in R.ROUNDING:
        if not R.ROUNDINGS[case.kind]:
            continue
        x = R.gaussian(R.in_shape(case), 11, case.mode)
        y, s = R.reference(case, x, want_s=True)
        for order in ('kernel', 'other'):
            r = _f32_model(case, x, order)
            if case.mode == 'split':
                got = R.x3_decode(R.x3_image(r))
            else:
                got = R.from_bits(R.to_bits(r.astype(np.float64), case.mode), case.mode)
            assert bool((np.abs(got - y) <= R.bound(case.kind, case.mode, y, s)).all()), (case.name, order)


# ---- the split models ---------------------------------------------------------------------------------------------------------------
def test_numpy_float16_cast_is_round_to_nearest_even_on_the_whole_sweep():
    s = R.split_sweep()
    assert 6.9e5 < s.size < 7.1e5 and s.size % 192 == 0
    fin = ~np.isnan(s)
    with np.errstate(over='ignore'):
        cast = s.astype(np.float16).astype(np.float32)
    assert np.array_equal(R.round_to_f16_grid(s)[fin].view(np.uint32), cast[fin].view(np.uint32))
    # and the grid function itself on values worked by hand: ties to even, the subnormal step 2^-24, the overflow threshold 65520
    hand = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, 65519.996, 65520.0, -2.0 ** -26], np.float32)
    want = np.array([1.0, 1.0 + 2.0 ** -9, 0.0, 2.0 ** -23, 65504.0, np.inf, -0.0], np.float32)
    assert np.array_equal(R.round_to_f16_grid(hand).view(np.uint32), want.view(np.uint32))


def test_x3_model_reproduces_x_and_saturates_flushes_and_keeps_nan():
    """Bound: x - h is exact in float32 and at most half a float16 step, 2^-11 |x| for |x| >= 2^-14; its image (x - h) * 2048 is rounded to
    float16 with relative error 2^-11 when it is a normal float16 number and absolute error 2^-25 (half a subnormal step) otherwise:
    |hi + lo / 2048 - x| <= max(2^-22 |x|, 2^-36) = 2^-22 |x| on 2^-14 <= |x| <= 65504."""
    s = R.split_sweep()
    hi, lo = R.x3_parts(s)
    dec = hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64) / 2048.0
    a = np.abs(s.astype(np.float64))
    rng = (a >= 2.0 ** -14) & (a <= 65504.0)
    assert int(rng.sum()) > 6e5
    assert bool((np.abs(dec - s)[rng] <= 2.0 ** -22 * a[rng]).all())
    assert bool((np.abs(hi.view(np.float16).astype(np.float64))[rng] >= 2.0 ** -14).all())       # hi is never a subnormal
    big = a > 65504.0                                            # saturation: +-65504 | +0, the infinities included
    assert int(big.sum()) >= 10
    assert np.array_equal(hi[big], np.where(s[big] > 0, 0x7BFF, 0xFBFF).astype(np.uint16)) and not lo[big].any()
    nan = np.isnan(s)
    assert int(nan.sum()) == 1
    for part in (hi, lo):
        assert bool(np.isnan(part[nan].view(np.float16)).all()) and not np.isnan(part[~nan].view(np.float16)).any()
    with np.errstate(over='ignore'):
        small = np.abs(s.astype(np.float16).astype(np.float64)) < 2.0 ** -14          # what rounds to a float16 subnormal (or zero)
    small &= ~nan
    assert int(small.sum()) > 2000 * 11
    assert not hi[small].any(), 'a flushed hi half is +0'
    assert np.array_equal(lo[small], R._f16_bits(s[small] * np.float32(2048.0)))
    assert bool((np.abs(dec - s)[small] <= 2.0 ** -11 * a[small] + 2.0 ** -36).all())
    # zero signs as IEEE gives them: -0 -> hi +0 (flushed), lo = (-0 - +0) * 2048 = -0
    z = R.x3_parts(np.array([0.0, -0.0], np.float32))
    assert z[0].tolist() == [0, 0] and z[1].tolist() == [0, 0x8000]


def test_x3_layout_is_hi32_lo32_per_group_of_the_concat():
    x1 = np.arange(2 * 40, dtype=np.float32).reshape(2, 40) + 1.0
    x2 = -(np.arange(2 * 24, dtype=np.float32).reshape(2, 24) + 1.0)
    img = R.x3_image(x1, x2)
    assert img.shape == (2, 128) and img.dtype == np.uint16
    cat = np.concatenate([x1, x2], -1)
    for row in range(2):
        for ch in range(64):
            off = ((ch >> 5) << 6) + (ch & 31)
            assert img[row, off] == np.float16(cat[row, ch]).view(np.uint16) and img[row, off + 32] == 0
    assert np.array_equal(R.x3_decode(img), cat.astype(np.float64))


def test_x2_model_reproduces_x_and_saturates():
    """y = 64 x is exact; y - hi is exact in float32 and its float16 rounding costs 2^-11 of it (<= 2^-22 |y|) or half a subnormal step
    (2^-25): |hi + lo - y| <= max(2^-22 |y|, 2^-25)."""
    s = R.split_sweep() / np.float32(64.0)
    img = R.x2_image(s.reshape(-1, 8)).reshape(-1, 2, 8)
    hi, lo = img[:, 0, :].reshape(-1), img[:, 1, :].reshape(-1)
    y = s.astype(np.float64) * 64.0
    a = np.abs(y)
    rng = (a >= 2.0 ** -14) & (a <= 65504.0)
    dec = hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64)
    assert bool((np.abs(dec - y)[rng] <= np.maximum(2.0 ** -22 * a[rng], 2.0 ** -25)).all())
    assert np.array_equal(hi[rng], y[rng].astype(np.float16).view(np.uint16))             # hi is the float16 rounding of 64 x, never flushed
    big = a > 65504.0
    assert int(big.sum()) >= 10
    assert np.array_equal(hi[big], np.where(y[big] > 0, 0x7BFF, 0xFBFF).astype(np.uint16)) and not lo[big].any()
    nan = np.isnan(y)
    assert bool(np.isnan(hi[nan].view(np.float16)).all()) and bool(np.isnan(lo[nan].view(np.float16)).all())
    # hi(C) | lo(C) per row; an exactly representable y has lo = y - y = +0, and -0 gives hi -0
    r = R.x2_image(np.array([[1.0, -0.0, 2.0 ** -6 + 2.0 ** -18, 0.5, 3.0, 4.0, 5.0, 6.0]], np.float32))
    assert r.shape == (1, 16) and r[0, 0] == np.float16(64.0).view(np.uint16) and r[0, 1] == 0x8000 and r[0, 8] == 0 and r[0, 9] == 0
    assert r[0, 2] == np.float16(1.0).view(np.uint16) and r[0, 10] == np.float16(2.0 ** -12).view(np.uint16)


# ---- the teeth ----------------------------------------------------------------------------------------------------------------------
def _applies(mistake, c):
    """the cases whose result a mistake must change"""
    if mistake == 'swap_hw':
        return c.h != c.w
    if mistake == 'parity':                      # (at 1 x 1 both neighbours of the only pixel are outside the image whichever parity is used)
        return c.kind == 'fir_up' and (c.h > 1 or c.w > 1)
    if mistake in ('renorm', 'swap38'):
        return c.kind in ('fir_down', 'fir_up')
    if mistake == 'ryrx':
        return c.kind == 's2d'
    assert mistake == 'pad'
    return c.kind == 's2d' and c.cpad > 4 * c.c


@pytest.mark.parametrize('mistake', R.MISTAKES)
def test_each_mistake_changes_every_case_it_applies_to(mistake):
    """made on the reference's own steps, on the lattice input the GPU file uses; where it does not apply the result is unchanged"""
    hit = 0
    for name, variant in R.launches():
        case = CASES[name]
        x = R.case_input(case, variant)
        good, bad = R.reference(case, x), R.reference(case, x, mistake)
        assert good.shape == bad.shape
        changed = not np.array_equal(good, bad)
        assert changed == _applies(mistake, case), (mistake, name, variant)
        hit += changed
    kinds = {c.kind for c in CASES.values() if _applies(mistake, c)}
    print(f'{mistake}: changes {hit} of {len(R.launches())} launches ({sorted(kinds)})')
    want = {'swap_hw': set(KINDS), 'parity': {'fir_up'}, 'renorm': {'fir_down', 'fir_up'}, 'swap38': {'fir_down', 'fir_up'},
            'ryrx': {'s2d'}, 'pad': {'s2d'}}[mistake]
    assert kinds == want


@pytest.mark.parametrize('mistake', R.SPLIT_MISTAKES)
def test_each_split_mistake_changes_the_image_of_the_sweep(mistake):
    s = R.split_sweep()
    for fn, c1, c2 in R.SPLIT_CASES:
        if fn != 'dts_split3_f16':
            continue
        m = s.reshape(-1, c1 + c2)
        x1, x2 = np.ascontiguousarray(m[:, :c1]), (np.ascontiguousarray(m[:, c1:]) if c2 else None)
        good, bad = R.x3_image(x1, x2), R.x3_image(x1, x2, mistake)
        nan = np.isnan(good.view(np.float16)) & np.isnan(bad.view(np.float16))
        diff = (good != bad) & ~nan
        print(f'{mistake} c1={c1} c2={c2}: {int(diff.sum())} of {good.size} halves differ')
        assert bool(diff.any()), (mistake, c1, c2)
        assert np.array_equal(good, R.x3_image(m))              # the concat boundary changes nothing
