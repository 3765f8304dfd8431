"""Every kernel of csrc/resample.hip (resample_fir_kernel and space_to_depth2_kernel in all their instantiations, the element-by-element
NHWC path included), resample_kernel (dts_resample2x) and the two split-image kernels (dts_split3_f16, dts_split2_f16: x3_split, x3_off and
x2_split of csrc/dts_common.h) against tests/resample_reference.py, which shares no code with the library.  The table of launches, with
the reason for every absent cell, is resample_reference.CASES / ABSENT.

HOW A LAUNCH IS MADE.  Through ops._call with raw pointers.  The input sits at a 16-byte-aligned, non-zero offset inside a buffer whose
other bytes are 0xFF; the output is the middle of a buffer filled with 0xFF -- the all-ones pattern, a NaN in f32, f16 and bf16.  After
the launch (a) the output equals the reference bit for bit, (b) no element still holds the fill pattern, (c) both guard bands are untouched.

EXACT LEG (test_exact, test_grid_stride).  The lattice inputs of resample_reference make every product, every partial sum in any order and
the stored result exact, so equality is asked in every storage type; the split forms are compared with x3_image(reference), NOT with
ops.split3_f16.  Nearest-up and space-to-depth are copies: equality on any input.  The grid-stride cases give each loop a thread count that
passes the launch cap by less than one block (the second trip, taken by a few threads only), on non-square images.

SPLIT IMAGES (test_split3_sweep, test_split2_sweep).  Every finite float16 value, ten float32 neighbours of each (the rounding ties
among them) and the specials -- zeros, float32 subnormals, both sides of the flush threshold 2^-14, the saturation edge, infinities, NaN
-- against the bit models x3_image / x2_image on the uint16 bits.  Zero signs are pinned; where the model holds a NaN a NaN is required
(its payload is not pinned).  The library is compiled without any flush-denormals option (no -fgpu-flush-denormals-to-zero, no fast
math), so float32-subnormal inputs follow IEEE on the device too and the model is NOT narrowed for them.

ROUNDING LEG (test_rounding).  Gaussian inputs rounded to the storage type, one non-square shape per kernel and type, judged PER ELEMENT
against resample_reference.bound (derived there from the kernels' operation counts; nothing is fitted); the copies must still be equal.
Record of a run on an MI355X (worst err / bound per kernel; a record, NOT the source of the bound):
    resample_fir_kernel<T, false>   down: f32 0.213, bf16 0.976, f16 0.973    up: f32 0.273, bf16 0.995, f16 0.994
    resample_fir_kernel<float, true>  (split image)   down 0.258, up 0.331
    resample_kernel<T>  (2x2 mean)  f32 0.517, bf16 0.995, f16 0.990          nearest-up: a copy, equal in every type
    space_to_depth2_kernel (all twelve instantiations): a copy, equal
(the 16-bit rows sit near 1 because their bound is the output rounding, u |y|, which a correctly rounded result reaches by itself; the f32
and split rows show the accumulation term alone).  No difference from the IEEE models was found in the split images, the float32
subnormals included.  The whole file takes 3.4 s on an MI355X (542 cases).

REFUSALS (test_refusals).  Odd h or w going down, c that is no whole vector, split_out with a 16-bit type or c % 32 != 0, cpad < 4c (or no
multiple of the vector / of 32): each raises and launches nothing -- the output buffer keeps its fill pattern everywhere."""
import functools

import numpy as np
import pytest
import torch

import resample_reference as R
from resample_reference import CASES

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD = 4096 + 16          # bytes on either side of an output: the output itself is 16-byte aligned and no more
IN_OFF = 48                # bytes in front of an input


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


def _dev_in(bits):
    """a numpy array's bytes at offset IN_OFF of a device buffer otherwise full of 0xFF: (buffer, pointer)"""
    b = torch.from_numpy(np.require(bits, requirements=['C', 'W']).view(np.uint8).reshape(-1))
    buf = torch.full((IN_OFF + b.numel() + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    buf[IN_OFF:IN_OFF + b.numel()] = b.to(DEV)
    assert (buf.data_ptr() + IN_OFF) % 16 == 0
    return buf, buf.data_ptr() + IN_OFF


def _dev_out(nbytes):
    buf = torch.full((2 * GUARD + nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    assert (buf.data_ptr() + GUARD) % 16 == 0
    return buf, buf.data_ptr() + GUARD


def _collect(buf, nbytes, dtype):
    """after the launch: the output as `dtype` bit patterns; asserts the guard bands"""
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert bool((host[:GUARD] == 0xFF).all()), 'a store in front of the output'
    assert bool((host[GUARD + nbytes:] == 0xFF).all()), 'a store behind the output'
    return host[GUARD:GUARD + nbytes].copy().view(dtype)


def _out_shape(case):
    if case.kind == 's2d':
        return (case.n, case.h // 2, case.w // 2, case.cpad)
    up = case.kind.endswith('up')
    return (case.n, 2 * case.h, 2 * case.w, case.c) if up else (case.n, case.h // 2, case.w // 2, case.c)


def _call(ops, case, xptr, optr):
    dt, split = R.DT_CODE[case.mode], int(case.mode == 'split')
    if case.kind in ('fir_down', 'fir_up'):
        ops._call('dts_resample_fir', xptr, optr, dt, case.n, case.h, case.w, case.c, int(case.kind == 'fir_up'), split)
    elif case.kind in ('box_down', 'box_up'):
        ops._call('dts_resample2x', xptr, optr, dt, case.n, case.h, case.w, case.c, int(case.kind == 'box_up'))
    else:
        ops._call('dts_space_to_depth2', xptr, int(case.layout == 'nchw'), optr, dt, case.n, case.h, case.w, case.c, case.cpad, split)


def _run(ops, case, x):
    """the case on the float64 input x: the output's bit patterns [n, ho, wo, c (2c for the split image)]"""
    shape = _out_shape(case)
    split = case.mode == 'split'
    odt = np.uint32 if case.mode == 'f32' else np.uint16
    nbytes = int(np.prod(shape)) * 4
    if not split and case.mode != 'f32':
        nbytes //= 2
    xin, xptr = _dev_in(R.to_bits(x, 'f32' if case.layout == 'nchw' else case.mode))       # the NCHW source is the float32 image
    buf, optr = _dev_out(nbytes)
    _call(ops, case, xptr, optr)
    got = _collect(buf, nbytes, odt)
    del xin
    return got.reshape(*shape[:-1], shape[-1] * (2 if split else 1))


def _assert_equal(case, got, ref):
    fill = np.uint32(0xFFFFFFFF) if got.dtype == np.uint32 else np.uint16(0xFFFF)
    assert not bool((got == fill).any()), f'{int((got == fill).sum())} output elements were never written'
    want = R.x3_image(ref.astype(np.float32)) if case.mode == 'split' else R.to_bits(ref, case.mode)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f'{int((got != want).sum())} of {want.size} elements differ'


@functools.lru_cache(maxsize=None)
def _exact(name, variant):
    case = CASES[name]
    x = R.case_input(case, variant)
    return x, R.reference(case, x)


@pytest.mark.parametrize('name,variant', R.launches(), ids=lambda v: str(v))
def test_exact(ops, name, variant):
    case = CASES[name]
    x, ref = _exact(name, variant)
    _assert_equal(case, _run(ops, case, x), ref)


def _split_call(ops, fn, c1, c2, m):
    """dts_split3_f16 of the concat (m[:, :c1], m[:, c1:]) / dts_split2_f16 of m (float32 [rows, C]): the image's uint16 bits [rows, 2C]"""
    rows, C = m.shape
    nbytes = rows * 2 * C * 2
    buf, optr = _dev_out(nbytes)
    if fn == 'dts_split3_f16':
        b1, p1 = _dev_in(m[:, :c1])
        b2, p2 = _dev_in(m[:, c1:]) if c2 else (None, None)
        ops._call(fn, p1, c1, p2, c2, optr, rows)
    else:
        b1, p1 = _dev_in(m)
        ops._call(fn, p1, C, optr, rows)
    return _collect(buf, nbytes, np.uint16).reshape(rows, 2 * C)


def _assert_image(got, want, x):
    """bit equality of two float16 images, except that where the model holds a NaN any NaN will do; the message classifies what differs"""
    g16, w16 = got.view(np.float16), want.view(np.float16)
    both_nan = np.isnan(g16) & np.isnan(w16)
    diff = (got != want) & ~both_nan
    if diff.any():
        idx = np.argwhere(diff)[:5]
        pytest.fail(f'{int(diff.sum())} of {want.size} halves differ; first (row, slot, got, want): '
                    f'{[(int(r), int(s), hex(int(got[r, s])), hex(int(want[r, s]))) for r, s in idx]}; input rows {[x[int(r)].tolist() for r, _ in idx[:2]]}')


@functools.lru_cache(maxsize=None)
def _sweep_model(fn, c1, c2):
    s = R.split_sweep()
    if fn == 'dts_split2_f16':
        m = (s / np.float32(64.0)).reshape(-1, c1)
        return m, R.x2_image(m)
    m = s.reshape(-1, c1 + c2)
    return m, R.x3_image(np.ascontiguousarray(m[:, :c1]), np.ascontiguousarray(m[:, c1:]) if c2 else None)


@pytest.mark.parametrize('c1,c2', [(c1, c2) for fn, c1, c2 in R.SPLIT_CASES if fn == 'dts_split3_f16'])
def test_split3_sweep(ops, c1, c2):
    """dts_split3_f16 over the whole sweep against x3_image: one source; a concat boundary inside a group of 32; two groups"""
    m, want = _sweep_model('dts_split3_f16', c1, c2)
    _assert_image(_split_call(ops, 'dts_split3_f16', c1, c2, m), want, m)


@pytest.mark.parametrize('c', [c1 for fn, c1, c2 in R.SPLIT_CASES if fn == 'dts_split2_f16'])
def test_split2_sweep(ops, c):
    """dts_split2_f16 over the sweep / 64 against x2_image"""
    m, want = _sweep_model('dts_split2_f16', c, 0)
    _assert_image(_split_call(ops, 'dts_split2_f16', c, 0, m), want, m)


@pytest.mark.parametrize('which', [g[0] for g in R.GRID_STRIDE])
def test_grid_stride(ops, which):
    """the second trip of every grid-stride loop: a thread count that passes the launch cap by less than one block"""
    _, cap, c = next(g for g in R.GRID_STRIDE if g[0] == which)
    if isinstance(c, R.Case):
        assert 0 < R.threads(c) - cap < 256
        x = R.case_input(c, 'lat')
        _assert_equal(c, _run(ops, c, x), R.reference(c, x))
        return
    fn, c1, c2, rows = c
    C = c1 + c2
    assert 0 < rows * (C // 8) - cap < 256
    rng = np.random.default_rng(rows)
    m = (rng.standard_normal((rows, C)) * np.exp2(rng.integers(-20, 12, size=(rows, C)))).astype(np.float32)
    if fn == 'dts_split2_f16':
        want = R.x2_image(m)
    else:
        want = R.x3_image(np.ascontiguousarray(m[:, :c1]), np.ascontiguousarray(m[:, c1:]))
    _assert_image(_split_call(ops, fn, c1, c2, m), want, m)


@pytest.mark.parametrize('case', R.ROUNDING, ids=lambda c: c.name)
def test_rounding(ops, case):
    x = R.gaussian(R.in_shape(case), 1 + R.hash_name(case.name), case.mode)
    y, s = R.reference(case, x, want_s=True)
    got = _run(ops, case, x)
    if not R.ROUNDINGS[case.kind]:               # a copy: equality
        _assert_equal(case, got, y)
        print(f'rounding {case.name}: {case.kernel}: a copy, equal')
        return
    val = R.x3_decode(got) if case.mode == 'split' else R.from_bits(got, case.mode)
    assert not bool(np.isnan(val).any()), 'an output element was never written'
    err, bnd = np.abs(val - y), R.bound(case.kind, case.mode, y, s)
    ratio = float((err / bnd).max())
    print(f'rounding {case.name}: {case.kernel}: max err/bound = {ratio:.3f}')
    assert bool((err <= bnd).all()), ratio


REFUSED = [  # (what, function, arguments after the two pointers are put in place)
    ('fir down, odd h', 'fir', dict(mode='f32', h=3, w=4, c=4, up=0, split=0)),
    ('fir down, odd w', 'fir', dict(mode='f16', h=4, w=3, c=8, up=0, split=0)),
    ('fir, f32 c % 4', 'fir', dict(mode='f32', h=4, w=4, c=6, up=1, split=0)),
    ('fir, bf16 c % 8', 'fir', dict(mode='bf16', h=4, w=4, c=12, up=0, split=0)),
    ('fir, split from bf16', 'fir', dict(mode='bf16', h=4, w=4, c=32, up=0, split=1)),
    ('fir, split from f16', 'fir', dict(mode='f16', h=4, w=4, c=32, up=1, split=1)),
    ('fir, split c % 32', 'fir', dict(mode='f32', h=4, w=4, c=40, up=1, split=1)),
    ('2x down, odd h', 'box', dict(mode='f32', h=3, w=4, c=4, up=0)),
    ('2x down, odd w', 'box', dict(mode='bf16', h=4, w=5, c=8, up=0)),
    ('2x, f16 c % 8', 'box', dict(mode='f16', h=4, w=4, c=12, up=1)),
    ('s2d, odd h', 's2d', dict(mode='f32', h=3, w=4, c=4, cpad=16, split=0, nchw=0)),
    ('s2d, odd w', 's2d', dict(mode='f32', h=4, w=3, c=3, cpad=12, split=0, nchw=1)),
    ('s2d, cpad < 4c', 's2d', dict(mode='f32', h=4, w=4, c=8, cpad=28, split=0, nchw=0)),
    ('s2d, cpad < 4c (bf16)', 's2d', dict(mode='bf16', h=4, w=4, c=8, cpad=24, split=0, nchw=0)),
    ('s2d, cpad % 8 (f16)', 's2d', dict(mode='f16', h=4, w=4, c=4, cpad=20, split=0, nchw=0)),
    ('s2d, split from f16', 's2d', dict(mode='f16', h=4, w=4, c=8, cpad=32, split=1, nchw=0)),
    ('s2d, split cpad % 32', 's2d', dict(mode='f32', h=4, w=4, c=8, cpad=40, split=1, nchw=0)),
    ('s2d, split cpad < 4c', 's2d', dict(mode='f32', h=4, w=4, c=12, cpad=32, split=1, nchw=0)),
]


@pytest.mark.parametrize('what,fn,a', REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals(ops, what, fn, a):
    """each raises, and the output buffer -- sized for the launch had it been made -- keeps its fill pattern everywhere: nothing ran"""
    n = 2
    xin, xptr = _dev_in(np.zeros(n * a['h'] * a['w'] * a['c'], np.float32))
    nbytes = n * (2 * a['h']) * (2 * a['w']) * max(a['c'], a.get('cpad', 0)) * 8
    buf, optr = _dev_out(nbytes)
    dt = R.DT_CODE[a['mode']]
    with pytest.raises(RuntimeError, match='libdts_hip'):
        if fn == 'fir':
            ops._call('dts_resample_fir', xptr, optr, dt, n, a['h'], a['w'], a['c'], a['up'], a['split'])
        elif fn == 'box':
            ops._call('dts_resample2x', xptr, optr, dt, n, a['h'], a['w'], a['c'], a['up'])
        else:
            ops._call('dts_space_to_depth2', xptr, a['nchw'], optr, dt, n, a['h'], a['w'], a['c'], a['cpad'], a['split'])
    torch.cuda.synchronize()
    assert bool((buf.cpu().numpy() == 0xFF).all()), what
