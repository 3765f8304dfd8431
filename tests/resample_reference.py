"""The resampling and rearrangement passes (dts_resample_fir, dts_resample2x, dts_space_to_depth2) in float64, written from their
definitions with explicit index arithmetic, bit models of the two split-precision operand images (x3_split / x3_off and x2_split of
csrc/dts_common.h: dts_split3_f16, dts_split2_f16 and every kernel that writes such an image), the inputs that make those launches
EXACT, and the table of launches the GPU file runs (tests/test_gpu_resample.py).  numpy / torch on the CPU only: nothing here calls
F.conv2d or anything of diffusion_tts_amd (tests/test_resample_reference.py pins this file against torch's convolutions and shows that
its inputs hide no indexing fault).  Activations are NHWC [n, h, w, c] numpy arrays throughout.

Why exact.  Every weight is a binary fraction ({1, 3, 9} / 64 down, {1, 3, 9} / 16 up, 1 / 4 for the 2x2 mean), so on the lattices of
`lattice()` -- 64 m with |m| <= 4 (down), 16 m with |m| <= 16 (up), 4 m with |m| <= 64 (mean), m an independent random integer per element
-- every product, every partial sum in any order and the result are integers of magnitude <= 256: exact in the f32 accumulators and in
bf16 / f16 / f32 storage.  The `lo` variant (f32 and split forms) adds b * 2^-6, b in {0, +-1}: everything is then a multiple of 2^-12
below 2^9 (21 bits), still exact in float32, and the split image of the result has a non-zero lo half.  A kernel must then return the
float64 result BIT FOR BIT; any border, parity, h/w, phase-order or padding mistake is a non-zero difference.

THE ROUNDING BOUND (`bound`; written from the kernels' operation counts before the first run, nothing in it is fitted).  With inputs
already rounded to the storage type the kernels hold the operands exactly.  A term w_a w_b x of the FIR passes goes through one
multiplication by the column weight, the additions of the row sum, one multiplication by the row weight and the additions of the output
sum: two multiplications and at most eight additions of which the first of each sum adds to zero and is exact -- eight roundings of
relative size e32 = 2^-24 at most (a fused multiply-add only removes some).  To first order the computed float32 value is within
8 e32 sum |w_a w_b x| of the exact one ((1 + e)^8 - 1 < 8.000004 e).  The 2x2 mean multiplies by 1/4 exactly and adds four terms:
3 e32 sum |x / 4|.  Nearest-up and space-to-depth copy: no error at all.  The store then rounds to the output type: u |y| with
u = 2^-8 (bf16), 2^-11 (f16, and half a subnormal step, 2^-25, below 2^-14), nothing for f32 (the accumulator IS the output).  The split
image holds the f32 value r as hi + lo / 2048 with hi = f16(r) and lo = f16((r - hi) * 2048): r - hi is exact in float32, at most 2^-11 |r|,
and its rounding to f16 costs 2^-11 of that -- 2^-22 |r| -- or half a subnormal step of lo, 2^-25 / 2048 = 2^-36; below 2^-14 the whole value
sits in lo (2^-11 |r| < 2^-25, which `bound` adds for the split form).  The factor 1.001 covers the second-order terms and the interplay of
the accumulation error with the last rounding, as in tests/test_gpu_conv.py."""
import collections

import numpy as np
import torch

MODES = ('f32', 'bf16', 'f16', 'split')
STORE = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16, 'split': torch.float32}      # what the kernel READS
EPV = {'f32': 4, 'bf16': 8, 'f16': 8, 'split': 8}                 # channels per thread: c (cpad) must be a multiple
GRANULE = {'f32': 32, 'bf16': 64, 'f16': 64, 'split': 32}         # input channels of one convolution K step: what ops.space_to_depth2 pads 4c to
DT_CODE = {'f32': 0, 'bf16': 1, 'f16': 2, 'split': 0}             # include/dts.h
E32 = 2.0 ** -24
TAPS = (1.0, 3.0, 3.0, 1.0)


# ---- the operations -----------------------------------------------------------------------------------------------------------------
def _gather(x, yy, xx, h, w):
    """x[:, yy, xx, :] for index vectors yy [H'], xx [W'] with zeros outside the h x w image: [n, H', W', c]"""
    n, c = x.shape[0], x.shape[-1]
    ok = ((yy >= 0) & (yy < h))[:, None] & ((xx >= 0) & (xx < w))[None, :]
    flat = np.clip(yy, 0, h - 1)[:, None] * w + np.clip(xx, 0, w - 1)[None, :]
    return x.reshape(n, h * w, c)[:, flat] * ok[None, :, :, None], ok


def _swapped(fn, x, **kw):
    """the `h and w exchanged` mistake: the same memory read as a [w, h] image, the result written as if it were the [h', w'] one"""
    n, h, w, c = x.shape
    o = fn(x.reshape(n, w, h, c), **kw)
    return o.reshape(n, o.shape[2], o.shape[1], o.shape[3])


def fir_down(x, mistake=None, want_s=False):
    """out[i][j] = sum_{a,b} k[a] k[b] / 64 * x[2i-1+a][2j-1+b], k = [1,3,3,1], zeros outside the image.  [n, h, w, c] -> [n, h/2, w/2, c]
    (float64).  want_s: also sum |w_ab x_ab|.  `mistake` (None in the reference): one of MISTAKES, made on this function's own steps."""
    if mistake == 'swap_hw':
        return _swapped(fir_down, x)
    x = np.asarray(x, np.float64)
    n, h, w, c = x.shape
    assert h % 2 == 0 and w % 2 == 0
    k = TAPS if mistake != 'swap38' else (3.0, 1.0, 1.0, 3.0)
    i, j = np.arange(h // 2), np.arange(w // 2)
    out, s, wsum = np.zeros((n, h // 2, w // 2, c)), np.zeros((n, h // 2, w // 2, c)), np.zeros((h // 2, w // 2))
    for a in range(4):
        for b in range(4):
            wgt = k[a] * k[b] / 64.0
            t, ok = _gather(x, 2 * i - 1 + a, 2 * j - 1 + b, h, w)
            out += wgt * t
            s += wgt * np.abs(t)
            wsum += wgt * ok
    if mistake == 'renorm':
        out = out / wsum[None, :, :, None]
    return (out, s) if want_s else out


def fir_up(x, mistake=None, want_s=False):
    """per axis out[2m] = 3/4 x[m] + 1/4 x[m-1], out[2m+1] = 3/4 x[m] + 1/4 x[m+1], zeros outside.  [n, h, w, c] -> [n, 2h, 2w, c]"""
    if mistake == 'swap_hw':
        return _swapped(fir_up, x)
    x = np.asarray(x, np.float64)
    n, h, w, c = x.shape
    near, far = (0.75, 0.25) if mistake != 'swap38' else (0.25, 0.75)
    yo, xo = np.arange(2 * h), np.arange(2 * w)
    step = -1 if mistake == 'parity' else 1

    def sources(o):             # (index, weight) of the two source rows / columns of output index o
        m, odd = o >> 1, o & 1
        return ((m, near), (np.where(odd == 1, m + step, m - step), far))

    out, s, wsum = np.zeros((n, 2 * h, 2 * w, c)), np.zeros((n, 2 * h, 2 * w, c)), np.zeros((2 * h, 2 * w))
    for yy, wa in sources(yo):
        for xx, wb in sources(xo):
            t, ok = _gather(x, yy, xx, h, w)
            out += wa * wb * t
            s += wa * wb * np.abs(t)
            wsum += wa * wb * ok
    if mistake == 'renorm':
        out = out / wsum[None, :, :, None]
    return (out, s) if want_s else out


def mean2x2_down(x, mistake=None, want_s=False):
    """dts_resample2x, mode 0: out[i][j] = (x[2i][2j] + x[2i][2j+1] + x[2i+1][2j] + x[2i+1][2j+1]) / 4"""
    if mistake == 'swap_hw':
        return _swapped(mean2x2_down, x)
    x = np.asarray(x, np.float64)
    n, h, w, c = x.shape
    assert h % 2 == 0 and w % 2 == 0
    i, j = np.arange(h // 2), np.arange(w // 2)
    out, s = np.zeros((n, h // 2, w // 2, c)), np.zeros((n, h // 2, w // 2, c))
    for dy in range(2):
        for dx in range(2):
            t, _ = _gather(x, 2 * i + dy, 2 * j + dx, h, w)
            out += 0.25 * t
            s += 0.25 * np.abs(t)
    return (out, s) if want_s else out


def nearest_up(x, mistake=None):
    """dts_resample2x, mode 1: out[i][j] = x[i >> 1][j >> 1]"""
    if mistake == 'swap_hw':
        return _swapped(nearest_up, x)
    x = np.asarray(x, np.float64)
    n, h, w, c = x.shape
    return _gather(x, np.arange(2 * h) >> 1, np.arange(2 * w) >> 1, h, w)[0]


def space_to_depth2(x, cpad, nchw=False, mistake=None):
    """out[n][i][j][(ry*2 + rx) * c + ci] = x[n][2i+ry][2j+rx][ci], channels 4c .. cpad-1 zero.  x is NHWC, or NCHW [n, c, h, w] with nchw;
    the result is NHWC [n, h/2, w/2, cpad] (float64)."""
    x = np.asarray(x, np.float64)
    if nchw:                                    # bring the element (n, ci, y, x) to where the NHWC formula looks for it
        n, c, h, w = x.shape
        v = np.zeros((n, h, w, c))
        for ci in range(c):
            v[:, :, :, ci] = x[:, ci]
        x = v
    if mistake == 'swap_hw':
        return _swapped(lambda t: space_to_depth2(t, cpad), x)
    n, h, w, c = x.shape
    assert h % 2 == 0 and w % 2 == 0 and cpad >= 4 * c
    out = np.full((n, h // 2, w // 2, cpad), 1.0 if mistake == 'pad' else 0.0)
    i, j = np.arange(h // 2), np.arange(w // 2)
    for ry in range(2):
        for rx in range(2):
            ph = rx * 2 + ry if mistake == 'ryrx' else ry * 2 + rx
            out[..., ph * c:(ph + 1) * c] = _gather(x, 2 * i + ry, 2 * j + rx, h, w)[0]
    return out


MISTAKES = ('swap_hw', 'parity', 'renorm', 'swap38', 'ryrx', 'pad')


# ---- bit models of the split images ---------------------------------------------------------------------------------------------------
F16_MAX = np.float32(65504.0)
F16_MIN_NORMAL = np.float32(2.0 ** -14)
SPLIT_MISTAKES = ('trunc', 'ties_away', 'no_flush', 'flush_le', 'lo_2p10', 'no_sat', 'sat_65520', 'lo_off64', 'group64')


def round_to_f16_grid(x, rule='even'):
    """float32 -> the nearest float16 VALUE (returned as float32), from the format's definition: the grid step at |x| in [2^e, 2^(e+1)) is
    2^(max(e, -14) - 10); what lands beyond 65504 is +-inf.  rule: 'even' (IEEE round to nearest even), 'away' (ties away from zero),
    'trunc' (towards zero).  The independent statement of what numpy's cast does (pinned in tests/test_resample_reference.py)."""
    x = np.asarray(x, np.float32)
    v = x.astype(np.float64)
    fin = np.isfinite(v)
    _, e = np.frexp(np.where(fin, v, 1.0))                   # |v| = m * 2^e, m in [0.5, 1): the binade's exponent is e - 1
    q = np.ldexp(1.0, np.maximum(e - 1, -14) - 10)
    r = np.where(fin, v, 0.0) / q                            # exact: a power-of-two scaling
    if rule == 'even':
        r = np.rint(r)
    elif rule == 'away':
        r = np.sign(r) * np.floor(np.abs(r) + 0.5)
    else:
        r = np.trunc(r)
    y = r * q
    y = np.where(np.abs(y) > 65504.0, np.copysign(np.inf, y), y)
    y = np.where(fin, y, v)
    return np.copysign(y, v).astype(np.float32)              # a result of zero keeps the operand's sign


def _f16_bits(v):
    with np.errstate(over='ignore', invalid='ignore'):
        return np.asarray(v, np.float32).astype(np.float16).view(np.uint16)


def x3_parts(x, mistake=None):
    """x3_split of csrc/dts_common.h on a float32 array: (hi, lo) as uint16 float16 bit patterns of x's shape.  |x| > 65504 is clamped to
    +-65504 (a NaN stays a NaN); h = f32(f16(x)), round to nearest even; h = +0 where |h| < 2^-14; hi = f16(h); lo = f16((x - h) * 2048),
    all in float32 (so zero signs are IEEE's)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        if mistake == 'no_sat':
            pass
        elif mistake == 'sat_65520':
            x = np.where(np.abs(x) >= np.float32(65520.0), np.copysign(F16_MAX, x), x)
        else:
            x = np.where(np.abs(x) > F16_MAX, np.copysign(F16_MAX, x), x)
        if mistake in ('trunc', 'ties_away'):
            h = round_to_f16_grid(x, 'trunc' if mistake == 'trunc' else 'away')
        else:
            h = x.astype(np.float16).astype(np.float32)
        if mistake == 'flush_le':
            h = np.where(np.abs(h) <= F16_MIN_NORMAL, np.float32(0.0), h)
        elif mistake != 'no_flush':
            h = np.where(np.abs(h) < F16_MIN_NORMAL, np.float32(0.0), h)
        lo = (x - h) * np.float32(1024.0 if mistake == 'lo_2p10' else 2048.0)
        assert h.dtype == np.float32 and lo.dtype == np.float32
        return _f16_bits(h), _f16_bits(lo)


def x3_image(x1, x2=None, mistake=None):
    """dts_split3_f16's image of the channel concat of x1 [..., c1] and x2 [..., c2] (float32; c1 + c2 a multiple of 32): uint16 [..., 2C];
    per pixel row and per group of 32 channels hi(32) | lo(32)  (x3_off: channel c's hi half at (c >> 5 << 6) + (c & 31), its lo half 32 on)"""
    x = np.asarray(x1, np.float32) if x2 is None else np.concatenate([np.asarray(x1, np.float32), np.asarray(x2, np.float32)], axis=-1)
    C = x.shape[-1]
    assert C % 32 == 0
    hi, lo = x3_parts(x, mistake if mistake not in ('lo_off64', 'group64') else None)
    rows = x.size // C
    img = np.zeros(rows * 2 * C, np.uint16)
    g = 64 if mistake == 'group64' else 32
    ch = np.arange(C)
    off = (ch // g) * (2 * g) + ch % g
    base = (np.arange(rows) * 2 * C)[:, None]
    lo_at = (base + off[None, :] + (64 if mistake == 'lo_off64' else g)).reshape(-1) % img.size      # (a mistaken offset wraps instead of leaving the array)
    img[(base + off[None, :]).reshape(-1) % img.size] = hi.reshape(-1)
    img[lo_at] = lo.reshape(-1)
    return img.reshape(*x.shape[:-1], 2 * C)


def x3_decode(img):
    """hi + lo / 2048 of an x3 image, float64 [..., C]"""
    img = np.asarray(img, np.uint16)
    C = img.shape[-1] // 2
    v = img.view(np.float16).astype(np.float64).reshape(*img.shape[:-1], C // 32, 2, 32)
    return (v[..., 0, :] + v[..., 1, :] / 2048.0).reshape(*img.shape[:-1], C)


def x2_image(x):
    """dts_split2_f16's image (x2_split): y = x * 64 in float32, clamped like x3_split; hi = f16(y), lo = f16(y - hi); the row is hi(C) | lo(C)"""
    x = np.asarray(x, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        y = x * np.float32(64.0)
        y = np.where(np.abs(y) > F16_MAX, np.copysign(F16_MAX, y), y)
        hi = y.astype(np.float16)
        lo = y - hi.astype(np.float32)
        assert y.dtype == np.float32 and lo.dtype == np.float32
        return np.concatenate([hi.view(np.uint16), _f16_bits(lo)], axis=-1)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
LATTICE = {'fir_down': (64.0, 4), 'fir_up': (16.0, 16), 'box_down': (4.0, 64), 'box_up': (1.0, 120), 's2d': (1.0, 120)}     # (step, max |m|)


def lattice(kind, shape, seed, lo=False):
    """step * m, m an independent random integer in [-max, max] per element [+ b * 2^-6, b in {0, +-1}: the `lo` variant]; float64.
    (nearest-up and space-to-depth copy: any value the storage type holds will do, the integers up to 120 fit bf16)"""
    step, mmax = LATTICE[kind]
    rng = np.random.default_rng(seed)
    x = step * rng.integers(-mmax, mmax + 1, size=shape).astype(np.float64)
    if lo:
        x = x + rng.integers(-1, 2, size=shape).astype(np.float64) * 2.0 ** -6
    return x


def gaussian(shape, seed, mode):
    """N(0, 1) rounded to the storage type of `mode`, as float64"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(STORE[mode]).double().numpy()


def to_bits(v, mode):
    """float64 array -> the bit patterns of its rounding (nearest even) to the storage type: uint32 (f32) or uint16"""
    t = torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(STORE[mode])
    if mode in ('f32', 'split'):
        return t.numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)


def from_bits(b, mode):
    """the inverse on what a kernel wrote: float64"""
    if mode in ('f32', 'split'):
        return np.asarray(b, np.uint32).view(np.float32).astype(np.float64)
    t = torch.from_numpy(np.asarray(b, np.uint16).view(np.int16).copy())
    return t.view(STORE[mode]).double().numpy()


_SPECIALS = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1.1754942e-38, 2.0 ** -25, -2.0 ** -25, 2.0 ** -24, -2.0 ** -24,
             float(np.nextafter(np.float32(2.0 ** -14), np.float32(0.0))), 2.0 ** -14, float(np.nextafter(np.float32(2.0 ** -14), np.float32(1.0))),
             -float(np.nextafter(np.float32(2.0 ** -14), np.float32(0.0))), -2.0 ** -14, -float(np.nextafter(np.float32(2.0 ** -14), np.float32(1.0))),
             65504.0, float(np.nextafter(np.float32(65504.0), np.float32(np.inf))), 65519.996, 65520.0, 1e5,
             -65504.0, -float(np.nextafter(np.float32(65504.0), np.float32(np.inf))), -65519.996, -65520.0, -1e5,
             float('inf'), -float('inf'), float('nan')]
_SWEEP = None


def split_sweep():
    """every finite float16 value v as float32, v + j * ulp16(v) / 8192 for j in {+-1, +-4095, +-4096 (the tie), +-4097, +-8191} (ulp16 /
    8192 is one float32 ulp of a normal v: all exact), and the specials; padded with ones to a multiple of 192.  float32 [about 7e5]."""
    global _SWEEP
    if _SWEEP is None:
        bits = np.concatenate([np.arange(0x0000, 0x7C00), np.arange(0x8000, 0xFC00)]).astype(np.uint16)
        v = bits.view(np.float16).astype(np.float64)
        _, e = np.frexp(np.where(v == 0.0, 1e-30, v))
        step = np.ldexp(1.0, np.maximum(e - 1, -14) - 10 - 13)
        js = [0, 1, -1, 4095, -4095, 4096, -4096, 4097, -4097, 8191, -8191]
        pts = np.concatenate([v + j * step for j in js])
        assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)          # every point is a float32
        s = np.concatenate([pts.astype(np.float32), np.array(_SPECIALS, np.float64).astype(np.float32)])
        s[:v.size] = bits.view(np.float16).astype(np.float32)                          # (keeps the sign of -0)
        _SWEEP = np.concatenate([s, np.ones(-s.size % 192, np.float32)])
        _SWEEP.setflags(write=False)
    return _SWEEP


def is_f32_subnormal(x):
    x = np.asarray(x, np.float32)
    return (x != 0) & (np.abs(x) < np.float32(2.0 ** -126))


# ---- the bound of the rounding leg --------------------------------------------------------------------------------------------------
U = {'f32': 0.0, 'bf16': 2.0 ** -8, 'f16': 2.0 ** -11, 'split': 2.0 ** -22}
ROUNDINGS = {'fir_down': 8, 'fir_up': 8, 'box_down': 3, 'box_up': 0, 's2d': 0}       # 0: a copy, judged by equality


def bound(kind, mode, y, s):
    """per-element bound on |stored - y| (the module docstring derives it): y the float64 result, s = sum |w x| of its terms"""
    assert ROUNDINGS[kind] > 0
    y = np.abs(y)
    tiny = 0.0
    if mode == 'f16':
        tiny = 2.0 ** -25                                     # half a subnormal step
    if mode == 'split':                                       # (2^-13 and not 2^-14: the value that was split is r, not y)
        tiny = np.where(y < 2.0 ** -13, 2.0 ** -25, 2.0 ** -36)
    return 1.001 * (U[mode] * y + ROUNDINGS[kind] * E32 * s) + tiny


# ---- the launches -------------------------------------------------------------------------------------------------------------------
# kind: fir_down / fir_up (dts_resample_fir), box_down / box_up (dts_resample2x), s2d (dts_space_to_depth2).  layout (s2d): 'nchw' (the
# float32 image), 'vec' (NHWC, c a whole number of the thread's vectors), 'elem' (NHWC, element by element).  cpad (s2d): the output channels.
Case = collections.namedtuple('Case', 'name kind kernel mode n h w c layout cpad variants')

_T = {'f32': 'float', 'bf16': 'bf16_t', 'f16': 'f16_t', 'split': 'float'}


def kernel_name(kind, mode, layout=None):
    """the template instantiation a launch runs, spelled as in the sources"""
    sp = 'true' if mode == 'split' else 'false'
    if kind.startswith('fir'):
        return f'resample_fir_kernel<{_T[mode]}, {sp}>'
    if kind.startswith('box'):
        return f'resample_kernel<{_T[mode]}>'
    return f'space_to_depth2_kernel<{_T[mode]}, {sp}, {"true" if layout == "nchw" else "false"}, {"true" if layout == "vec" else "false"}>'


# every instantiation in csrc/resample.hip (plus resample_kernel of csrc/groupnorm.hip, which dts_resample2x launches)
INSTANCES = tuple([kernel_name('fir', m) for m in MODES] + [kernel_name('box', m) for m in MODES[:3]]
                  + [kernel_name('s2d', m, lay) for m in MODES for lay in ('nchw', 'vec', 'elem')])

# every (kernel family, cell) without a case, and why
ABSENT = {
    ('dts_resample_fir', 'split from bf16 / f16'): 'the split image is written from float32 activations only (refused: test_refusals)',
    ('dts_resample2x', 'split'): 'no split_out form: the 2x2-averaged split image is dts_gn_apply_x3\'s raw output (tests/test_gpu_groupnorm.py)',
    ('dts_space_to_depth2', 'nchw + vec'): 'space_to_depth2_kernel<T, SPLIT, true, true> is never instantiated: NCHW channels are not contiguous',
    ('dts_space_to_depth2', 'split from bf16 / f16'): 'the split image is written from float32 activations only (refused: test_refusals)',
    ('dts_space_to_depth2', 'nchw bf16 / f16 input'): 'the NCHW source is the float32 image whatever the output type (x_nchw_f32)',
    ('dts_split3_f16', 'bf16 / f16 / f32 out'): 'one kernel: float32 in, the f16 image out',
    ('dts_split2_f16', 'bf16 / f16 / f32 out'): 'one kernel: float32 in, the f16 image out',
}

DOWN_HW = ((2, 2), (2, 6), (6, 2), (4, 10))
UP_HW = ((1, 1), (1, 3), (3, 1), (3, 5), (4, 2))
S2D_HW = ((2, 2), (2, 6), (6, 2), (12, 8))
FIR_C = {'f32': (4, 12), 'bf16': (8, 24, 40), 'f16': (8, 24, 40), 'split': (32, 96)}
BOX_C = {'f32': (4, 12), 'bf16': (8, 24, 40), 'f16': (8, 24, 40)}
S2D_C = {'nchw': {m: (3, 5) for m in MODES}, 'vec': {m: (8, 40) for m in MODES},
         'elem': {'f32': (6,), 'bf16': (4, 12), 'f16': (4, 12), 'split': (4, 12)}}


def _round_up(v, g):
    return -(-v // g) * g


def _build_cases():
    cases, k = collections.OrderedDict(), 0

    def add(kind, mode, h, w, c, layout=None, cpad=0, tag=''):
        nonlocal k
        n = (1, 3)[k % 2]
        k += 1
        name = f'{kind}_{mode}_{h}x{w}_c{c}_n{n}' + (f'_{layout}_cpad{cpad}{tag}' if kind == 's2d' else '')
        variants = ('lat', 'lo') if mode in ('f32', 'split') and kind != 'box_up' and kind != 'box_down' else ('lat',)
        assert name not in cases
        cases[name] = Case(name, kind, kernel_name(kind, mode, layout), mode, n, h, w, c, layout, cpad, variants)

    for mode in MODES:
        for kind, hws in (('fir_down', DOWN_HW), ('fir_up', UP_HW)):
            for h, w in hws:
                for c in FIR_C[mode]:
                    add(kind, mode, h, w, c)
    for mode in MODES[:3]:
        for kind, hws in (('box_down', DOWN_HW), ('box_up', UP_HW)):
            for h, w in hws:
                for c in BOX_C[mode]:
                    add(kind, mode, h, w, c)
    for mode in MODES:
        for layout in ('nchw', 'vec', 'elem'):
            for c in S2D_C[layout][mode]:
                for h, w in S2D_HW:
                    cp = _round_up(4 * c, GRANULE[mode])                       # what ops.space_to_depth2 chooses
                    add('s2d', mode, h, w, c, layout, cp)
                    add('s2d', mode, h, w, c, layout, cp + GRANULE[mode])      # an explicit cpad: one whole granule more
                    tight = _round_up(4 * c, 32 if mode == 'split' else EPV[mode])     # the least the ABI takes
                    if tight != cp and (h, w) == (2, 6):
                        add('s2d', mode, h, w, c, layout, tight, '_tight')
    return cases


CASES = _build_cases()

# the split images: (function, c1, c2) over the whole sweep
SPLIT_CASES = (('dts_split3_f16', 32, 0), ('dts_split3_f16', 8, 24), ('dts_split3_f16', 40, 24), ('dts_split2_f16', 8, 0), ('dts_split2_f16', 192, 0))

# one launch per grid-stride kernel whose thread count exceeds the launch cap (blocks x 256) by less than one block: the second trip of the
# loop, taken by some threads only.  (name, cap in threads, Case or (function, c1, c2, rows))
GRID_STRIDE = (
    ('fir', 2048 * 256, Case('grid_fir_up_f16_34x241_c128', 'fir_up', kernel_name('fir', 'f16'), 'f16', 1, 34, 241, 128, None, 0, ('lat',))),
    ('s2d', 2048 * 256, Case('grid_s2d_bf16_396x662_c16', 's2d', kernel_name('s2d', 'bf16', 'vec'), 'bf16', 1, 396, 662, 16, 'vec', 64, ('lat',))),
    ('box', 4096 * 256, Case('grid_box_up_f16_29x565_c128', 'box_up', kernel_name('box', 'f16'), 'f16', 1, 29, 565, 128, None, 0, ('lat',))),
    ('split3', 2048 * 256, ('dts_split3_f16', 8, 24, 131075)),
    ('split2', 2048 * 256, ('dts_split2_f16', 8, 0, 524388)),
)

# the rounding leg (Gaussian inputs): one non-square shape per kernel and type
def _rounding_cases():
    out = []
    for mode, c in (('f32', 12), ('bf16', 24), ('f16', 24), ('split', 96)):
        for kind, h, w in (('fir_down', 6, 10), ('fir_up', 3, 5), ('box_down', 6, 10), ('box_up', 3, 5)):
            if not (kind.startswith('box') and mode == 'split'):
                out.append(Case(f'gauss_{kind}_{mode}', kind, kernel_name(kind, mode), mode, 2, h, w, c, None, 0, ('gauss',)))
        for layout in ('nchw', 'vec', 'elem'):
            cs = S2D_C[layout][mode][-1]
            out.append(Case(f'gauss_s2d_{layout}_{mode}', 's2d', kernel_name('s2d', mode, layout), mode, 2, 6, 10, cs, layout,
                            _round_up(4 * cs, GRANULE[mode]), ('gauss',)))
    return tuple(out)


ROUNDING = _rounding_cases()


def threads(case):
    """threads' worth of work of a launch (one output vector each)"""
    if case.kind == 's2d':
        return case.n * (case.h // 2) * (case.w // 2) * (case.cpad // EPV[case.mode])
    up = case.kind.endswith('up')
    ho, wo = (2 * case.h, 2 * case.w) if up else (case.h // 2, case.w // 2)
    return case.n * ho * wo * (case.c // EPV[case.mode])


def launches():
    return [(name, v) for name, c in CASES.items() for v in c.variants]


def in_shape(case):
    return (case.n, case.c, case.h, case.w) if case.layout == 'nchw' else (case.n, case.h, case.w, case.c)


def case_input(case, variant='lat', seed=0):
    """the exact input of a case (float64; NCHW for the nchw layout)"""
    s = hash_name(case.name) + seed
    return lattice(case.kind, in_shape(case), s, lo=variant == 'lo')


def hash_name(name):
    v = 0
    for ch in name:
        v = (v * 131 + ord(ch)) % 1000003
    return v


def reference(case, x, mistake=None, want_s=False):
    """the float64 result of a case on the input x"""
    if case.kind == 'fir_down':
        return fir_down(x, mistake, want_s)
    if case.kind == 'fir_up':
        return fir_up(x, mistake, want_s)
    if case.kind == 'box_down':
        return mean2x2_down(x, mistake, want_s)
    if case.kind == 'box_up':
        o = nearest_up(x, mistake)
        return (o, np.abs(o)) if want_s else o
    o = space_to_depth2(x, case.cpad, case.layout == 'nchw', mistake)
    return (o, np.abs(o)) if want_s else o
