"""The convolution in float64, written from the definition, the inputs that make every launch route of dts_conv2d / dts_conv_in3 /
dts_conv_out3 EXACT, and the table of launches the GPU file runs (tests/test_gpu_conv.py).  Torch on the CPU only: nothing here calls
F.conv2d or anything of diffusion_tts_amd / oracle, so the kernels meet something that shares no code with them
(tests/test_conv_reference.py pins this file and shows that its sparse integer inputs hide no indexing fault).

Why exact.  Activations in {0, +-1, +-2}, weights in {0, +-1}, epilogue operands integers in [-8, 8], out_scale 1 or 0.5 (the `x_lo` /
`w_lo` variants add a term of 2^-13 / 2^-12 that lives in the lo plane of the split-precision images).  Every product and every partial
sum, in ANY order, is then an integer multiple of 2^-14 of magnitude below 2^8 (assert_exact_conditions: S <= 256): 22 bits, exact in the
f32 accumulators of every kernel, in the bf16 / f16 storage of the operands, under the 2^k scaling of the packed split-precision weights,
and -- where the result itself is representable in the output type, which is asserted too -- in the stored output.  A kernel must then
return the float64 result BIT FOR BIT whatever its summation order; any halo, border, concat-offset, upsample-mapping, split-K or epilogue
mistake is a nonzero difference."""
import collections
import math

import torch

MODES = ('f32', 'bf16', 'f16', 'f16x3')
H16 = ('bf16', 'f16')               # the 16-bit storage modes
W32 = ('f32', 'f16x3')              # float32 activations and outputs
STORE = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16, 'f16x3': torch.float32}     # storage type of activations / outputs
GRANULE = {'f32': 32, 'bf16': 64, 'f16': 64, 'f16x3': 32}       # input channels of one K step (128 bytes of the staged row)

Ref = collections.namedtuple('Ref', 'o S prod')          # result, sum of magnitudes of everything added, the products' part of S (both * |out_scale|)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def upsample2(x):
    """nearest 2x by index: output pixel (h, w) is input pixel (h >> 1, w >> 1)"""
    return x[:, :, torch.arange(2 * x.shape[2]) >> 1][:, :, :, torch.arange(2 * x.shape[3]) >> 1]


def norm_input(x, gn):
    """act(x * a + b) per (sample, channel); gn = (a [n, c], b [n, c], silu) or None"""
    if gn is None:
        return x
    a, b, silu = gn
    y = x * a.double()[:, :, None, None] + b.double()[:, :, None, None]
    return y * torch.sigmoid(y) if silu else y


def prepare_input(x1, x2, gn=None, up=False):
    """the tensor the taps read, before the zero padding: concatenate, normalise, upsample"""
    x = norm_input(torch.cat([x1.double()] + ([] if x2 is None else [x2.double()]), 1), gn)
    return upsample2(x) if up else x


def tap_sums(x, w):
    """sum over the k*k taps of einsum(w[:, :, kh, kw], shifted slice of the zero-padded x); x NCHW float64, w OIHW float64.
    Returns (conv, sum |x||w|)."""
    n, c, h, wd = x.shape
    k = w.shape[2]
    p = k // 2
    xp = torch.zeros(n, c, h + 2 * p, wd + 2 * p, dtype=torch.float64)
    xp[:, :, p:p + h, p:p + wd] = x
    o = torch.zeros(n, w.shape[0], h, wd, dtype=torch.float64)
    s = torch.zeros_like(o)
    for kh in range(k):
        for kw in range(k):
            xs = xp[:, :, kh:kh + h, kw:kw + wd]
            o += torch.einsum('oc,nchw->nohw', w[:, :, kh, kw], xs)
            s += torch.einsum('oc,nchw->nohw', w[:, :, kh, kw].abs(), xs.abs())
    return o, s


def epilogue(o, s, bias, bias_nc, residual, out_scale):
    """(o + bias + bias_nc + residual) * out_scale and the magnitudes that went into it: Ref(o, S, prod)"""
    prod = s.clone()
    if bias is not None:
        o = o + bias.double()[None, :, None, None]
        s = s + bias.double().abs()[None, :, None, None]
    if bias_nc is not None:
        o = o + bias_nc.double()[:, :, None, None]
        s = s + bias_nc.double().abs()[:, :, None, None]
    if residual is not None:
        o = o + residual.double()
        s = s + residual.double().abs()
    return Ref(o * out_scale, s * abs(out_scale), prod * abs(out_scale))


def conv_ref64(x1, x2, w, bias, bias_nc, residual, up, out_scale, gn=None, skip=None):
    """(conv(act(concat(x1, x2) * a + b) [nearest 2x]) + bias + bias_nc + residual [+ 1x1 conv of the skip source]) * out_scale in float64.
    x1, x2 NCHW; w OIHW (k = 1 or 3, zero padding k // 2, the padding applied AFTER the gn affine); bias [cout]; bias_nc [n, cout]; residual
    [n, cout, ho, wo]; gn = (a [n, cin], b [n, cin], silu); skip = (src NCHW, w_skip [cout, cs, 1, 1], up).  Returns Ref(o, S, prod) with
    S = (sum |x||w| + |bias| + |bias_nc| + |residual|) * |out_scale| per output element and prod the products' share of it."""
    o, s = tap_sums(prepare_input(x1, x2, gn, up), w.double())
    if skip is not None:
        src, w_skip, s_up = skip
        o2, s2 = tap_sums(prepare_input(src, None, None, s_up), w_skip.double())
        o, s = o + o2, s + s2
    return epilogue(o, s, bias, bias_nc, residual, out_scale)


def strip_stats64(o):
    """GroupNorm moments as the conv epilogue emits them: per 64 consecutive NHWC pixels and channel (sum, sum of squares), float64
    [n*h*w / 64, c, 2]; o NCHW."""
    n, c, h, w = o.shape
    v = o.double().permute(0, 2, 3, 1).reshape(-1, 64, c)
    return torch.stack([v.sum(1), (v * v).sum(1)], dim=-1)


def image_stats64(o):
    """the same moments per image [n, c, 2] (the ping-pong kernel's strips are patch rows: only their sums per image are layout-free)"""
    v = o.double().flatten(2)
    return torch.stack([v.sum(2), (v * v).sum(2)], dim=-1)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ---- the launches -----------------------------------------------------------------------------------------------------------------
# form: the kernel (form) a case is meant for.  What ops.conv_kernel answers for it: igemm* -> 0, pp192* -> 6, pp128* -> 4.
FORMS = ('igemm', 'igemm_splitk', 'pp192', 'pp128', 'pp_splitk', 'pp_gn', 'pp_skip', 'in3_direct', 'in3_mfma', 'out3_tiled', 'out3_direct')

# every (form, mode) cell without a case, and why
ABSENT = {
    ('pp192', 'f32'): 'no f32 ping-pong form (the kernel is 16-bit matrix instructions only)',
    ('pp128', 'f32'): 'no f32 ping-pong form',
    ('pp_splitk', 'f32'): 'no f32 ping-pong form',
    ('pp_gn', 'f32'): 'no f32 ping-pong form',
    ('pp_gn', 'f16x3'): 'gn_coef refused in F16X3 (dts_conv2d)',
    ('pp_skip', 'f32'): 'the skip fold is the split-precision mode\'s (dts_conv_folds_skip)',
    ('pp_skip', 'bf16'): 'the skip fold is the split-precision mode\'s',
    ('pp_skip', 'f16'): 'the skip fold is the split-precision mode\'s',
    ('in3_direct', 'f16x3'): 'the first convolution reads the f32 image: no split-precision form',
    ('in3_mfma', 'f16x3'): 'the first convolution reads the f32 image: no split-precision form',
    ('out3_tiled', 'f16x3'): 'float32 activations take the f32 kernel (covered as f32)',
    ('out3_direct', 'f16x3'): 'float32 activations take the f32 kernel (covered as f32)',
}

# knob forms that do not exist (the knob is ignored there), so no case claims them
KNOB_ABSENT = {
    ('conv_waves', 'f32'): 'the f32 parity kernel has one configuration: 4 waves',
    ('conv_stages', 'f32'): 'the f32 parity kernel has one configuration: a 2-deep ring',
    ('conv_stages=4', 'f16x3'): 'the 4-deep ring is instantiated for 16-bit outputs only (f16x3 takes the 3-deep one)',
    ('conv_stages=4 + conv_waves=8', 'any'): 'the 8-wave form has 2- and 3-deep rings only',
    ('conv_epi32', 'bf16 / f16'): 'the knob selects among the epilogues of f32 outputs',
}

Case = collections.namedtuple('Case', 'name form modes n h w c1 c2 cout k up ep scale stats knobs variants gn skip split2 splits note')

CASES = collections.OrderedDict()


def _case(name, form, modes, n, h, w, c1, cout, k=3, c2=0, up=False, ep='b', scale=1.0, stats=False, knobs=(), variants=('int',), gn=False,
          skip=None, split2=False, splits=None, note=''):
    """ep: which epilogue operands are present -- b bias, B bias handed over ONE FLOAT INTO ITS STORAGE (not 16-byte aligned: the first
    convolution's route depends on it), n bias_nc, N bias_nc as a column slice of a [n, 2*cout] tensor, r residual.
    h, w: the INPUT size (the output is twice that with up).  knobs: ((name, value), ...) set around the launch.
    splits: how K is split, which decides whether the kernel's OWN epilogue runs or the reduce pass's (ops.conv_kernel cannot tell them
    apart, and left alone the launchers split most small grids by an estimate of their own):
        1 (the default of every dts_conv2d case)  pinned unsplit with conv_splits = 1: the kernel's own epilogue;
        s > 1  forced with conv_splits = s: partial slabs + reduce pass (effective_splits() restates what the launcher makes of s);
        -1  the launcher's own choice (the `auto_*` cases);
        0  no knob: the skip fold (never split; the fold refuses a set conv_splits) and the first / last convolutions.
    skip: (cs, up[, unit of the skip weights: 2^-6 unless given]) of the folded 1x1 skip convolution.
    stats: the launch is asked for the strip statistics (with the integer inputs only: the squares of the lo-plane variants' outputs,
    multiples of 2^-26, do not sum exactly in float32)."""
    assert name not in CASES and form in FORMS
    if splits is None:
        splits = 0 if (skip is not None or form.startswith('in3') or form.startswith('out3')) else 1
    knobs = tuple(knobs)
    assert 'conv_splits' not in dict(knobs)
    if splits > 0:
        knobs += (('conv_splits', splits),)
    assert (splits > 1) == form.endswith('_splitk'), name
    CASES[name] = Case(name, form, tuple(modes), n, h, w, c1, c2, cout, k, up, ep, scale, stats, knobs, tuple(variants), gn, skip, split2,
                       splits, note)


ALL = MODES
# -- implicit GEMM: tiles (cout 64: 64 x 256 tiles; 128 / 192: 128- / 192-cout x 128-pixel tiles; 576 = 3 x 192)
_case('tile64', 'igemm', ALL, 2, 8, 8, 64, 64, stats=True)
_case('tile128', 'igemm', ALL, 2, 8, 8, 64, 128, stats=True)
_case('tile192', 'igemm', ALL, 2, 8, 8, 64, 192, stats=True)
_case('tile576', 'igemm', ALL, 1, 8, 8, 64, 576, ep='br')
# -- forced knob forms (cout 384: 2 x 192 by default)
for _t in (64, 128):
    _case(f'knob_tile{_t}', 'igemm', ALL, 1, 8, 16, 64, 384, ep='bnr', knobs=(('conv_tile', _t),))
M16 = H16 + ('f16x3',)             # the modes that run on the 16-bit matrix instructions
for _w in (4, 8):
    _case(f'knob_waves{_w}', 'igemm', M16, 2, 8, 8, 128, 128, ep='br', stats=True, knobs=(('conv_waves', _w),))
    _case(f'knob_waves{_w}_split2', 'igemm_splitk', M16, 2, 8, 8, 128, 128, ep='br', stats=True, knobs=(('conv_waves', _w),), splits=2)
for _s in (2, 3, 4):
    _case(f'knob_stages{_s}', 'igemm', H16 if _s == 4 else M16, 2, 8, 8, 128, 192, ep='br', stats=True, knobs=(('conv_stages', _s), ('conv_waves', 4)))
for _s in (2, 3):
    _case(f'knob_stages{_s}_waves8', 'igemm', M16, 1, 8, 16, 128, 128, k=1, ep='bn', knobs=(('conv_stages', _s), ('conv_waves', 8)))
_case('knob_stages3_split3', 'igemm_splitk', M16, 2, 8, 8, 192, 192, ep='bnr', stats=True, knobs=(('conv_stages', 3), ('conv_waves', 4)), splits=3)
# conv_epi32 (f32 outputs): 0 = accumulator-layout epilogue, 1 = row-layout epilogue (needs hout * wout % 64 == 0; the ragged twins stay
# on the accumulator layout whatever the knob says), 2 = row layout with the former store form of an out_split2 output
for _e in (0, 1, 2):
    _case(f'knob_epi32_{_e}', 'igemm', W32, 2, 8, 8, 64, 192, ep='bnr', scale=0.5, stats=True, knobs=(('conv_epi32', _e),))
    _case(f'knob_epi32_{_e}_ragged', 'igemm', W32, 3, 5, 7, 64, 128, ep='bnr', knobs=(('conv_epi32', _e),))
    _case(f'knob_epi32_{_e}_split2', 'igemm', ('f16x3',), 2, 8, 8, 64, 192, k=1, ep='b', variants=('x_lo',), split2=True, knobs=(('conv_epi32', _e),))
# -- K loops of one and two steps (a granule is 32 channels in f32 / f16x3, 64 in bf16 / f16), also with a ring deeper than the loop
# (the prologue issues tile q only if ks_begin + q < ks_end: conv_igemm_kernel)
_case('k1_c32', 'igemm', W32, 2, 8, 8, 32, 64, k=1, stats=True)
_case('k1_c64', 'igemm', ALL, 2, 8, 8, 64, 64, k=1, stats=True)
_case('k1_c128', 'igemm', ALL, 2, 8, 8, 128, 128, k=1)
_case('k3_c32', 'igemm', W32, 1, 8, 8, 32, 64)
_case('k3_c64', 'igemm', ALL, 1, 8, 8, 64, 64)
for _s in (3, 4):
    _case(f'k1_c64_ring{_s}', 'igemm', H16 if _s == 4 else M16, 2, 8, 8, 64, 128, k=1, ep='br', knobs=(('conv_stages', _s), ('conv_waves', 4)),
          note='ring deeper than the K loop (one step in 16-bit, two in f16x3)')
    _case(f'k1_c128_ring{_s}', 'igemm', H16 if _s == 4 else M16, 1, 5, 7, 128, 64, k=1, ep='bn', knobs=(('conv_stages', _s), ('conv_waves', 4)))
# -- forced K splits: nk = 18 (even and uneven: 8 -> 6 splits of 3) and nk = 27 (2 -> 14 + 13, 3 -> 9 each, 8 -> 7 splits of 4, the last of 3)
for _s in (2, 3, 8):
    for _nk, _c16 in ((18, 128), (27, 192)):
        _case(f'split{_s}_nk{_nk}_16bit', 'igemm_splitk', H16, 2, 8, 8, _c16, 128, ep='b', splits=_s)
        _case(f'split{_s}_nk{_nk}_32bit', 'igemm_splitk', W32, 2, 8, 8, _c16 // 2, 128, ep='b', splits=_s)
# the reduce pass is a template over its slab count (conv_splitk_reduce_kernel<T, SPLITS> and conv_splitk_reduce_stats_kernel<T, SPLITS>,
# SPLITS 2..8); the cases above end at 2, 3, 6 and 7 slabs.  SPLITS 4 and 5 at nk = 18 (4 -> 5 + 5 + 5 + 3, 5 -> 4 + 4 + 4 + 4 + 2), SPLITS 8 at
# nk = 36 (8 -> seven splits of 5 and one of 1); each once through the plain reduce kernel and once (`_stats`: 2 strips of 64 pixels) through
# the one that also writes the strip statistics
for _s, _nk, _c16 in ((4, 18, 128), (5, 18, 128), (8, 36, 256)):
    for _st in (False, True):
        _sfx = '_stats' if _st else ''
        _case(f'split{_s}_nk{_nk}_16bit{_sfx}', 'igemm_splitk', H16, 2, 8, 8, _c16, 128, ep='b', stats=_st, splits=_s)
        _case(f'split{_s}_nk{_nk}_32bit{_sfx}', 'igemm_splitk', W32, 2, 8, 8, _c16 // 2, 128, ep='b', stats=_st, splits=_s)
# the plain reduce kernel's grid-stride loop: P * cout / 4 = 32775 * 16 = 524,400 threads' worth against the cap of 2048 blocks x 256 =
# 524,288: 112 threads take a SECOND trip (the last 7 pixels: 448 output elements).  32775 pixels are no whole strips, so the plain kernel
# runs whatever is asked.  Two f32 slabs of 32775 x 64: 16.8 MB of the 96 MB workspace.  nk = 9 (16-bit: 5 + 4) / 18 (9 + 9).
_case('split2_reduce_2trips', 'igemm_splitk', ALL, 1, 75, 437, 64, 64, ep='bnr', splits=2)
_case('split3_full_16bit', 'igemm_splitk', H16, 2, 8, 8, 192, 192, ep='bNr', scale=0.5, stats=True, splits=3)
_case('split3_full_32bit', 'igemm_splitk', W32, 2, 8, 8, 96, 192, ep='bNr', scale=0.5, stats=True, splits=3)
_case('split2_ragged', 'igemm_splitk', ALL, 3, 5, 7, 128, 64, ep='bnr', splits=2)
_case('split2_cat', 'igemm_splitk', ALL, 2, 8, 8, 64, 128, c2=128, ep='b', stats=True, splits=2)
# split twins of cases that run unsplit elsewhere in this table: epilogue operands, statistics, upsample through the reduce pass
_case('epi_all_split2', 'igemm_splitk', ALL, 2, 8, 8, 128, 128, ep='bnr', scale=0.5, stats=True, splits=2)
_case('up_res_split2', 'igemm_splitk', ALL, 2, 4, 8, 128, 192, up=True, ep='br', scale=0.5, stats=True, splits=2)
_case('auto_3x3_c128', 'igemm', ALL, 2, 8, 8, 128, 128, ep='bnr', stats=True, splits=-1, note='whatever the launcher\'s estimate picks')
# -- geometry
_case('ragged_3x5x7', 'igemm', ALL, 3, 5, 7, 64, 64, ep='bnr', stats=True)                           # 105 pixels: one partial tile, division path
_case('image_1x1', 'igemm', ALL, 1, 1, 1, 64, 64)                                         # every tap but the centre is padding
_case('h_is_1', 'igemm', ALL, 1, 1, 40, 64, 128)
_case('w_is_1', 'igemm', ALL, 2, 9, 1, 64, 64, ep='br', stats=True)              # (statistics asked for, none possible: 9 pixels)
_case('rows_samples_2x12x20', 'igemm', ALL, 2, 12, 20, 64, 128, ep='bn')                  # 480 pixels: tiles cross rows and samples, division path
_case('shift_1x8x32', 'igemm', ALL, 1, 8, 32, 64, 128, ep='br', stats=True)               # power-of-two, non-square: shift path; whole tiles (early residual fetch)
_case('geom_1x24x40', 'igemm', ALL, 1, 24, 40, 64, 64, ep='br', stats=True)               # 960 pixels = 15 strips, 4 tiles of 256 (the last partial)
_case('grid1', 'igemm', ALL, 1, 6, 9, 64, 192)                                            # blocks of the grid: 1, 3, 7, 9, 13 (the XCD remap's remainder branch)
_case('grid3', 'igemm', ALL, 1, 12, 25, 64, 192, ep='bn')
_case('grid7', 'igemm', ALL, 1, 24, 35, 64, 128, ep='br')
_case('grid9', 'igemm', ALL, 2, 12, 16, 64, 576, ep='bnr', stats=True)
_case('grid13', 'igemm', ALL, 1, 40, 41, 64, 128)
# -- fused nearest-2x upsample
_case('up_3x5', 'igemm', ALL, 2, 3, 5, 64, 64, up=True)                                 # odd sources -> 6x10
_case('up_cat', 'igemm', ALL, 1, 3, 5, 64, 128, c2=128, up=True, ep='bn')
_case('up_res', 'igemm', ALL, 2, 4, 8, 64, 192, up=True, ep='br', scale=0.5, stats=True)
_case('up_1x1', 'igemm', ALL, 2, 3, 5, 128, 64, k=1, up=True, ep='bn')
# -- concat under a 3x3
_case('cat_128_64', 'igemm', ALL, 2, 6, 7, 128, 128, c2=64)
_case('cat_64_128', 'igemm', ALL, 2, 6, 7, 64, 128, c2=128, ep='br')
_case('cat_32_96', 'igemm', ('f32',), 2, 6, 7, 32, 64, c2=96, note='f16x3 reads ONE source, the split image of the concat (32 + 96 channels there too)')
_case('cat_32_96_x3', 'igemm', ('f16x3',), 2, 6, 7, 32, 64, c2=96, variants=('int', 'x_lo'))
# -- epilogue operands, each alone and all together
_case('epi_none', 'igemm', ALL, 2, 8, 8, 64, 128, ep='', stats=True)
_case('epi_bias', 'igemm', ALL, 2, 8, 8, 64, 128, ep='b')
_case('epi_bias_nc', 'igemm', ALL, 2, 8, 8, 64, 128, ep='n')
_case('epi_residual', 'igemm', ALL, 2, 8, 8, 64, 128, ep='r')
_case('epi_scale', 'igemm', ALL, 2, 8, 8, 64, 128, ep='', scale=0.5, stats=True)
_case('epi_all', 'igemm', ALL, 2, 8, 8, 64, 128, ep='bnr', scale=0.5, stats=True)
_case('epi_wide_bias_nc', 'igemm', ALL, 3, 5, 7, 64, 192, ep='N')
_case('epi_all_wide_1x1', 'igemm', ALL, 2, 8, 8, 128, 64, k=1, ep='bNr', scale=0.5, stats=True)
# -- lo planes of the split images (F32 runs the same inputs through the f32 kernel)
_case('lo_planes', 'igemm', W32, 2, 8, 8, 64, 128, ep='bnr', variants=('x_lo', 'w_lo'))
_case('lo_planes_1x1', 'igemm', W32, 3, 5, 7, 96, 64, k=1, variants=('x_lo', 'w_lo'))
_case('out_split2', 'igemm', ('f16x3',), 2, 8, 8, 64, 192, k=1, ep='b', variants=('x_lo',), split2=True)
_case('out_split2_ragged', 'igemm', ('f16x3',), 3, 5, 7, 64, 192, k=1, ep='b', variants=('x_lo',), split2=True)

# -- ping-pong kernel (forced with conv_variant 1): square power-of-two images >= 16, whole 256-pixel tiles
PPM = H16 + ('f16x3',)
_PP = (('conv_variant', 1),)
_case('pp192_16x16', 'pp192', PPM, 1, 16, 16, 64, 192, knobs=_PP, stats=True)                                       # linear tiles
_case('pp192_16x16_n2', 'pp192', PPM, 2, 16, 16, 128, 192, ep='bNr', scale=0.5, stats=True, knobs=_PP, variants=('int', 'x_lo', 'w_lo'))
_case('pp192x2_32x32_cat', 'pp192', PPM, 1, 32, 32, 64, 384, c2=64, ep='bn', stats=True, knobs=_PP)                 # 16x16 patches, two cout tiles
_case('pp192_64x64', 'pp192', PPM, 1, 64, 64, 64, 192, ep='br', stats=True, knobs=_PP)
_case('pp192_up8', 'pp192', PPM, 1, 8, 8, 64, 192, up=True, ep='br', stats=True, knobs=_PP)
_case('pp192_up16_cat', 'pp192', PPM, 1, 16, 16, 64, 192, c2=64, up=True, ep='bn', knobs=_PP)
_case('pp128_32x32', 'pp128', PPM, 1, 32, 32, 64, 128, ep='br', stats=True, knobs=_PP, variants=('int', 'x_lo', 'w_lo'))
_case('pp128x2_16x16_n2', 'pp128', PPM, 2, 16, 16, 128, 256, ep='bN', scale=0.5, stats=True, knobs=_PP)
_case('pp128_16x16_cat', 'pp128', PPM, 1, 16, 16, 64, 128, c2=64, ep='n', knobs=_PP)
_case('pp128_up8', 'pp128', PPM, 2, 8, 8, 64, 128, up=True, ep='b', stats=True, knobs=_PP)
_case('pp128_up16', 'pp128', PPM, 1, 16, 16, 128, 128, up=True, ep='br', knobs=_PP)
# forced splits are whole 64-channel chunks of the staged image: 3 chunks -> 2 + 1 / 1 + 1 + 1, 5 chunks -> 3 + 2 / 2 + 2 + 1
# (the split image of f16x3 has twice the chunks: 6 -> 3 + 3 / 2 + 2 + 2, 10 -> 5 + 5 / 4 + 4 + 2)
_case('pp192_split2_c192', 'pp_splitk', PPM, 1, 16, 16, 192, 192, ep='b', knobs=_PP, splits=2)
_case('pp128_split3_c192', 'pp_splitk', PPM, 1, 16, 16, 192, 128, ep='bnr', stats=True, knobs=_PP, splits=3)
_case('pp192_split3_c320', 'pp_splitk', PPM, 1, 16, 16, 320, 192, ep='bnr', scale=0.5, stats=True, knobs=_PP, splits=3)
_case('pp128_split2_c320', 'pp_splitk', PPM, 2, 16, 16, 320, 128, ep='b', knobs=_PP, splits=2)
# the reduce pass at 5 and 8 slabs behind the ping-pong kernel: 5 chunks -> 1 + 1 + 1 + 1 + 1 (f16x3: 10 -> five splits of 2), 8 chunks -> eight
# splits of 1 (f16x3: 16 -> eight of 2); the first with the strip statistics (the reduce pass's statistics kernel), the second without
_case('pp192_split5_c320', 'pp_splitk', PPM, 1, 16, 16, 320, 192, ep='br', stats=True, knobs=_PP, splits=5)
_case('pp128_split8_c512', 'pp_splitk', PPM, 1, 16, 16, 512, 128, ep='bn', knobs=_PP, splits=8)
_case('pp192x2_32x32_cat_split2', 'pp_splitk', PPM, 1, 32, 32, 64, 384, c2=64, ep='bn', stats=True, knobs=_PP, splits=2)
_case('pp128x2_16x16_n2_split2', 'pp_splitk', PPM, 2, 16, 16, 128, 256, ep='bN', scale=0.5, stats=True, knobs=_PP, splits=2)
_case('pp_auto_c128', 'pp192', PPM, 2, 16, 16, 128, 192, ep='bnr', stats=True, knobs=_PP, splits=-1, note='whatever the launcher\'s estimate picks')
# fused GroupNorm apply with caller-made coefficients a in {1, 2, -1}, b in {-1, 0, 1}, no SiLU
_case('pp_gn_16x16', 'pp_gn', H16, 2, 16, 16, 128, 192, ep='b', stats=True, knobs=_PP, gn=True)
_case('pp_gn_32x32_cat', 'pp_gn', H16, 1, 32, 32, 64, 192, c2=64, ep='br', knobs=_PP, gn=True)
# the 1x1 skip convolution folded into the launch (skip weights in {0, +-2^-6})
_case('pp192_skip_same', 'pp_skip', ('f16x3',), 1, 16, 16, 64, 192, ep='b', knobs=_PP, skip=(64, False))
_case('pp192_skip_half', 'pp_skip', ('f16x3',), 1, 32, 32, 64, 192, ep='b', scale=0.5, knobs=_PP, skip=(128, True), variants=('int', 'x_lo'))
_case('pp128_skip_same', 'pp_skip', ('f16x3',), 2, 16, 16, 128, 128, ep='b', scale=0.5, knobs=_PP, skip=(64, False), variants=('int', 'w_lo'))
_case('pp128_skip_half', 'pp_skip', ('f16x3',), 1, 32, 32, 64, 256, ep='b', knobs=_PP, skip=(64, True))
# (outputs in units of 2^-6 have sums of squares beyond 24 bits: the statistics of a folded launch are checked with integer skip weights)
_case('pp192_skip_stats', 'pp_skip', ('f16x3',), 2, 16, 16, 64, 192, ep='b', stats=True, knobs=_PP, skip=(64, False, 1.0))
_case('pp128_skip_half_stats', 'pp_skip', ('f16x3',), 1, 16, 16, 64, 128, ep='b', stats=True, knobs=_PP, skip=(128, True, 1.0))

# -- first and last convolutions (conv_small.hip): c1 = 3 / cout = 3; the first reads the f32 NCHW image
F3 = ('f32', 'bf16', 'f16')
_case('in3_direct_12x20', 'in3_direct', F3, 2, 12, 20, 3, 64, ep='b')
_case('in3_direct_nobias', 'in3_direct', F3, 1, 12, 20, 3, 128, ep='')
_case('in3_mfma_16x16', 'in3_mfma', F3, 2, 16, 16, 3, 64, ep='b')
_case('in3_mfma_32x16', 'in3_mfma', F3, 1, 32, 16, 3, 192, ep='')
_case('in3_mfma_32x16_bias', 'in3_mfma', F3, 3, 32, 16, 3, 128, ep='b')
_case('out3_tiled_16x16', 'out3_tiled', F3, 2, 16, 16, 64, 3, ep='b')
_case('out3_tiled_32x48', 'out3_tiled', F3, 1, 32, 48, 192, 3, ep='b')
_case('out3_direct_12x20', 'out3_direct', F3, 2, 12, 20, 64, 3, ep='b')
_case('out3_direct_12x20_c192', 'out3_direct', F3, 1, 12, 20, 192, 3, ep='b')
# The loops of these kernels whose trip count the launcher derives from the size (small_trips() restates the rules; tests/test_conv_reference.py
# asserts every number written here).  In the cases above every such loop makes ONE trip.
# conv_in3_mfma_kernel, `seg += gridDim.x * 4`: 67 x 62 = 4154 segments of 16 pixels, 2 per wave -> 520 blocks = 2080 waves; 2074 waves take a
# second segment, the last 6 take one
_case('in3_mfma_67x992', 'in3_mfma', F3, 1, 67, 992, 3, 64, ep='b')
# 260 x 253 = 65780 segments, 8 per wave -> 2056 blocks, CAPPED at 2048 = 8192 waves: eight trips for every wave and a NINTH for 244 of them
# (65780 - 8 * 8192).  One mode: the float64 reference takes 2.3 GB.
_case('in3_mfma_260x4048', 'in3_mfma', ('bf16',), 1, 260, 4048, 3, 64, ep='b')
# conv_in3_kernel, `pbase += gridDim.x * 256`: 1,048,640 pixels against the cap of 4096 blocks x 256 = 1,048,576: block 0 takes a second trip
# of 64 pixels, through the LDS staging slab its first trip left behind
_case('in3_direct_928x1130_c8', 'in3_direct', F3, 1, 928, 1130, 3, 8, ep='b')
# its staging in groups of GRP = 8 output chunks of 16 bytes: cout 40 = 5 chunks in 16-bit (one ragged group), 10 in f32 (a full group and a
# ragged one of 2).  (cout 64 / 128 / 192 above: whole groups only)
_case('in3_direct_12x20_c40', 'in3_direct', F3, 2, 12, 20, 3, 40, ep='b')
# a shape the matrix-core kernel takes (w % 16 == 0, cout 64) with a bias that is not 16-byte aligned: the launcher must take the direct kernel
# (the other one reads the bias as float4)
_case('in3_direct_16x16_unaligned_bias', 'in3_direct', F3, 1, 16, 16, 3, 64, ep='B')
# conv_out3_kernel (4 lanes per pixel), `pix0 += gridDim.x * 64`: 524,320 pixels against the cap of 8192 blocks x 64 = 524,288: 32 pixels in a
# second trip
_case('out3_direct_464x1130_c8', 'out3_direct', F3, 1, 464, 1130, 8, 3, ep='b')
# c = 48: three channel chunks of 16 in the tiled f32 kernel; 48 % 32 != 0 sends the 16-bit modes to the direct kernel (6 chunks over 4 lanes)
_case('out3_tiled_16x16_c48', 'out3_tiled', ('f32',), 1, 16, 16, 48, 3, ep='b')
_case('out3_direct_16x16_c48', 'out3_direct', H16, 1, 16, 16, 48, 3, ep='b')

# the cases whose float64 reference is large (hundreds of MB to 2.3 GB): computed where they are used and dropped, never cached
LARGE = ('in3_mfma_260x4048', 'in3_direct_928x1130_c8', 'out3_direct_464x1130_c8')


def launches():
    """every (case, mode, variant) the GPU file runs, as pytest ids"""
    return [(c.name, m, v) for c in CASES.values() for m in c.modes for v in c.variants if v == 'int' or m in W32]


def out_hw(case):
    return (2 * case.h, 2 * case.w) if case.up else (case.h, case.w)


def igemm_blocks(case, mode):
    """blocks of conv_igemm_kernel's grid (x): cout tiles x pixel tiles; a 64-cout tile spans 256 pixels, the others 128"""
    tile = dict(case.knobs).get('conv_tile') or (192 if case.cout % 192 == 0 else 128 if case.cout % 128 == 0 else 64)
    ho, wo = out_hw(case)
    bn = 256 if tile == 64 else 128
    return (case.cout // tile) * -(-(case.n * ho * wo) // bn)


def k_steps(case, mode):
    """K steps of the launch: taps x granules of the staged channels"""
    return case.k * case.k * ((case.c1 + case.c2) // GRANULE[mode])


def effective_splits(case, mode):
    """(splits, K steps per split) a forced-split launch ends up with -- the launch plan's rules restated (conv_plan with igemm_splits / pp_splits, conv_igemm.hip).
    conv_igemm_kernel: conv_splits = s is honoured (at most 8) when nk >= 2 s; each split takes ceil(nk / s) steps and empty splits are
    dropped.  conv_pp_kernel: s is cut to nk / 8 and to the number of chunks (a chunk = all nine taps of one granule); each split takes
    ceil(chunks / s) whole chunks."""
    nk, s = k_steps(case, mode), min(case.splits, 8)
    if case.form == 'pp_splitk':
        chunks = nk // 9
        s = max(1, min(s, nk // 8, chunks))
        per = -(-chunks // s)
        return -(-chunks // per), per * 9
    if nk < 2 * s:
        return 1, nk
    per = -(-nk // s)
    return -(-nk // per), per


def small_route(case, mode):
    """the kernel a first / last convolution takes -- the launchers' rules restated (dts_conv_in3, dts_conv_out3: conv_small.hip).  The first:
    the matrix-core kernel iff w % 16 == 0, cout is 64 / 128 / 192 and the bias (if any) is 16-byte aligned.  The last: the tiled kernel iff
    h % 16 == 0, w % 16 == 0 and c is whole chunks of 4 vectors (16 channels in f32, 32 in 16-bit)."""
    if case.form.startswith('in3'):
        return 'in3_mfma' if case.w % 16 == 0 and case.cout in (64, 128, 192) and 'B' not in case.ep else 'in3_direct'
    assert case.form.startswith('out3')
    return 'out3_tiled' if case.h % 16 == 0 and case.w % 16 == 0 and case.c1 % (16 if mode == 'f32' else 32) == 0 else 'out3_direct'


Trips = collections.namedtuple('Trips', 'units per_wave blocks per_pass trips last_start')


def _ceil(a, b):
    return -(-a // b)


def small_trips(case, mode):
    """The size-driven loop of the kernel small_route() names, from the launchers' rules restated: units = what the loop walks (segments of 16
    pixels in conv_in3_mfma_kernel, pixels elsewhere), per_wave = segments a wave is meant to take (the matrix-core kernel only: nseg / 2048
    clamped to 1..8), blocks = the grid after its cap (2048 / 4096 / 8192), per_pass = units the whole grid covers in one trip, trips = the
    most trips any thread makes, last_start = the first output PIXEL of the last trip.  The tiled last convolution has no such loop."""
    route, npix = small_route(case, mode), case.n * case.h * case.w
    if route == 'in3_mfma':
        nseg = case.n * case.h * (case.w // 16)
        spw = max(1, min(8, nseg // 2048))
        blocks = min(_ceil(nseg, 4 * spw), 2048)
        trips = _ceil(nseg, 4 * blocks)
        return Trips(nseg, spw, blocks, 4 * blocks, trips, (trips - 1) * 4 * blocks * 16)
    if route == 'in3_direct':
        blocks = min(_ceil(npix, 256), 4096)
        trips = _ceil(npix, 256 * blocks)
        return Trips(npix, None, blocks, 256 * blocks, trips, (trips - 1) * 256 * blocks)
    if route == 'out3_direct':
        blocks = min(_ceil(4 * npix, 256), 8192)
        trips = _ceil(npix, 64 * blocks)
        return Trips(npix, None, blocks, 64 * blocks, trips, (trips - 1) * 64 * blocks)
    return Trips(npix, None, case.n * (case.h // 16) * (case.w // 16), npix, 1, 0)


def in3_direct_groups(case, mode):
    """chunks per staging round of conv_in3_kernel: cout / (channels of a 16-byte chunk) in groups of GRP = 8, the last one ragged"""
    nchunk = case.cout // (4 if mode == 'f32' else 8)
    return [min(8, nchunk - c0) for c0 in range(0, nchunk, 8)]


def reduce_trips(case, mode):
    """the grid-stride loop of conv_splitk_reduce_kernel (launch_reduce_n restated): one thread per 4 couts of a pixel, 2048 blocks of 256 at
    the most.  Trips(units = P * cout / 4, -, blocks, per_pass, trips, last_start = first output pixel of the last trip)."""
    ho, wo = out_hw(case)
    total = case.n * ho * wo * (case.cout // 4)
    blocks = min(_ceil(total, 256), 2048)
    trips = _ceil(total, 256 * blocks)
    return Trips(total, None, blocks, 256 * blocks, trips, (trips - 1) * 256 * blocks * 4 // case.cout)


def last_trip_values(case, mode, o):
    """the elements of the result o (NCHW) that the LAST trip of the case's size-driven loop writes (every channel of the pixels from
    last_start on): if they were all zero, a launch that never made the trip could still equal the reference on a zeroed buffer"""
    t = small_trips(case, mode) if case.splits == 0 else reduce_trips(case, mode)
    n, _, h, w = o.shape
    pix = torch.arange(t.last_start, n * h * w)
    return o[pix // (h * w), :, (pix // w) % h, pix % w]


def last_split_mask(case, mode):
    """[k, k, cin] of 0 / 1: zero on the K steps of the LAST split of a forced-split launch.  conv_igemm_kernel walks K tap by tap (steps of
    one granule inside a tap); conv_pp_kernel walks it chunk by chunk (one granule, all nine taps)."""
    cin, g, k = case.c1 + case.c2, GRANULE[mode], case.k
    splits, per = effective_splits(case, mode)
    mask = torch.ones(k, k, cin)
    if case.form == 'pp_splitk':
        mask[:, :, (splits - 1) * (per // 9) * g:] = 0
    else:
        spt = cin // g
        for ks in range((splits - 1) * per, k * k * spt):
            tap, ci = divmod(ks, spt)
            mask[tap // k, tap % k, ci * g:(ci + 1) * g] = 0
    return mask


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _sparse(gen, shape, density, values):
    v = torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), shape, generator=gen)]
    return v * (torch.rand(shape, generator=gen, dtype=torch.float64) < density)


def _ints(gen, shape, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def exact_inputs(case, mode, seed=0, variant='int'):
    """The seeded inputs of a case as float64 NCHW / OIHW tensors (a dict of conv_ref64's arguments, plus `bias_nc_wide` [n, 2*cout] where
    bias_nc is its right half).  Activations {0, +-1, +-2} and weights {0, +-1} with equal densities d, d^2 = 32 / K (K = k*k*cin): about
    32 nonzero products reach each output.  (A fused GroupNorm's b != 0 makes every activation nonzero: those cases take the weights at
    24 / K alone.)  Variants, F32 and F16X3 only: x_lo adds b * 2^-13, b in {0, +-1}, to the activations (the hi part stays the integer,
    the lo plane carries b); w_lo adds d * 2^-12 to the weights."""
    case = CASES[case] if isinstance(case, str) else case
    assert variant == 'int' or mode in W32, 'the lo-plane variants are the float32-activation modes\''
    gen = torch.Generator().manual_seed(1000 * seed + sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)) % 100003)
    n, h, w, k = case.n, case.h, case.w, case.k
    cin, cout = case.c1 + case.c2, case.cout
    ho, wo = out_hw(case)
    K = k * k * cin
    d = min(1.0, math.sqrt(32.0 / K))
    dx, dw = (d, min(1.0, 24.0 / K)) if case.gn else (d, d)
    x = _sparse(gen, (n, cin, h, w), dx, [1, -1, 2, -2])
    wt = _sparse(gen, (cout, cin, k, k), dw, [1, -1])
    if variant == 'x_lo':
        x = x + _sparse(gen, x.shape, 0.5, [1, -1]) * 2.0 ** -13
    if variant == 'w_lo':
        wt = wt + _sparse(gen, wt.shape, d, [1, -1]) * 2.0 ** -12
    a = dict(x1=x[:, :case.c1].contiguous(), x2=x[:, case.c1:].contiguous() if case.c2 else None, w=wt, bias=None, bias_nc=None, residual=None,
             up=case.up, out_scale=case.scale, gn=None, skip=None)
    if 'b' in case.ep or 'B' in case.ep:
        a['bias'] = _ints(gen, (cout,))
    if 'n' in case.ep:
        a['bias_nc'] = _ints(gen, (n, cout))
    if 'N' in case.ep:
        a['bias_nc_wide'] = _ints(gen, (n, 2 * cout))
        a['bias_nc'] = a['bias_nc_wide'][:, cout:]
    if 'r' in case.ep:
        a['residual'] = _ints(gen, (n, cout, ho, wo))
    if case.gn:
        a['gn'] = (torch.tensor([1.0, 2.0, -1.0], dtype=torch.float64)[torch.randint(0, 3, (n, cin), generator=gen)],
                   _ints(gen, (n, cin), -1, 1), False)
    if case.skip is not None:
        cs, s_up, unit = (tuple(case.skip) + (2.0 ** -6,))[:3]
        ds = min(1.0, math.sqrt(8.0 / cs))
        a['skip'] = (_sparse(gen, (n, cs, h // 2 if s_up else h, w // 2 if s_up else w), ds, [1, -1, 2, -2]),
                     _sparse(gen, (cout, cs, 1, 1), ds, [1, -1]) * unit, s_up)
    return a


def reference(args):
    """conv_ref64 of an exact_inputs() dict"""
    return conv_ref64(*(args[k] for k in ('x1', 'x2', 'w', 'bias', 'bias_nc', 'residual', 'up', 'out_scale')), gn=args['gn'], skip=args['skip'])


def representable(t, dtype):
    return torch.equal(t.to(dtype).double(), t.double())


def assert_exact_conditions(ref, dtype, stats=None, args=None):
    """The conditions under which a kernel's result must EQUAL ref.o: max S <= 256 (every value a kernel can form is a multiple of 2^-14
    below 2^8: exact in f32 in any order) and o representable in the storage type `dtype`; `stats` (strip or image moments of o, emitted
    as float32) representable in float32; `args`: the operands themselves representable in `dtype` (weights, activations, bias_nc,
    residual) or float32 (bias).  Asserted, never skipped."""
    assert float(ref.S.max()) <= 256.0, f'max S = {float(ref.S.max())}'
    assert representable(ref.o, dtype), 'the result is not representable in the output type'
    assert bool(((ref.o * 2.0 ** 14) == (ref.o * 2.0 ** 14).round()).all())
    if stats is not None:
        assert representable(stats, torch.float32) and float(stats.abs().max()) < 2.0 ** 24
    if args is not None:
        for name in ('x1', 'x2', 'w', 'bias_nc', 'residual'):
            assert args[name] is None or representable(args[name], dtype), name
        assert args['bias'] is None or representable(args['bias'], torch.float32)
        if args['gn'] is not None:
            x = torch.cat([args['x1']] + ([] if args['x2'] is None else [args['x2']]), 1)
            assert representable(norm_input(x, args['gn']), dtype)
        if args['skip'] is not None:
            assert representable(args['skip'][0], dtype) and representable(args['skip'][1], dtype)


# ---- Gaussian inputs of the rounding leg ---------------------------------------------------------------------------------------------
def gaussian_inputs(case, mode, seed=0):
    """the inputs of the older tests -- N(0, 1) activations, N(0, 1 / K) weights, N(0, 1) epilogue operands -- rounded to the storage type
    (bias stays float32), as float64 tensors in exact_inputs' layout; out_scale as the case says"""
    case = CASES[case] if isinstance(case, str) else case
    dt = STORE[mode]
    gen = torch.Generator().manual_seed(77 + seed)
    q = lambda t: t.to(dt).double()
    n, h, w, k, cin, cout = case.n, case.h, case.w, case.k, case.c1 + case.c2, case.cout
    ho, wo = out_hw(case)
    x = q(torch.randn(n, cin, h, w, generator=gen))
    a = dict(x1=x[:, :case.c1].contiguous(), x2=x[:, case.c1:].contiguous() if case.c2 else None,
             w=q(torch.randn(cout, cin, k, k, generator=gen) / math.sqrt(cin * k * k)), bias=None, bias_nc=None, residual=None, up=case.up,
             out_scale=0.70710678 if case.scale != 1.0 else 1.0, gn=None, skip=None)
    if 'b' in case.ep:
        a['bias'] = torch.randn(cout, generator=gen).double()
    if 'n' in case.ep or 'N' in case.ep:
        a['bias_nc_wide'] = q(torch.randn(n, 2 * cout, generator=gen))
        a['bias_nc'] = a['bias_nc_wide'][:, cout:]
    if 'r' in case.ep:
        a['residual'] = q(torch.randn(n, cout, ho, wo, generator=gen))
    if case.skip is not None:
        cs, s_up = case.skip[:2]
        a['skip'] = (q(torch.randn(n, cs, h // 2 if s_up else h, w // 2 if s_up else w, generator=gen)),
                     q(torch.randn(cout, cs, 1, 1, generator=gen) / math.sqrt(cs)), s_up)
    return a
