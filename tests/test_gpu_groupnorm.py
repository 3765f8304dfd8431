"""Every GroupNorm route and apply kernel (csrc/groupnorm.hip, ops.group_norm) against ONE float64 reference written from the definition
(tests/gn_reference.py), on the networks' own (channels, resolution) pairs, ragged pixel counts and statistics regimes up to and
beyond what the networks produce.

One error measure, err = max |got - ref64| / max |ref64|, and one bound:

    err(kernel) < K * max(e_ref32, 1e-7) * max(1, r^2)              K = 4

e_ref32 is the error of the reference's own float32 arithmetic (oracle.edm_nets.group_norm ...) on the same input, computed here on
the CPU; r is the |mean| / std the input was built with, and max(1, r^2) the known cost of a one-pass variance E[x^2] - mean^2.
16-bit storage adds 1.01 ulp of the storage type at max |ref64|, a split-precision image 2^-22.  Every case prints err, e_ref32 and
ratio = err / (max(e_ref32, 1e-7) * max(1, r^2)), which the bound holds below K.  The inputs are proven fair on the CPU by
tests/test_groupnorm_reference.py."""
import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

import launch_rules as LR
from gn_reference import FLOOR, K, REGIMES, bound, err, gn_ref64, groups_of, ref32, regime_input

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TOL = {torch.bfloat16: 2.5e-2, torch.float16: 4e-3}          # test_gpu_ops.TOL: conv results in 16-bit storage
ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTN = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


def q(x, dtype):
    """round-trip through the storage dtype so the reference sees the stored values"""
    return x.to(dtype).to(torch.float32)


def nhwc(x, dtype=torch.float32):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV, dtype)


def nchw64(y):
    return y.float().cpu().permute(0, 3, 1, 2).double()


def strip_stats(x, perm=None):
    """what a producing convolution attaches: per 64 consecutive pixels (NHWC order) and channel, (sum, sum of squares) -- in float64
    on the CPU, rounded to float32.  perm: a permutation of the strips within each sample."""
    n, c, h, w = x.shape
    v = x.double().permute(0, 2, 3, 1).reshape(n, (h * w) // 64, 64, c)
    st = torch.stack([v.sum(2), (v * v).sum(2)], dim=-1)
    if perm is not None:
        st = st[:, perm]
    return st.reshape(n * ((h * w) // 64), c, 2).float().to(DEV)


def split_value(img):
    """hi + lo * 2^-11 of a SplitAct, float64 NCHW"""
    hi, lo = img.planes()
    return nchw64(hi).double() + nchw64(lo).double() / 2048.0


class Case:
    def __init__(self, regime, n, c1, c2, h, w, adm=True, silu=True, dtype=torch.float32, groups=None, seed=None):
        c = c1 + c2
        self.n, self.c1, self.c2, self.c, self.h, self.w, self.dtype, self.silu, self.regime = n, c1, c2, c, h, w, dtype, silu, regime
        self.groups = groups or groups_of(c)
        self.eps = 1e-5 if adm else 1e-6                  # ADM / DDPM++ (networks.py)
        seed = seed if seed is not None else 7 * c + h * w + n
        base = regime if regime in REGIMES else 'centred'
        x, self.r = regime_input(base, n, c, h, w, seed)
        cg = c // self.groups
        if regime == 'constant':
            x[n - 1, 3 * cg:4 * cg] = 3.0
        if regime == 'constant3000':
            x[n - 1, 3 * cg:4 * cg] = 3000.0
            self.eps = 1e-6
        if regime == 'dead_row':
            x[n - 1] = 0.0
        x = q(x, dtype)
        self.x1, self.x2 = x[:, :c1].contiguous(), (x[:, c1:].contiguous() if c2 else None)
        gen = torch.Generator().manual_seed(seed + 1)
        self.gamma, self.beta = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
        self.ss = q(torch.randn(n, 2 * c, generator=gen) * 0.3, dtype) if adm else None        # adaptive scale / shift: ADM only
        self.label = f'{regime} {c1}+{c2}x{h}x{w} n={n} {DTN[dtype]}'
        self._refs = {}

    def ref(self, pool=False, plain=False):
        """(ref64, a64, b64, e_ref32); plain: no scale/shift, no SiLU"""
        if (pool, plain) not in self._refs:
            self._refs[(pool, plain)] = self._ref(pool, plain)
        return self._refs[(pool, plain)]

    def _ref(self, pool, plain):
        ss, silu = (None, False) if plain else (self.ss, self.silu)
        y, a, b = gn_ref64(self.x1, self.x2, self.groups, self.eps, self.gamma, self.beta, ss, silu, pool)
        assert self.groups == groups_of(self.c)
        e32 = err(ref32(self.x1, self.x2, self.eps, self.gamma, self.beta, ss, silu, pool), y)
        return y, a, b, e32

    def xmax(self):
        return float(max(self.x1.abs().max(), 0.0 if self.x2 is None else self.x2.abs().max()))


@functools.lru_cache(maxsize=3)
def case(*a, **kw):
    return Case(*a, **kw)


def routes_for(c1, c2, h, w, pool=False):
    """the routes that accept a shape, spelled out so that a missing route is visible here and not as a skip"""
    cg = (c1 + c2) // groups_of(c1 + c2)
    rt = ['split']
    if not pool and cg % 2 == 0 and cg <= 64 and c1 % 2 == 0:
        rt.append('fused')
    if (h * w) % 64 == 0 and cg <= 128:
        rt.append('strips')
    return rt


def run(ops, cs, route, pool=False, plain=False, **kw):
    """-> (output, coef or None) of one route"""
    x1d, x2d = nhwc(cs.x1, cs.dtype), (None if cs.x2 is None else nhwc(cs.x2, cs.dtype))
    g, b = cs.gamma.to(DEV), cs.beta.to(DEV)
    ss = None if (cs.ss is None or plain) else cs.ss.to(DEV, cs.dtype)
    silu = cs.silu and not plain
    if route == 'split':
        coef = ops.gn_coef(x1d, cs.groups, cs.eps, g, b, x2=x2d, scale_shift=ss)
        return ops.gn_apply(x1d, coef, x2=x2d, silu=silu, pool=pool, **kw), coef
    if route == 'fused':
        return ops.group_norm(x1d, cs.groups, cs.eps, g, b, x2=x2d, scale_shift=ss, silu=silu, pool=pool, path='fused', **kw), None
    assert route == 'strips'
    x1d._gn_stats = strip_stats(cs.x1)
    if x2d is not None:
        x2d._gn_stats = strip_stats(cs.x2)
    coef = ops._coef_from_strips(x1d, x2d, cs.groups, cs.eps, g, b, ss)
    assert coef is not None
    return ops.group_norm(x1d, cs.groups, cs.eps, g, b, x2=x2d, scale_shift=ss, silu=silu, pool=pool, path='strips', **kw), coef


def report(label, e, e32, r, limit):
    ratio = e / (max(e32, FLOOR) * max(1.0, r * r))
    fn = os.environ.get('PYTEST_CURRENT_TEST', '').split('::')[-1].split('[')[0]
    print(f'\n  [{fn}] {label}: err {e:.3e}  e_ref32 {e32:.3e}  err/e_ref32 {e / max(e32, 1e-30):.2f}  ratio {ratio:.2f} (K = {K})')
    assert e < limit, (label, e, e32, ratio)
    return ratio


def check_out(cs, route, got64, ref, extra=0.0, what='out'):
    y, _, _, e32 = ref
    return report(f'{route} {cs.label} {what}', err(got64, y), e32, cs.r, bound(e32, cs.r, extra + 1.01 * ULP[cs.dtype]))


def check_coef(cs, route, coef, ref):
    """the coefficients alone (statistics, not apply): max |a - a64| / max |a64| and max |b - b64| / max(|b64|, |a64| max|x|)"""
    _, a64, b64, e32 = ref
    co = coef.cpu().double()
    ea = float((co[..., 0] - a64).abs().max() / a64.abs().max())
    eb = float((co[..., 1] - b64).abs().max() / max(float(b64.abs().max()), float(a64.abs().max()) * cs.xmax()))
    report(f'{route} {cs.label} coef a', ea, e32, cs.r, bound(e32, cs.r))
    report(f'{route} {cs.label} coef b', eb, e32, cs.r, bound(e32, cs.r))


def check_route(ops, cs, route, pool=False):
    ref = cs.ref(pool)
    out, coef = run(ops, cs, route, pool=pool)
    assert tuple(out.shape) == (cs.n, cs.h // 2 if pool else cs.h, cs.w // 2 if pool else cs.w, cs.c) and out.dtype == cs.dtype
    if coef is not None:
        check_coef(cs, route, coef, ref)
    return check_out(cs, route, nchw64(out), ref)


# ---- statistics regimes on four network shapes, every route ----------------------------------------------------------------------
# (c1, c2, res, adm): ADM's narrowest level at both ends, its widest concat, a DDPM++ level (eps 1e-6, no scale/shift)
REGIME_SHAPES = [(192, 0, 8, True), (192, 0, 64, True), (768, 576, 8, True), (256, 0, 16, False)]
REGIME_CASES = [(rg, s, rt) for s in REGIME_SHAPES for rg in REGIMES for rt in routes_for(s[0], s[1], s[2], s[2])]


@pytest.mark.parametrize('regime,shape,route', REGIME_CASES, ids=[f'{rg}-{s[0]}+{s[1]}x{s[2]}-{rt}' for rg, s, rt in REGIME_CASES])
def test_every_route_in_every_statistics_regime(ops, regime, shape, route):
    """float32, all routes against gn_ref64, coefficients and outputs.  offset4 / offset16 are the characterisation of the one-pass
    variance: they hold only through the max(1, r^2) factor.
    Largest ratio measured on an MI355X: 1.31 (centred / large); per route in the network regime: split 1.49, fused 1.18, strips 1.18; at offset16
    0.07 / 0.04 / 0.06 (err / e_ref32 about 18 / 10 / 15, against the r^2 = 256 the bound allows); at offset4 0.29 / 0.09 / 0.12."""
    c1, c2, res, adm = shape
    check_route(ops, case(regime, 2, c1, c2, res, res, adm), route)


# ---- the network regime on every (C, resolution) pair of the networks ----------------------------------------------------------
ADM_SHAPES = [(192, 0, 32), (192, 0, 64), (384, 0, 16), (384, 0, 32), (192, 192, 64), (576, 0, 8), (576, 0, 16), (384, 192, 32), (384, 192, 64),
              (768, 0, 8), (768, 0, 16), (384, 384, 32), (576, 384, 16), (576, 384, 32), (576, 576, 16), (768, 576, 8), (768, 576, 16), (768, 768, 8)]
DDPMPP_SHAPES = [(128, 0, 32), (256, 0, 8), (256, 0, 16), (256, 0, 32), (256, 128, 32), (256, 256, 8), (256, 256, 16), (256, 256, 32)]
# (n, c1, c2, h, w, adm): n = 2, or 1 where 2 would exceed 2 x 192 x 64 x 64 elements (the float64 reference stays cheap)
NET_SHAPES = [(2 if 2 * (a + b) * r * r <= 2 * 192 * 64 * 64 else 1, a, b, r, r, True) for a, b, r in ADM_SHAPES] + \
             [(2, a, b, r, r, False) for a, b, r in DDPMPP_SHAPES]
OTHER_SHAPES = [
    (2, 128, 0, 16, 16, False), (2, 256, 0, 8, 8, True), (2, 512, 0, 8, 8, False), (2, 64, 0, 16, 16, True),   # classifier / VAE widths; C = 64: 16 groups
    (2, 192, 0, 5, 7, True), (2, 192, 0, 6, 10, True), (2, 960, 0, 1, 1, True), (2, 384, 0, 4, 4, False), (5, 192, 0, 3, 64, True),    # ragged pixel counts
    (2, 576, 384, 5, 7, True), (3, 1344, 0, 6, 10, False),
    (2, 1536, 0, 6, 10, True),            # 384 chunks per row: the grid-stride apply kernel
    (2, 1024, 0, 6, 10, False),           # 256 chunks per row: the largest row kernel
    (2, 656, 656, 16, 16, True),          # 41 channels per group: where float32 e * (1 / cg) falls below the integer at e = k * cg (the strip index's + 0.5f)
]
NETWORK_CASES = [(i, s, rt) for i, s in enumerate(NET_SHAPES + OTHER_SHAPES) for rt in routes_for(s[1], s[2], s[3], s[4])]


def _sid(s):
    return f'n{s[0]}-{s[1]}+{s[2]}x{s[3]}x{s[4]}-' + ('adm' if s[5] else 'ddpmpp')


@pytest.mark.parametrize('i,shape,route', NETWORK_CASES, ids=[f'{_sid(s)}-{rt}' for _, s, rt in NETWORK_CASES])
def test_network_regime_on_every_network_shape(ops, i, shape, route):
    """float32, |mean| / std = 1.2 (measured in the networks: <= 1.14), std 0.15 or 3.0 (both ends of the measured range, alternating over
    the shapes).  Every shape runs `split`, and test-built `strips` where the pixel count is a multiple of 64.
    Largest ratio measured on an MI355X: 1.25."""
    n, c1, c2, h, w, adm = shape
    check_route(ops, case('network_lo' if i % 2 else 'network_hi', n, c1, c2, h, w, adm), route)


POOL_SHAPES = [(2, 192, 0, 64, 64, True), (2, 384, 0, 32, 32, True), (2, 576, 0, 16, 16, True), (2, 256, 0, 32, 32, False), (2, 192, 0, 6, 10, True),
               (2, 1536, 0, 6, 10, True)]


POOL_CASES = [(s, rt) for s in POOL_SHAPES for rt in routes_for(s[1], s[2], s[3], s[4], pool=True)]


@pytest.mark.parametrize('shape,route', POOL_CASES, ids=[f'{_sid(s)}-{rt}' for s, rt in POOL_CASES])
def test_pooled_apply(ops, shape, route):
    """GroupNorm + SiLU + 2x2 average (the down blocks), coefficients from both statistics routes
    Largest ratio measured on an MI355X: 0.86."""
    n, c1, c2, h, w, adm = shape
    check_route(ops, case('network_hi', n, c1, c2, h, w, adm), route, pool=True)


# ---- 16-bit storage ----------------------------------------------------------------------------------------------------------
# one shape per channels-per-group value 6, 12, 18, 24, 30, 42 (with 30 and 42 a 16-byte chunk of 8 channels straddles two groups)
SHAPES16 = [(2, 192, 0, 8, 8, True), (2, 384, 0, 16, 16, True), (2, 576, 0, 8, 8, True), (2, 768, 0, 8, 8, True), (2, 576, 384, 16, 16, True),
            (2, 768, 576, 8, 8, True)]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('shape', SHAPES16, ids=_sid)
@pytest.mark.parametrize('route', ['split', 'fused', 'strips', 'pool'])
def test_16_bit_storage(ops, dtype, shape, route):
    """bf16 / f16 tensors, network regime: err < 1.01 ulp of the storage type + the float32 bound; the coefficients (float32 from the
    stored values) under the float32 bound itself
    Largest ratio measured on an MI355X: 0.92 (coefficients)."""
    n, c1, c2, h, w, adm = shape
    cs = case('network_hi', n, c1, c2, h, w, adm, dtype=dtype)
    check_route(ops, cs, 'split' if route == 'pool' else route, pool=route == 'pool')


# ---- split-precision outputs ---------------------------------------------------------------------------------------------------
SPLIT_SHAPES = [(2, 192, 0, 64, 64, True), (2, 768, 576, 8, 8, True), (2, 576, 384, 16, 16, True), (2, 256, 128, 32, 32, False), (2, 192, 0, 5, 7, True),
                (5, 192, 0, 3, 64, True), (2, 1536, 0, 6, 10, True), (2, 64, 0, 16, 16, True),
                (2, 772, 572, 6, 10, True)]       # c1 % 8 != 0: the 8-byte-store form whatever the knob says (a lane pair would straddle the concat)


@pytest.mark.parametrize('shape', SPLIT_SHAPES, ids=_sid)
@pytest.mark.parametrize('form', ['default', 'gn_fuse2'])
@pytest.mark.parametrize('pool', [False, True], ids=['plain', 'pool'])
def test_split_precision_output_is_the_normalised_tensor(ops, shape, form, pool):
    """split_out=True / raw_split=True (dts_gn_apply_x3): hi + lo * 2^-11 of the image against gn_ref64 (not against the product's own
    float32 pass): the float32 bound + 2^-22 (dts.h: the pair carries about 22 bits); the raw image reconstructs the un-normalised input
    (2x2-averaged in float64 when pooled) to 2^-22 * max |x|.  Both store forms: 16-byte lane-pair stores (default) and gn_fuse = 2.
    Largest ratio measured on an MI355X: 1.49."""
    n, c1, c2, h, w, adm = shape
    if pool and (h % 2 or w % 2):
        h, w = h + h % 2, w + w % 2                     # (5 x 7 -> 6 x 8)
    check_split_images(ops, case('network_lo', n, c1, c2, h, w, adm), form, pool)


def check_split_images(ops, cs, form, pool):
    """the checks of test_split_precision_output_is_the_normalised_tensor on one case: -> the largest ratio of the split images"""
    from diffusion_tts_amd import _lib
    n, c1, c2, h, w = cs.n, cs.c1, cs.c2, cs.h, cs.w
    ref = cs.ref(pool)
    worst = 0.0
    if form == 'gn_fuse2':
        _lib.set_tuning('gn_fuse', 2)
    try:
        for route in [r for r in routes_for(c1, c2, h, w, pool) if r != 'fused']:            # (the fused kernel has no split output)
            (img, raw), coef = run(ops, cs, route, pool=pool, split_out=True, raw_split=True)
            only, _ = run(ops, cs, route, pool=pool, split_out=True)
            assert isinstance(img, ops.SplitAct) and tuple(img.shape) == tuple(ref[0].permute(0, 2, 3, 1).shape)
            assert torch.equal(only.data, img.data)
            worst = max(worst, check_out(cs, route, split_value(img), ref, extra=2.0 ** -22, what=f'split image ({form})'))
            x = (cs.x1 if cs.x2 is None else torch.cat([cs.x1, cs.x2], 1)).double()
            if pool:
                x = x.reshape(n, cs.c, h // 2, 2, w // 2, 2).sum((3, 5)) / 4.0
            eraw = float((split_value(raw) - x).abs().max()) / cs.xmax()
            print(f'  raw image: max |hi + lo/2048 - x| / max |x| = {eraw:.3e} (2^-22 = {2.0 ** -22:.3e})')
            assert eraw <= 2.0 ** -22
    finally:
        _lib.set_tuning('gn_fuse', -1)
    return worst


# ---- the second trip of the apply kernels' size-driven loops -----------------------------------------------------------------------------
# At every shape above, a thread of gn_apply_rows_kernel makes ONE pair trip (n * hw <= 4096 * 2k) and a thread of gn_apply_kernel ONE
# grid-stride trip (at most 98304 threads' worth against 4096 * 256).  launch_rules.gn_apply_plan restates gn_apply_impl; each case below
# asserts which kernel serves it and the trips it makes before it runs (tests/test_launch_rules.py asserts the same without a GPU).
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}


def _sized(table, name, dt, **kw):
    """the Case of a launch_rules entry, after asserting that the restated launcher sends it where the entry says"""
    e = table[name]
    plan = LR.gn_apply_plan(e.n, e.c1, e.c2, e.h, e.w, dt == 'f32', e.pool, **kw)
    for field, want in e.expect.items():
        assert getattr(plan, field) == want, (name, field, plan)
    assert plan.trips == 2
    return case('network_lo', e.n, e.c1, e.c2, e.h, e.w, True, dtype=DT[dt]), plan


ROWS_CASES = [(name, dt) for name, e in LR.GN_ROWS_TWO_TRIPS.items() for dt in e.dtypes]


@pytest.mark.parametrize('name,dt', ROWS_CASES, ids=[f'{n}-{d}' for n, d in ROWS_CASES])
def test_row_apply_second_pair_trip(ops, name, dt):
    """gn_apply_rows_kernel where every thread makes TWO pair trips (the stride p += 2k) at k = 1, 3 and 5 pixels per block pass, and the
    ragged last block of a sample: one pair and the single-pixel tail (k = 1), a pair for every pixel row and the tail for two (k = 5).
    Largest ratio measured on an MI355X: 1.03 (coefficient a of the bf16 case; outputs: 0.50 at k = 1, 0.73 at k = 5)."""
    cs, plan = _sized(LR.GN_ROWS_TWO_TRIPS, name, dt)
    assert plan.kernel == 'rows'
    check_route(ops, cs, 'split')


@pytest.mark.parametrize('name,form', [('c192', 'default'), ('c192', 'gn_fuse2'), ('c100+92', 'default')])
def test_row_apply_second_pair_trip_split_images(ops, name, form):
    """the same loop in the split-image instantiations, normalised and raw image: <float, SPLIT, W16> (16-byte lane-pair stores), <float,
    SPLIT> under gn_fuse = 2, and <float, SPLIT> because c1 % 8 != 0 (a lane pair would straddle the concat).
    Largest ratio measured on an MI355X: 0.99 (all three forms give the same image)."""
    cs, plan = _sized(LR.GN_ROWS_TWO_TRIPS, name, 'f32', split=True, gn_fuse=2 if form == 'gn_fuse2' else -1)
    assert plan.kernel == 'rows' and plan.w16 == (name == 'c192' and form == 'default')
    check_split_images(ops, cs, form, False)


GRID_CASES = [(name, dt) for name, e in LR.GN_GRID_TWO_TRIPS.items() for dt in e.dtypes]


@pytest.mark.parametrize('name,dt', GRID_CASES, ids=[f'{n}-{d}' for n, d in GRID_CASES])
def test_grid_stride_apply_second_trip(ops, name, dt):
    """gn_apply_kernel past its cap of 4096 blocks x 256 threads by less than a block: the threads of the first blocks take a second trip
    (idx += gridDim.x * blockDim.x), pooled (<T, true>) in all three types and unpooled (<float, false>: 384 chunks per row).
    Largest ratio measured on an MI355X: 0.95 (coefficient a of the bf16 case; float32 outputs: 0.46 pooled, 0.50 unpooled)."""
    cs, plan = _sized(LR.GN_GRID_TWO_TRIPS, name, dt)
    assert plan.kernel == 'grid' and 0 < plan.threads - 4096 * 256 < 256
    check_route(ops, cs, 'split', pool=LR.GN_GRID_TWO_TRIPS[name].pool)


@pytest.mark.parametrize('name', ['pool_f32', 'wide_f32'])
def test_grid_stride_apply_second_trip_split_images(ops, name):
    """the same as split images: gn_apply_kernel<float, true, true> and <float, false, true>.
    Largest ratio measured on an MI355X: 0.68 (unpooled; pooled 0.51)."""
    cs, plan = _sized(LR.GN_GRID_TWO_TRIPS, name, 'f32', split=True)
    assert plan.kernel == 'grid'
    check_split_images(ops, cs, 'default', LR.GN_GRID_TWO_TRIPS[name].pool)


# ---- exact cases ---------------------------------------------------------------------------------------------------------------
EXACT_SHAPES = REGIME_SHAPES


@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=lambda s: f'{s[0]}+{s[1]}x{s[2]}')
def test_dead_row(ops, shape):
    """an all-zero sample (a dead candidate): sums of zeros are exact, so without scale/shift and SiLU every output equals beta[c] BIT FOR
    BIT on every route, b == beta bit for bit and a is finite; with scale/shift and SiLU the outputs sit within 4 * 2^-23 (relative, the
    one error measure) of act(beta * (1 + scale) + shift) in float64 (fma contraction, the sigmoid's last ulp).
    Largest ratio measured on an MI355X: 1.48."""
    c1, c2, res, adm = shape
    cs = case('dead_row', 2, c1, c2, res, res, adm)
    want = cs.beta[None, None, :].expand(res, res, cs.c)
    for route in routes_for(c1, c2, res, res):
        out, coef = run(ops, cs, route, plain=True)
        assert torch.equal(out[1].cpu(), want), (route, float((out[1].cpu() - want).abs().max()))
        if coef is not None:
            assert torch.equal(coef[1, :, 1].cpu(), cs.beta) and bool(torch.isfinite(coef).all()), route
        if route != 'fused':
            img, _ = run(ops, cs, route, plain=True, split_out=True)
            assert float((split_value(img)[1] - want.permute(2, 0, 1).double()).abs().max()) <= 2.0 ** -22 * float(cs.beta.abs().max())
        check_out(cs, route, nchw64(out), cs.ref(plain=True), what='whole tensor (plain)')
        out, _ = run(ops, cs, route)
        y = cs.ref()[0]
        e = err(nchw64(out)[1], y[1])
        print(f'  {route} {cs.label}: dead row with scale/shift + SiLU: err {e:.3e} (4 * 2^-23 = {4 * 2.0 ** -23:.3e})')
        assert e < 4 * 2.0 ** -23, (route, e)
        check_out(cs, route, nchw64(out), cs.ref(), what='whole tensor')


@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=lambda s: f'{s[0]}+{s[1]}x{s[2]}')
@pytest.mark.parametrize('regime', ['constant', 'constant3000'])
def test_constant_group(ops, shape, regime):
    """one group of one sample is a constant: 3.0, and 3000.0 at eps = 1e-6, where E[x^2] - mean^2 of float32 sums can go negative (the
    `var < 0` clamp).  Everything finite; the group's outputs within K * max(e_ref32, 1e-7) (of max |ref64|) + value * |a| * 2^-23 of
    ref64 (the mean of a constant is not exact in float32 sums, and rstd = 1 / sqrt(eps) multiplies what is left)."""
    c1, c2, res, adm = shape
    value = 3.0 if regime == 'constant' else 3000.0
    cs = case(regime, 2, c1, c2, res, res, adm)
    y, a64, b64, e32 = cs.ref(plain=True)
    cg = cs.c // cs.groups
    sl = slice(3 * cg, 4 * cg)
    limit = K * max(e32, FLOOR) * float(y.abs().max()) + value * float(a64[1, sl].abs().max()) * 2.0 ** -23
    for route in routes_for(c1, c2, res, res):
        out, coef = run(ops, cs, route, plain=True)
        assert bool(torch.isfinite(out).all()) and (coef is None or bool(torch.isfinite(coef).all())), route
        d = float((nchw64(out)[1, sl] - y[1, sl]).abs().max())
        print(f'  {route} {cs.label}: constant group |out - ref64| = {d:.3e} (limit {limit:.3e}); e_ref32 {e32:.3e}')
        assert d <= limit, (route, d, limit)
        full, _ = run(ops, cs, route)
        assert bool(torch.isfinite(full).all()), route
        # the other groups and the other sample are ordinary centred data.  (err's denominator is max |ref64| of what is compared.)
        e0 = err(nchw64(out)[0], y[0])
        assert e0 < bound(e32, cs.r), (route, e0)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_identical_rows_give_identical_bits(ops, dtype):
    """the header of groupnorm.hip promises fixed-order sums: the same row at five batch positions gives the same bits on every route
    (ties between candidates stay ties), plain, pooled and as a split image"""
    for (c1, c2, h, w) in ((192, 0, 3, 64), (768, 576, 8, 8), (192, 0, 64, 64)):
        one = Case('network_hi', 1, c1, c2, h, w, dtype=dtype)
        cs = Case('network_hi', 5, c1, c2, h, w, dtype=dtype)
        cs.x1 = one.x1.repeat(5, 1, 1, 1)
        cs.x2 = None if c2 == 0 else one.x2.repeat(5, 1, 1, 1)
        cs.ss = cs.ss[:1].repeat(5, 1)
        for route in routes_for(c1, c2, h, w):
            out, coef = run(ops, cs, route)
            for i in range(1, 5):
                assert torch.equal(out[0], out[i]), (route, c1, c2, h, w, i)
                assert coef is None or torch.equal(coef[0], coef[i])
            if route != 'fused' and dtype == torch.float32:
                img, _ = run(ops, cs, route, split_out=True, pool=h % 2 == 0)
                for i in range(1, 5):
                    assert torch.equal(img.data[0], img.data[i]), (route, 'split', i)


# ---- strip statistics: the two block forms, concat, VAE sizes --------------------------------------------------------------------
@pytest.mark.parametrize('n,c1,c2,res', [(1, 128, 0, 256), (1, 512, 0, 128), (2, 128, 0, 64), (2, 256, 256, 64), (1, 64, 64, 256),
                                         (2, 656, 656, 16), (2, 976, 976, 16)],
                         ids=['128x256', '512x128', '128x64', '256+256x64', '64+64x256', '656+656x16', '976+976x16'])
def test_strip_coefficients_at_vae_size(ops, n, c1, c2, res):
    """gn_coef_strips_kernel alone, statistics built here: > 4096 strip-channel elements per group (128 channels at 256 x 256: 16384: the
    four-wave form; the float strip index (int)((e + 0.5f) * inv_cg)), against gn_ref64's coefficients; and the strips of a sample in
    another order give the same coefficients to 1e-6 (a sum does not depend on which pixels make a strip): catches an index that reads the
    wrong strip or channel.  41 and 61 channels per group (no network has them; the entry point takes up to 128) are where the index needs
    its + 0.5f: float32 e * (1 / cg) lands below the integer at multiples of cg; a concat, so that a wrong index stays inside the tensors.
    Largest ratio measured on an MI355X: 0.44."""
    cs = case('network_hi', n, c1, c2, res, res, False)
    ref = cs.ref(plain=True)
    g, b = cs.gamma.to(DEV), cs.beta.to(DEV)
    strips = res * res // 64
    perm = torch.randperm(strips, generator=torch.Generator().manual_seed(5))
    coefs = []
    for p1, p2 in ((None, None), (perm, perm.flip(0))):
        x1d = torch.empty((n, res, res, c1), dtype=torch.float32, device=DEV)
        x1d._gn_stats = strip_stats(cs.x1, p1)
        x2d = None
        if c2:
            x2d = torch.empty((n, res, res, c2), dtype=torch.float32, device=DEV)
            x2d._gn_stats = strip_stats(cs.x2, p2)
        coef = ops._coef_from_strips(x1d, x2d, cs.groups, cs.eps, g, b, None)
        assert coef is not None
        coefs.append(coef.cpu().double())
    check_coef(cs, 'strips', coefs[0], ref)
    d = float(((coefs[0] - coefs[1]).abs() / coefs[0].abs().clamp_min(1e-3 * float(coefs[0].abs().max()))).max())
    print(f'  permuted strips: max relative coefficient change {d:.3e}')
    assert d < 1e-6


# ---- strip statistics from the producing convolutions ------------------------------------------------------------------------------
PRODUCERS = ['igemm_4_waves', 'igemm_8_waves', 'ping_pong_192', 'ping_pong_128', 'split_k_reduce', 'folded_skip']


@pytest.mark.parametrize('producer', PRODUCERS)
def test_strip_statistics_from_each_producing_convolution(ops, producer):
    """path='strips' on the statistics a split-precision convolution's epilogue emitted, one case per producer.  ref64 is GroupNorm in
    float64 of the conv's STORED output read back from the GPU: the conv's own error is not charged to GroupNorm.  r is measured on that
    output in float64 (the largest |mean| / std over its groups).
    Largest ratio measured on an MI355X: 1.01 (ping-pong, 128-cout blocks)."""
    from diffusion_tts_amd import _lib
    gen = torch.Generator().manual_seed(17)
    n, res, c, cout, ks = 2, 16, 64, 128, 3
    knobs = {}
    if producer == 'igemm_4_waves':
        knobs = dict(conv_variant=0, conv_waves=4, conv_splits=1)
    if producer == 'igemm_8_waves':
        knobs = dict(conv_variant=0, conv_waves=8, conv_splits=1)
    if producer == 'ping_pong_192':
        n, res, c, cout, knobs = 2, 32, 128, 192, dict(conv_variant=1, conv_splits=1)
    if producer == 'ping_pong_128':
        n, res, c, cout, knobs = 2, 32, 64, 128, dict(conv_variant=1, conv_splits=1)
    if producer == 'split_k_reduce':
        n, res, c, cout, knobs = 2, 8, 256, 128, dict(conv_variant=0, conv_splits=2)
    if producer == 'folded_skip':
        n, res, c, cout, knobs = 2, 32, 192, 192, dict(conv_variant=1)
    x = torch.randn(n, c, res, res, generator=gen)
    wt = torch.randn(cout, c, ks, ks, generator=gen) / math.sqrt(c * ks * ks)
    bias = torch.randn(cout, generator=gen) * 1.2
    w3 = ops.pack_conv_weight(wt.to(DEV), ops.F16X3)
    xd = nhwc(x)
    for k, v in knobs.items():
        _lib.set_tuning(k, v)
    try:
        if producer.startswith('ping_pong'):
            assert ops.conv_kernel(xd, w3) == (6 if cout == 192 else 4)
        if producer.startswith('igemm') or producer == 'split_k_reduce':
            assert ops.conv_kernel(xd, w3) == 0
        if producer == 'folded_skip':
            src = torch.randn(n, 64, res, res, generator=gen)
            wsk = ops.pack_conv_weight((torch.randn(cout, 64, 1, 1, generator=gen) / 8).to(DEV), ops.F16X3)
            skip = (ops.SplitAct(ops.split3_f16(nhwc(src)), 64), wsk, False)
            hd = ops.SplitAct(ops.split3_f16(xd), c)
            assert ops.conv_folds_skip(hd, w3, skip)
            y = ops.conv2d(hd, w3, bias.to(DEV), skip=skip, out_scale=0.70710678, gn_stats=True)
        else:
            y = ops.conv2d(xd, w3, bias.to(DEV), gn_stats=True)
    finally:
        for k in knobs:
            _lib.set_tuning(k, -1)
    assert y._gn_stats is not None and tuple(y._gn_stats.shape) == (n * res * res // 64, cout, 2)
    cs = Case('centred', n, cout, 0, res, res, True)
    cs.x1 = y.cpu().permute(0, 3, 1, 2).contiguous()
    xg = cs.x1.double().reshape(n, cs.groups, -1)
    cs.r = float((xg.mean(2).abs() / xg.std(2)).max())
    cs.label = f'{producer} conv output {cout}x{res}x{res} (|mean|/std <= {cs.r:.2f})'
    ref = cs.ref()
    g, b, ss = cs.gamma.to(DEV), cs.beta.to(DEV), cs.ss.to(DEV)
    coef = ops._coef_from_strips(y, None, cs.groups, cs.eps, g, b, ss)
    assert coef is not None
    check_coef(cs, 'strips', coef, ref)
    out = ops.group_norm(y, cs.groups, cs.eps, g, b, scale_shift=ss, silu=True, path='strips')
    check_out(cs, 'strips', nchw64(out), ref)


# ---- GroupNorm applied inside the consuming convolution (16-bit) ---------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('regime', ['network_hi', 'offset4'])
@pytest.mark.parametrize('res,c1,c2,cout', [(16, 128, 0, 192), (32, 64, 128, 384)])
def test_conv_with_fused_group_norm_against_float64(ops, dtype, regime, res, c1, c2, cout):
    """conv2d(..., gn_coef=...) where conv_fuses_gn says yes (bit for bit apply + conv in test_gpu_ops): here against gn_ref64 followed by
    the float64 convolution, bound as there (TOL[dtype])
    Largest ratio measured on an MI355X: 0.64 (coefficients)."""
    from diffusion_tts_amd import _lib
    cs = case(regime, 2, c1, c2, res, res, True, dtype=dtype)
    gen = torch.Generator().manual_seed(23)
    wt = q(torch.randn(cout, cs.c, 3, 3, generator=gen) / math.sqrt(cs.c * 9), dtype)
    bias = torch.randn(cout, generator=gen)
    ref = F.conv2d(cs.ref()[0], wt.double(), bias.double(), padding=1)
    x1d, x2d = nhwc(cs.x1, dtype), (None if cs.x2 is None else nhwc(cs.x2, dtype))
    wp = ops.pack_conv_weight(wt.to(DEV), dtype)
    _lib.set_tuning('conv_variant', 1)
    try:
        assert ops.conv_fuses_gn(x1d, wp, x2=x2d)
        coef = ops.gn_coefficients(x1d, cs.groups, cs.eps, cs.gamma.to(DEV), cs.beta.to(DEV), x2=x2d, scale_shift=cs.ss.to(DEV, dtype))
        check_coef(cs, 'split', coef, cs.ref())
        out = ops.conv2d(x1d, wp, bias.to(DEV), x2=x2d, gn_coef=coef, gn_silu=True)
    finally:
        _lib.set_tuning('conv_variant', -1)
    e = err(nchw64(out), ref)
    print(f'  conv with fused GroupNorm {cs.label}: err {e:.3e} (TOL {TOL[dtype]:.1e})')
    assert e < TOL[dtype]


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(ops):
    """what a route does not take raises with a message instead of computing"""
    f32 = dict(dtype=torch.float32, device=DEV)
    g = lambda c: torch.ones(c, **f32)
    x = lambda c, h=8, w=8, n=1, dt=torch.float32: torch.zeros((n, h, w, c), dtype=dt, device=DEV)
    with pytest.raises(ValueError, match='fused GroupNorm needs'):
        ops.group_norm(x(96), 32, 1e-5, g(96), g(96), path='fused')                      # 3 channels per group: odd
    with pytest.raises(ValueError, match='fused GroupNorm needs'):
        ops.group_norm(x(256), 2, 1e-5, g(256), g(256), path='fused')                    # 128 channels per group
    with pytest.raises(ValueError, match='fused GroupNorm needs'):
        ops.group_norm(x(192), 32, 1e-5, g(192), g(192), path='fused', pool=True)
    out = x(256)
    for groups, c in ((32, 96), (2, 256)):                                                # the C entry point refuses them too
        with pytest.raises(RuntimeError, match='channels per group'):
            ops._call('dts_gn_fused', x(c).data_ptr(), c, None, 0, 0, 1, 64, groups, 1e-5, None, None, None, 0, out.data_ptr(), 1)
    st = torch.zeros((1, 512, 2), **f32)
    coef = torch.zeros((1, 512, 2), **f32)
    with pytest.raises(RuntimeError, match='dts_gn_coef_strips: hw=35'):
        ops._call('dts_gn_coef_strips', st.data_ptr(), 192, None, 0, 0, 1, 35, 32, 1e-5, None, None, None, 0, coef.data_ptr())
    with pytest.raises(RuntimeError, match='channels per group'):
        ops._call('dts_gn_coef_strips', st.data_ptr(), 512, None, 0, 0, 1, 64, 2, 1e-5, None, None, None, 0, coef.data_ptr())
    ragged = x(192, 5, 7)
    ragged._gn_stats = st
    with pytest.raises(ValueError, match='strip statistics are not attached'):            # 35 pixels: ops.py does not hand them over
        ops.group_norm(ragged, 32, 1e-5, g(192), g(192), path='strips')
    narrow = torch.zeros((1, 2 * 192 - 8), **f32)
    for path in ('split', 'fused'):
        with pytest.raises(RuntimeError, match='ld_ss'):
            ops.group_norm(x(192), 32, 1e-5, g(192), g(192), scale_shift=narrow, path=path)
    xs = x(192)
    xs._gn_stats = torch.zeros((1, 192, 2), **f32)
    with pytest.raises(RuntimeError, match='ld_ss'):
        ops.group_norm(xs, 32, 1e-5, g(192), g(192), scale_shift=narrow, path='strips')
    c48 = torch.zeros((1, 48, 2), **f32)
    with pytest.raises(RuntimeError, match='not a multiple of 32'):
        ops.gn_apply(x(48), c48, split_out=True)
    c192 = torch.zeros((1, 192, 2), **f32)
    for so in (False, True):
        with pytest.raises(RuntimeError, match='pool needs even'):
            ops.gn_apply(x(192, 5, 8), c192, pool=True, split_out=so)
        with pytest.raises(RuntimeError, match='pool needs even'):
            ops.gn_apply(x(192, 8, 7), c192, pool=True, split_out=so)
    # channel counts that are not a multiple of the 16-byte chunk: 4 float32 / 8 16-bit channels, on either side of a concat
    with pytest.raises(RuntimeError, match='unsupported'):
        ops.group_norm(x(6), 1, 1e-5, g(6), g(6), path='split')
    with pytest.raises(RuntimeError, match='unsupported'):
        ops.group_norm(x(36, dt=torch.bfloat16), 1, 1e-5, g(36), g(36), path='split')
    with pytest.raises(RuntimeError, match='unsupported'):
        ops.gn_apply(x(36, dt=torch.float16), torch.zeros((1, 36, 2), **f32))
    with pytest.raises(RuntimeError, match='unsupported'):
        ops.gn_apply(x(190), c192, x2=x(2))
    # empty tensors: n, h, w > 0 (valid pointers, so that it is the size check that answers)
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        with pytest.raises(RuntimeError, match='dts_gn_apply: n='):
            ops._call('dts_gn_apply', x(192).data_ptr(), 192, None, 0, 0, c192.data_ptr(), out.data_ptr(), n, h, w, 1, 0)
        with pytest.raises(RuntimeError, match='dts_gn_apply: n='):
            ops._call('dts_gn_apply_x3', x(192).data_ptr(), 192, None, 0, c192.data_ptr(), out.data_ptr(), None, n, h, w, 1, 0)

