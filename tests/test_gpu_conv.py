"""Every launch route of the convolutions (dts_conv2d: conv_igemm_kernel in its tile / wave / ring / epilogue / split-K forms and
conv_pp_kernel with its fused GroupNorm apply and skip fold; dts_conv_in3; dts_conv_out3) against tests/conv_reference.py: a float64
reference that shares no code with the library.  Two legs.

EXACT LEG (test_exact).  The inputs of conv_reference.exact_inputs make every product and every partial sum, in any order, exactly
representable in float32 and the result representable in the output type (conv_reference.assert_exact_conditions, asserted for every
launch).  The output must EQUAL the reference; there is no tolerance in this leg.  The output tensor is the middle of a NaN-filled buffer:
every element must have been written and the guard bands on both sides must still be NaN (the first and last convolutions too: `out=`).
Loops whose trip count a launcher derives from the size (the first / last convolutions' grids under their caps, the reduce pass) have cases
that take the second trip; conv_reference.small_trips / reduce_trips restate the rules and each such case asserts, before it runs, that
the reference is nonzero where only the last trip writes.  Where the launch reports GroupNorm strip
statistics they must equal the float64 moments of the stored output (per 64-pixel strip for the implicit-GEMM kernel and the reduce pass,
per image for the ping-pong kernel, whose strips are patch rows); where it cannot, `_gn_stats` must be None.  Each case asserts
ops.conv_kernel's answer and the whole route of ops.conv_plan (tile, waves, ring depth, K split, who wrote the statistics:
_assert_plan), and forms the queries cannot tell apart are forced with _lib.set_tuning (the old values put back whatever
happens).  That includes the K split, which decides whether the kernel's own epilogue or the reduce pass writes the output: every case
pins it (conv_splits = 1, or a forced split under its own name; two `auto_*` cases leave it to the launcher).  The route
table -- which (kernel form) x (mode) cells exist and why the others do not -- is conv_reference.CASES / ABSENT.

ROUNDING LEG (test_rounding).  The Gaussian inputs of the older tests (tests/test_gpu_ops.py), rounded to the storage type, through one
representative shape per route; judged PER ELEMENT against conv_ref64 of the same (rounded) inputs:

    |got - o| <= 1.001 u |o| + c (K + 8) 2^-24 S      [F16X3: + 3 * 2^-22 * sum |x||w| * |out_scale|]

Derivation (written before the first run; nothing here is fitted).  The kernels hold the operands exactly (they were rounded to the
storage type beforehand; the split-precision mode holds float32 operands as hi + lo, see below).  A 16-bit product of two 8- or 11-bit
significands is exact in float32, so the only roundings are (a) the additions of the accumulation, in whatever order the kernel, its K
splits and its reduce pass make them, (b) the epilogue's additions and its multiplication by out_scale, and (c) the final rounding to
the output type.  (a) + (b): a sum of m terms t_i evaluated in ANY order with at most one rounding error of relative size e per operation
is within (m - 1) e sum|t_i| of the exact sum to first order (Higham, Accuracy and Stability of Numerical Algorithms, 4.2; the
second-order remainder is below 1e-4 of this at m <= 3000); here m <= K + 3 terms (K = k*k*cin products [+ the skip source's channels],
bias, bias_nc, residual), one more operation for out_scale, acc_scale's power of two is exact -- (K + 8) covers it -- and sum|t_i| *
|out_scale| is the reference's S.  The matrix cores' internal additions are not documented as round-to-nearest, so e is taken as one
float32 ulp, 2^-23 = c * 2^-24 with c = 2, instead of the half ulp of a rounded addition.  (c): rounding the exact result to the output type
moves it by at most u |o|, u the unit roundoff (2^-8 bfloat16, 2^-11 float16, 2^-24 float32); the value actually rounded differs from o
by the second term, which can carry it across one rounding boundary, hence 1.001 for the interplay.  The f32 products of the f32 parity
kernel round once each (2^-24 |x||w|): one more operation per term, inside the factor c.  F16X3: x = hi + lo, w = wh + wl with f16 parts;
the kernel forms hi.wh + lo.wh + hi.wl.  lo and wl are themselves rounded to f16 (relative 2^-11 of a part that is at most 2^-11 of the
operand: 2^-22 |x| and 2^-22 |w|) and the lo.wl product (<= 2^-22 |x||w|) is dropped: 3 * 2^-22 per product.  (An operand below 2^-13 of its
tensor's scale has an f16-subnormal lo part that the matrix cores flush: it then carries 2^-12 of that operand instead of 2^-22, an
absolute 2^-25 of the tensor's scale -- a thousandth of the bound's smallest term here, and not counted.)

Record of a run of this leg on an MI355X (max err / bound per route; a record, NOT the source of the bound):
    f32_parity / plain   epi_all                  kernel 0:  f32 0.004, bf16 0.937, f16 0.668, f16x3 0.002
    ring3                knob_stages3             kernel 0:  bf16 0.825, f16 0.462, f16x3 0.001
    ring4                knob_stages4             kernel 0:  bf16 0.825, f16 0.462
    waves8               knob_waves8              kernel 0:  bf16 0.834, f16 0.461, f16x3 0.001
    ring3 + splitk       knob_stages3_split3      kernel 0:  bf16 0.801, f16 0.380, f16x3 0.000
    splitk               split3_full_16bit        kernel 0:  bf16 0.771, f16 0.341
    splitk               split3_full_32bit        kernel 0:  f32 0.001, f16x3 0.001
    ragged + up          up_cat                   kernel 0:  f32 0.001, bf16 0.739, f16 0.324, f16x3 0.001
    pp192                pp192_16x16_n2           kernel 6:  bf16 0.865, f16 0.462, f16x3 0.001
    pp128                pp128_32x32              kernel 4:  bf16 0.913, f16 0.680, f16x3 0.003
    pp_up                pp192_up16_cat           kernel 6:  bf16 0.847, f16 0.471, f16x3 0.001
    pp_splitk            pp192_split3_c320        kernel 6:  bf16 0.644, f16 0.255, f16x3 0.000
    pp_splitk            pp128x2_16x16_n2_split2  kernel 4:  bf16 0.850, f16 0.451, f16x3 0.001
    pp_skip              pp192_skip_half          kernel 6:  f16x3 0.002
    pp_skip              pp128_skip_same          kernel 4:  f16x3 0.001
(the 16-bit rows sit near 1 because their bound is dominated by the output rounding, u |o|, which a rounded result reaches by itself;
the float32-output rows show the accumulation term alone)"""
import functools

import pytest
import torch

import conv_reference as R
from conv_reference import CASES, STORE

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD = 4096
U = {'f32': 2.0 ** -24, 'bf16': 2.0 ** -8, 'f16': 2.0 ** -11, 'f16x3': 2.0 ** -24}


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def _exact(name, variant):
    a = R.exact_inputs(name, 'f32', 0, variant)
    return a, R.reference(a)


@functools.lru_cache(maxsize=None)
def _gauss(name, mode):
    a = R.gaussian_inputs(name, mode)
    return a, R.reference(a)


def _kernel_of(case):
    if case.form.startswith('igemm'):
        return 0
    return 6 if case.cout % 192 == 0 else 4


class _Knobs:
    """sets the tuning knobs of a case around its launch and puts back the values they had (dts_get_tuning), whatever happens"""

    def __init__(self, knobs):
        self.knobs, self.old = knobs, []

    def __enter__(self):
        from diffusion_tts_amd import _lib
        lib = _lib.load()
        try:
            for k, v in self.knobs:
                self.old.append((k, int(lib.dts_get_tuning(_lib.KNOBS[k]))))
                _lib.set_tuning(k, v)
        except Exception:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        from diffusion_tts_amd import _lib
        for k, v in reversed(self.old):
            _lib.set_tuning(k, v)
        self.old = []
        return False


def _guarded(shape, dtype):
    """an output tensor in the middle of a NaN-filled buffer: (buffer, view)"""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + 2 * GUARD,), float('nan'), dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + numel].view(shape)


def _assert_plan(case, mode, plan, stats_written):
    """the whole route, not only the kernel: ops.conv_plan (what the launcher itself derives) names the tile, waves and ring depth the case's knobs
    ask for and the K split the table says; and its stats_written is what the launch then reported -- observable from the launch itself, which
    ties the query to what ran"""
    knobs = dict(case.knobs)
    assert plan['refused'] == 0 and plan['kernel'] == _kernel_of(case)
    if plan['kernel'] == 0:
        default_tile = 192 if case.cout % 192 == 0 else 128 if case.cout % 128 == 0 else 64
        assert plan['tile'] == knobs.get('conv_tile', default_tile)
        if mode == 'f32':             # one configuration (conv_reference.KNOB_ABSENT)
            assert (plan['waves'], plan['stages']) == (4, 2)
        else:
            assert plan['waves'] == knobs.get('conv_waves', plan['waves']) and plan['waves'] in (4, 8)
            assert plan['stages'] == knobs.get('conv_stages', plan['stages']) and plan['stages'] in (2, 3, 4)
    else:
        assert (plan['gn'], plan['sk']) == (int(case.gn), int(case.skip is not None))
    if case.splits > 0:
        assert (plan['splits'], plan['ks_per_split']) == R.effective_splits(case, mode)
    else:
        assert plan['splits'] >= 1
    assert plan['stats_written'] == int(stats_written)


def _launch(ops, case, mode, a, want_stats):
    """ops.conv2d of the case on the arguments `a` (float64 CPU tensors): (out NCHW on the CPU in its own dtype, stats or None, the guard
    buffer, the kernel the query names); a SplitQKV's data comes back as it is"""
    dt = STORE[mode]
    x3 = mode == 'f16x3'
    dev = lambda t: None if t is None else t.to(dt).to(DEV).contiguous()
    x1d = dev(R.nhwc(a['x1']))
    x2d = None if a['x2'] is None else dev(R.nhwc(a['x2']))
    wp = ops.pack_conv_weight(a['w'].float().to(DEV), ops.F16X3 if x3 else dt)
    bias = None if a['bias'] is None else a['bias'].float().to(DEV)
    bnc = None
    if a['bias_nc'] is not None:
        bnc = dev(a['bias_nc_wide'])[:, case.cout:] if 'N' in case.ep else dev(a['bias_nc'])
    res = None if a['residual'] is None else dev(R.nhwc(a['residual']))
    kw = {}
    if a['gn'] is not None:
        ga, gb, silu = a['gn']
        kw.update(gn_coef=torch.stack([ga, gb], dim=-1).float().to(DEV).contiguous(), gn_silu=silu)
    if a['skip'] is not None:
        src, w_skip, s_up = a['skip']
        kw['skip'] = (ops.SplitAct(ops.split3_f16(R.nhwc(src).float().to(DEV)), src.shape[1]),
                      ops.pack_conv_weight(w_skip.float().to(DEV), ops.F16X3), s_up)
    ho, wo = R.out_hw(case)
    with _Knobs(case.knobs):
        kernel = ops.conv_kernel(x1d, wp, x2=x2d, up=case.up, residual=res, gn_coef=kw.get('gn_coef'))
        if a['gn'] is not None:
            assert ops.conv_fuses_gn(x1d, wp, x2=x2d)
        if a['skip'] is not None:
            assert ops.conv_folds_skip(x1d, wp, kw['skip'])
        if case.split2:
            call = dict(x2=x2d, bias_nc=bnc, residual=res, up=case.up, out_scale=a['out_scale'], out_split2=True, **kw)
            out = ops.conv2d(x1d, wp, bias, **call)
            torch.cuda.synchronize()
            _assert_plan(case, mode, ops.conv_plan(x1d, wp, bias, **call), False)
            return out.data.cpu(), None, None, kernel
        buf, view = _guarded((case.n, ho, wo, case.cout), dt)
        call = dict(x2=x2d, bias_nc=bnc, residual=res, up=case.up, out_scale=a['out_scale'], out=view, gn_stats=want_stats, **kw)
        out = ops.conv2d(x1d, wp, bias, **call)
        torch.cuda.synchronize()
        _assert_plan(case, mode, ops.conv_plan(x1d, wp, bias, **call), out._gn_stats is not None)
    assert out.data_ptr() == view.data_ptr()
    st = out._gn_stats
    return R.nchw(out.cpu()), (None if st is None else st.cpu()), buf.cpu(), kernel


def _small(ops, case, mode, a):
    """the first / last convolution of a network (conv_small.hip): (output NCHW on the CPU, the guard buffer).  Nothing reports which kernel
    ran: the shapes follow the launchers' rules -- dts_conv_in3 takes the matrix-core kernel iff w % 16 == 0 and cout is 64 / 128 / 192 (16-byte
    aligned bias), else the direct one; dts_conv_out3 takes the tiled kernel iff h % 16 == 0, w % 16 == 0 and c % 32 == 0 (16 in f32), else the
    direct one (conv_reference.small_route restates them and tests/test_conv_reference.py holds every case's form to it).  The output is the
    middle of a NaN-filled buffer handed over as `out=`, like every other launch of this file."""
    dt = STORE[mode]
    bias = None if a['bias'] is None else a['bias'].float().to(DEV)
    if 'B' in case.ep:          # the same bias one float into its storage
        store = torch.zeros(case.cout + 1, device=DEV)
        store[1:] = bias
        bias = store[1:]
        assert bias.data_ptr() % 16 == 4 and bias.is_contiguous()
    if case.form.startswith('in3'):
        buf, view = _guarded((case.n, case.h, case.w, case.cout), dt)
        out = ops.conv_in3(a['x1'].float().to(DEV).contiguous(), a['w'].float().to(DEV).contiguous(), bias, case.cout, dt, out=view)
        torch.cuda.synchronize()
        assert out is view
        return R.nchw(out.cpu()), torch.cat([buf[:GUARD], buf[-GUARD:]]).cpu()        # (the bands alone: the large cases' buffers stay on the device)
    buf, view = _guarded((case.n, 3, case.h, case.w), torch.float32)
    out = ops.conv_out3(R.nhwc(a['x1']).to(dt).to(DEV), a['w'].permute(0, 2, 3, 1).float().contiguous().to(DEV), bias, out=view)
    torch.cuda.synchronize()
    assert out is view
    return out.cpu(), torch.cat([buf[:GUARD], buf[-GUARD:]]).cpu()


@pytest.mark.parametrize('name,mode,variant', R.launches(), ids=lambda v: str(v))
def test_exact(ops, name, mode, variant):
    case = CASES[name]
    # (the large cases' references, up to 2.3 GB, live for this one test: _exact.__wrapped__ is the function without its cache)
    a, ref = _exact.__wrapped__(name, variant) if name in R.LARGE else _exact(name, variant)
    small = case.form.startswith('in3') or case.form.startswith('out3')
    out_dt = torch.float32 if case.form.startswith('out3') else STORE[mode]
    ho, wo = R.out_hw(case)
    want_stats = case.stats and variant == 'int'
    want = ref.o.to(out_dt)
    stats64 = None
    if want_stats and (ho * wo) % 64 == 0:
        stats64 = R.image_stats64(want) if case.form.startswith('pp') else R.strip_stats64(want)
    R.assert_exact_conditions(ref, out_dt, stats64, a)
    if small:
        assert R.small_route(case, mode) == case.form
        t = R.small_trips(case, mode)
        if t.trips > 1:         # what only the last trip writes is not all zero: a launch without it cannot equal the reference
            assert bool((R.last_trip_values(case, mode, want) != 0).any(1).all())
        got, bands = _small(ops, case, mode, a)
        print(f'{name} [{mode}]: {case.form}, {t.blocks} blocks, {t.trips} trip(s) of the size-driven loop'
              + (f', staging groups {R.in3_direct_groups(case, mode)}' if case.form == 'in3_direct' else ''))
        assert got.dtype == out_dt
        assert not bool(torch.isnan(got).any()), 'an output element was never written'
        assert torch.equal(got, want), f'{int((got != want).sum())} of {want.numel()} elements differ'
        assert bool(torch.isnan(bands[:GUARD]).all()) and bool(torch.isnan(bands[-GUARD:]).all()), 'a store outside the output'
        return
    if name == 'split2_reduce_2trips':
        t = R.reduce_trips(case, mode)
        assert t.trips == 2 and bool((R.last_trip_values(case, mode, want).reshape(-1, 4) != 0).any(1).all())
    got, st, buf, kernel = _launch(ops, case, mode, a, want_stats)
    split = {-1: 'by the launcher', 0: 'none'}.get(case.splits, case.splits)
    print(f'{name} [{mode}, {variant}]: kernel {kernel} ({case.form}), K split {split}, knobs {dict(case.knobs)}')
    assert kernel == _kernel_of(case)
    if case.split2:         # the attention's operand image: hi(cout) | lo(cout) of 64 * o, hi the float16 rounding
        o64 = 64.0 * R.nhwc(ref.o)
        hi, lo = got[..., :case.cout].double(), got[..., case.cout:].double()
        assert got.dtype == torch.float16 and tuple(got.shape) == (case.n, ho, wo, 2 * case.cout)
        assert torch.equal(hi, o64.to(torch.float16).double()) and torch.equal(hi + lo, o64)
        return
    assert got.dtype == out_dt
    assert not bool(torch.isnan(got).any()), 'an output element was never written'
    assert torch.equal(got, want), f'{int((got != want).sum())} of {want.numel()} elements differ'
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), 'a store outside the output'
    if not want_stats or (ho * wo) % 64 != 0:
        assert st is None
    else:
        assert st is not None and tuple(st.shape) == (case.n * ho * wo // 64, case.cout, 2)
        if case.form.startswith('pp') and case.splits <= 1:
            st = st.double().view(case.n, -1, case.cout, 2).sum(1)          # per image (exact: integers far below 2^53)
            assert torch.equal(st, stats64)
        elif case.form.startswith('pp'):                                     # (the reduce pass of a split launch works in pixel strips)
            assert torch.equal(st, R.strip_stats64(want).float())
        else:
            assert torch.equal(st, stats64.float())


def test_first_and_last_convolution_refuse_a_wrong_out(ops):
    """out= of conv_in3 / conv_out3 (every exact case above hands one over): a tensor of another shape, type, device or layout raises; the
    allocating form gives the same bits"""
    x = torch.randn(1, 3, 12, 20, generator=torch.Generator().manual_seed(1)).to(DEV)
    w = torch.randn(64, 3, 3, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    good = torch.empty(1, 12, 20, 64, dtype=torch.bfloat16, device=DEV)
    assert ops.conv_in3(x, w, None, 64, torch.bfloat16, out=good) is good and torch.equal(good, ops.conv_in3(x, w, None, 64, torch.bfloat16))
    for bad in (torch.empty(1, 12, 20, 128, dtype=torch.bfloat16, device=DEV), torch.empty(1, 12, 20, 64, dtype=torch.float16, device=DEV),
                torch.empty(1, 12, 20, 64, dtype=torch.bfloat16), torch.empty(1, 12, 20, 128, dtype=torch.bfloat16, device=DEV)[..., ::2]):
        with pytest.raises(ValueError):
            ops.conv_in3(x, w, None, 64, torch.bfloat16, out=bad)
    xl, wl = good, torch.randn(3, 3, 3, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
    o3 = torch.empty(1, 3, 12, 20, device=DEV)
    assert ops.conv_out3(xl, wl, None, out=o3) is o3 and torch.equal(o3, ops.conv_out3(xl, wl, None))
    for bad in (torch.empty(1, 3, 20, 12, device=DEV), torch.empty(1, 3, 12, 20, dtype=torch.float16, device=DEV), torch.empty(1, 3, 12, 20),
                torch.empty(1, 3, 12, 40, device=DEV)[..., ::2]):
        with pytest.raises(ValueError):
            ops.conv_out3(xl, wl, None, out=bad)


ROUTES = [  # (route, case, modes): one representative shape per route
    ('f32_parity / plain', 'epi_all', R.MODES),
    ('ring3', 'knob_stages3', R.H16 + ('f16x3',)),
    ('ring4', 'knob_stages4', R.H16),
    ('waves8', 'knob_waves8', R.H16 + ('f16x3',)),
    ('ring3 + splitk', 'knob_stages3_split3', R.H16 + ('f16x3',)),
    ('splitk', 'split3_full_16bit', R.H16),
    ('splitk', 'split3_full_32bit', R.W32),
    ('ragged + up', 'up_cat', R.MODES),
    ('pp192', 'pp192_16x16_n2', R.H16 + ('f16x3',)),
    ('pp128', 'pp128_32x32', R.H16 + ('f16x3',)),
    ('pp_up', 'pp192_up16_cat', R.H16 + ('f16x3',)),
    ('pp_splitk', 'pp192_split3_c320', R.H16 + ('f16x3',)),
    ('pp_splitk', 'pp128x2_16x16_n2_split2', R.H16 + ('f16x3',)),
    ('pp_skip', 'pp192_skip_half', ('f16x3',)),
    ('pp_skip', 'pp128_skip_same', ('f16x3',)),
]


@pytest.mark.parametrize('route,name,mode', [(r, c, m) for r, c, ms in ROUTES for m in ms])
def test_rounding(ops, route, name, mode):
    case = CASES[name]
    a, ref = _gauss(name, mode)
    got, st, buf, kernel = _launch(ops, case, mode, a, False)
    assert kernel == _kernel_of(case)
    K = case.k * case.k * (case.c1 + case.c2) + (case.skip[0] if case.skip else 0)
    bound = 1.001 * U[mode] * ref.o.abs() + 2.0 * (K + 8) * 2.0 ** -24 * ref.S
    if mode == 'f16x3':
        bound = bound + 3.0 * 2.0 ** -22 * ref.prod
    err = (got.double() - ref.o).abs()
    ratio = float((err / bound).max())
    print(f'rounding {route} {name} [{mode}]: kernel {kernel}, max err/bound = {ratio:.3f}')
    assert bool((err <= bound).all()), ratio
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())
