"""Batches past 2^31 and 2^32 bytes per tensor through the kernels of the lock-step and VAE paths: launch_rules.LARGE_CASES, one launch each.

The construction (tests/large_rows.py): the batch is x = base[idx], base the K = 7 samples of an EXISTING small case of the kernel's reference
module and idx a seeded random map.  After the launch
    1. every row with idx == k is BIT-equal to the first such row (integer view, in chunks) -- identical rows at different batch positions give
       identical bits, so exact ties of the search stay ties at every batch position up to the 4 GiB mark;
    2. the first row of each class meets the criterion its reference module already uses (conv: EQUAL to the float64 reference on the exact
       inputs; GroupNorm, attention, the row kernels: their derived bounds, unchanged) -- no tolerance is new here;
    3. the output is the middle of a NaN-filled buffer: no NaN in the first rows (with 1: every element was written), both bands still NaN.
A case whose tensors exceed the free device memory skips with both numbers; there is no other skip.  tests/test_large_rows_cpu.py holds the
table, the map and the comparison to account without a GPU, and pins every dts_conv2d route and the switch at the limits through launch-free
queries; no launching entry point is ever called here with a size its buffers do not back.

SIZE LIMITS (the audit this file was written from: widest type of every element / byte offset, the host guard with its line, what it supports;
csrc/ is diffusion_tts_amd/csrc/)

  entry point                  offsets in the kernel                                  host guard (file:line)                           supports
  dts_conv2d, implicit GEMM    pixel index int (n*h*w of output and input); every     conv_igemm.hip:1974 n*hin*win*(up ? 4 : 1) < 2^30  < 2^30 pixels per tensor; bytes
    (+ phase up=2, stride 2)   byte offset (size_t)pixel * channels * size; phase     "too many pixels"; :2022 hout, wout < 32768;       unlimited below that
                               form: PhaseTileMap::pix in int (< P)                   :2045-2053 what up = 2 takes
  dts_conv2d, ping-pong        loads: 32-bit lane offsets into buffer descriptors     conv_igemm.hip:1851-1853 (conv_pp_eligible)        each OPERAND < 2^31 bytes, else the
    (kernel 6 / 4, GN, skip)   (:1211, :1492-1493 byte count as uint32_t, DTS_OOR =   n*hin*win*max(c1,c2)*2 < 2^31, weights < 2^31      implicit GEMM takes the layer; output,
                               2^31 marks padding); stores, residual, statistics:     (also :1871), P < 2^30; skip source :2014 < 2^31   residual, statistics 64-bit
                               (size_t)pixel * cout * 2
  split-K reduce               (size_t)pixel * cout, slab (size_t)P * cout            conv_igemm.hip:1790, :1808, :1841 slabs fit the    as the launch it follows
                                                                                      workspace
  dts_conv_in3                 direct: long long pixel, (size_t) offsets; matrix-core conv_small.hip:284 nseg < 2^31 - 8192, else the    any size (direct kernel 64-bit)
                               form: int segment + int stride gridDim.x * 4           direct kernel
  dts_conv_out3                tiled: int block -> (size_t) offsets; direct: long     conv_small.hip:315 n*(h/16)*(w/16) < 2^31, else    any size
                               long pixel                                             the direct kernel
  dts_gn_coef                  (size_t)n * hw * C; grid.y = n                         groupnorm.hip:471 n <= 65535                       n <= 65535
  dts_gn_fused, _coef_strips   (size_t)n * hw * C; grid.y = n                         groupnorm.hip:583, :499 n <= 65535                 n <= 65535
  dts_gn_apply, _apply_x3      rows kernel grid.y = n, (size_t) offsets; grid kernel  groupnorm.hip:537, :559 n <= 65535 for the rows    any n (in practice n <= 65535: the
                               long long thread index                                 kernel, else the grid-stride kernel                coefficients come from the above)
  dts_attention, _masked       64-bit base per block (size_t)n * t * rowstride        attention.hip:875 blocks < 2^31                    2^31 blocks
  dts_attention_x3, _x3_masked 64-bit base per block; 32-bit buffer offsets INSIDE    attention.hip:931, :956 t*6*heads*d*2 < 2^31;      one sample's rows < 2 GiB
                               one sample                                             :875
  dts_cross_attention          64-bit row bases                                       transformer.hip:256 grid < 2^31                    2^31 blocks
  dts_geglu                    long long thread and row index                         transformer.hip:287 grid < 2^31                    2^31 blocks of 256 vectors
  dts_layer_norm               long long row, row * stride                            transformer.hip:266 rows < 2^32                    rows < 2^32
  dts_gelu                     long long vector index                                 vit.hip:174 grid < 2^31 (count % 8: :219)          2^31 blocks of 256 vectors
  dts_cast_*, dts_split2/3_f16 GSL: long long index and stride (elementwise.hip:53)   counts int64_t: elementwise.hip:791, :801, :771,   count < 2^63
  dts_quantize_u8, _u8_to_unit                                                        :780, :959, :1004, :1103; grid capped (grid1d :47)
  dts_cfg_combine
  dts_nchw_to_nhwc(_pad),      GSL over (long long)n*c*h*w; coordinates by division   elementwise.hip:679, :700, :710 (positive ints;    n, c, h, w < 2^31 each
  dts_nhwc_to_nchw                                                                    totals :681, :702, :712 in long long)
  dts_edm_precond_in / _out,   GSL over (long long)n * chw; row = (int)(i / chw)      elementwise.hip:813, :838, :883, :898, :907,       n, chw < 2^31 each
  dts_heun_*_rows,                                                                    :1068 (n, chw > 0 as int; products in long long)
  dts_candidate_noise_rows,
  dts_brightness               one block per image, (size_t)blockIdx.x * 3 * hw       elementwise.hip:971
  dts_resample2x, _resample_fir long long thread index, (size_t) pixel offsets        groupnorm.hip:599 / resample.hip:166 totals in     n*h*w*c < 2^63
                                                                                      long long, grid capped (grid_for, grid1d)
  dts_ddim_candidates(_groups) GSL over count (x groups), (size_t) candidate offsets  elementwise.hip:1115, :1128 (count int64_t)        count < 2^63 (no 2^31 cap)
  dts_candidate_noise_sd(_rows) one block per candidate, (size_t)cn * count; INSIDE a elementwise.hip:1079, :1091 count <= 2^31 - 256,   a candidate of < 2^31 - 256
                               candidate `int i += 256`                               searches * per < 2^31                              elements; rows 64-bit
  dts_jpeg_size                int bit counts / offsets per image; int64 workspace    jpeg.hip:289-294 (shape_ok, asked launch-free      n <= 65535, n * blocks <= 2^24 (the
                               layout                                                 through dts_jpeg_workspace_bytes :313), :318       bit buffer, 256 B per block, < 2^32)
  dts_group_rows               (size_t)row * chunks; chunks int                       group_rows.hip:123 n <= 1024, row_bytes / 16 < 2^31 1024 rows of < 32 GiB
Findings.  conv_in3_mfma_kernel's `seg += gridDim.x * 4` and candidate_noise_sd_kernel's `i += blockDim.x` are int sums that could pass 2^31
just under their guards (nseg < 2^31, count < 2^31): the guards now leave the step's room (2^31 - 8192, 2^31 - 256).  dts_gn_coef launched
grid.y = n without its own check (a launch error past 65535, no fault): it refuses by name like its siblings.  Nothing else: every byte offset is
64-bit.  The caps: dts_jpeg_size runs AT its cap (n * 384 blocks, the last n the query admits; test_large_rows_cpu.py asks the query from both
sides), dts_group_rows at its 1024 rows of 4 MiB, the last 7 beyond byte 2^32.  dts_candidate_noise_sd*'s cap is on ONE candidate's elements, which
one block walks: a candidate of 2^31 - 256 elements is a single row (no classes, no reference of that size, tens of seconds on one CU), so
these run with latents of 16384 elements in 131079 rows, past 2^32 bytes in total; their cap has no launch-free query and is not pinned.
dts_ddim_candidates* carry no 2^31 cap: both forms run past 2^31 elements.

Record of a run on an MI355X (53 passed, none skipped, 14 s; a record, not the source of any bound).  Every class bit-identical in every case.
The seven reference rows, beside what the same kernel's small case records in its own file:
  dts_conv2d (10 cases, the phase form among them), dts_conv_in3 / _out3 (4)    0 elements differ (exact leg, as in test_gpu_conv*.py)
  GroupNorm f32: split 0.61, fused 0.46, strips 0.46, pooled 0.82, split image 0.61 of K = 4 (test_gpu_groupnorm.py: up to 1.25 / 0.86 / 1.49);
  bf16: inside 1.01 ulp + the float32 bound on every route (coefficients 0.68 / 0.40 of K; there 0.92)
  attention d = 64 bf16 0.258, masked kernel f16 0.247, d = 40 bf16 0.242 of bound16 (randn there: 0.26 - 0.42); split precision 2.26 of K = 4 (2.16)
  cross attention (kv_rows, 2 contexts) 0.289; layer_norm 0.992, geglu 0.999, gelu 0.975, quick-GELU 0.989 (the output rounding fills these bounds)
  casts, quantiser, u8 -> [0, 1], the three layout kernels, both split images, resample2x and resample_fir up and down: 0 elements differ
  brightness 0.17, cfg_combine 0.996 (output rounding), precond in 0.14 / 0.28, out 0.47, Heun rows 0.25 / 0 / 0.15 / 0.16, candidate_noise_rows 0.75
  DDIM candidates 0.99 (output rounding); candidate_noise_sd and _rows (float16): 0 elements differ from the reference expression;
  jpeg_size: the 7 sizes equal Pillow's; group_rows: 1017 groups, the 7 twins beyond 2^32 bytes found
One dtype per case; the second 16-bit type of each case is not run here."""
import math

import pytest
import torch

import conv_reference as R
import elementwise_reference as E
import large_rows as LG
import launch_rules as LR
import resample_reference as RS
import test_gpu_attention as TA
import test_gpu_clip_vision_ops as TV
import test_gpu_conv_stride as TS
import test_gpu_groupnorm as TG
import test_gpu_sd_unet_ops as TU

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DT = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _free_memory():
    yield
    torch.cuda.empty_cache()


def _cases(family):
    return [c for c in LR.LARGE_CASES.values() if c.family == family]


def _begin(lc, extra_bytes=0):
    """the one skip: tensors of the case against the free device memory; prints the bookkeeping; returns the map"""
    need = sum(t.bytes for t in lc.tensors) + extra_bytes + (256 << 20)
    free, _ = torch.cuda.mem_get_info()
    if need > free:
        pytest.skip(f'{lc.name} needs {need} bytes of device memory, {free} are free')
    print(f'\n{lc.name}: n = {lc.n}; ' + '; '.join(f'{t.name} {t.bytes} B crosses [{" ".join(t.crosses)}]' for t in lc.tensors))
    return LG.row_map(lc.n)


def _check_rows(lc, what, out, idx, buf=None):
    """bit equality of the classes, the bands, no NaN in the first rows; returns the K first rows on the CPU"""
    torch.cuda.synchronize()
    LG.assert_classes_bit_equal(out, idx, f'{lc.name} {what}')
    if buf is not None:
        assert LG.bands_intact(buf), f'{lc.name} {what}: a store outside the output'
    first = LG.first_of_classes(out, idx)
    if first.dtype.is_floating_point:
        assert not bool(torch.isnan(first).any()), f'{lc.name} {what}: an output element was never written'
    return first


# ---- dts_conv2d ---------------------------------------------------------------------------------------------------------------------------
def _small_case(lc):
    """the K-sample twin of a large dts_conv2d case as a conv_reference.Case (exact_inputs draws from its fields)"""
    s = lc.spec
    form = ('pp_gn' if s['gn'] else 'pp192') if s['plan']['kernel'] == 6 else 'igemm'
    return R.Case('large_' + lc.name, form, (s['mode'],), LG.K, s['h'], s['w'], s['c1'], 0, s['cout'], s['k'], s['up'] in (1, 2), s['ep'], 1.0, s['stats'], (),
                  ('int',), s['gn'], None, False, 1, '')


def _conv_reference(lc):
    case, s = _small_case(lc), lc.spec
    a = R.exact_inputs(case, s['mode'], 0, 'int')
    if s['up'] == -1:
        ref = TS.reference(a)
    else:
        ref = R.reference(a)
    return case, a, ref


@pytest.mark.parametrize('lc', _cases('conv2d'), ids=lambda c: c.name)
def test_conv2d(ops, lc):
    s, mode = lc.spec, lc.spec['mode']
    case, a, ref = _conv_reference(lc)
    dt, x3 = R.STORE[mode], mode == 'f16x3'
    ho, wo = ((s['h'] + 1) // 2, (s['w'] + 1) // 2) if s['up'] == -1 else R.out_hw(case)
    want = ref.o.to(dt)
    stats64 = R.image_stats64(want) if s['stats'] else None
    R.assert_exact_conditions(ref, dt, stats64, a)
    idx = _begin(lc)
    dev = lambda t: t.to(dt).to(DEV).contiguous()
    base = dev(R.nhwc(a['x1']))
    if x3:          # the operand image of the K samples, tiled: the launch reads it as it reads a GroupNorm's split output
        x1 = ops.SplitAct(LG.tile(ops.split3_f16(base), idx), s['c1'])
    else:
        x1 = LG.tile(base, idx)
    wp = ops.pack_conv_weight(a['w'].float().to(DEV), ops.F16X3 if x3 else dt, up_phases=s['up'] == 2)
    bias = a['bias'].float().to(DEV)
    call = dict(up=s['up'] in (1, 2), stride=2 if s['up'] == -1 else 1, out_scale=a['out_scale'], gn_stats=s['stats'])
    if s['up'] == 2:          # the phase form or a refusal, never the nine-tap route by a quiet choice
        call['phases'] = True
    if 'n' in s['ep']:
        call['bias_nc'] = LG.tile(dev(a['bias_nc']), idx)
    if 'r' in s['ep']:
        call['residual'] = LG.tile(dev(R.nhwc(a['residual'])), idx)
    if s['gn']:
        ga, gb, silu = a['gn']
        call.update(gn_coef=LG.tile(torch.stack([ga, gb], dim=-1).float().to(DEV), idx), gn_silu=silu)
    buf, view = LG.guarded((lc.n, ho, wo, s['cout']), dt, DEV)
    call['out'] = view
    # the route, BEFORE the launch (dts_conv_plan launches nothing): what the table says, unsplit
    plan = ops.conv_plan(x1, wp, bias, **call)
    assert plan['refused'] == 0 and plan['splits'] == 1
    for f, v in s['plan'].items():
        assert plan[f] == v, (f, plan)
    out = ops.conv2d(x1, wp, bias, **call)
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr()
    assert plan['stats_written'] == int(out._gn_stats is not None) == int(s['stats'])
    first = _check_rows(lc, 'out', out, idx, buf)
    got = R.nchw(first)
    ndiff = int((got != want).sum())
    print(f'  route: kernel {plan["kernel"]}, tile {plan["tile"]}, waves {plan["waves"]}, stages {plan["stages"]}, splits {plan["splits"]}, '
          f'{plan["nblk"]} blocks; {ndiff} of {want.numel()} elements of the {LG.K} reference rows differ (exact leg)')
    assert got.dtype == dt and torch.equal(got, want), f'{ndiff} of {want.numel()} elements differ'
    if s['stats']:
        st = out._gn_stats.view(lc.n, -1)
        # (ops.conv2d allocates the statistics itself: no bands around them; every class bit-identical and the first rows equal to the moments)
        first_st = _check_rows(lc, 'statistics', st, idx)
        per_image = first_st.double().view(LG.K, -1, s['cout'], 2).sum(1)
        assert torch.equal(per_image, stats64)


# ---- first and last convolutions ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lc', _cases('conv_in3') + _cases('conv_out3'), ids=lambda c: c.name)
def test_first_and_last_convolution(ops, lc):
    s, mode = lc.spec, lc.spec['mode']
    dt = R.STORE[mode]
    first_conv = lc.family == 'conv_in3'
    case = R.Case('large_' + lc.name, s['route'], (mode,), LG.K, s['h'], s['w'], 3 if first_conv else s['c'], 0, s['cout'] if first_conv else 3, 3, False, 'b',
                  1.0, False, (), ('int',), False, None, False, 0, '')
    assert R.small_route(case, mode) == s['route']
    a = R.exact_inputs(case, mode, 0, 'int')
    ref = R.reference(a)
    out_dt = dt if first_conv else torch.float32
    R.assert_exact_conditions(ref, out_dt, None, a)
    idx = _begin(lc)
    bias = a['bias'].float().to(DEV)
    if first_conv:
        x = LG.tile(a['x1'].float().to(DEV).contiguous(), idx)
        buf, view = LG.guarded((lc.n, s['h'], s['w'], s['cout']), dt, DEV)
        out = ops.conv_in3(x, a['w'].float().to(DEV).contiguous(), bias, s['cout'], dt, out=view)
    else:
        x = LG.tile(R.nhwc(a['x1']).to(dt).to(DEV), idx)
        buf, view = LG.guarded((lc.n, 3, s['h'], s['w']), torch.float32, DEV)
        out = ops.conv_out3(x, a['w'].permute(0, 2, 3, 1).float().contiguous().to(DEV), bias, out=view)
    assert out is view
    first = _check_rows(lc, 'out', out, idx, buf)
    got, want = (R.nchw(first) if first_conv else first), ref.o.to(out_dt)
    t = R.small_trips(case._replace(n=lc.n), mode)
    ndiff = int((got != want).sum())
    print(f'  route: {s["route"]}, {t.blocks} blocks, {t.trips} trip(s); {ndiff} of {want.numel()} elements of the {LG.K} reference rows differ (exact leg)')
    assert torch.equal(got, want), f'{ndiff} of {want.numel()} elements differ'


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------------------------
def _gn_apply(ops, x, coef, out, silu, pool, split=False):
    """dts_gn_apply / dts_gn_apply_x3 into a caller-owned (guarded) output: ops.gn_apply with `out`"""
    n, h, w, c = x.shape
    if split:
        ops._call('dts_gn_apply_x3', x.data_ptr(), c, None, 0, coef.data_ptr(), out.data_ptr(), None, n, h, w, int(silu), int(pool))
    else:
        ops._call('dts_gn_apply', x.data_ptr(), c, None, 0, ops.dt_code(x.dtype), coef.data_ptr(), out.data_ptr(), n, h, w, int(silu), int(pool))


@pytest.mark.parametrize('lc', _cases('groupnorm'), ids=lambda c: c.name)
def test_groupnorm(ops, lc):
    s = lc.spec
    dt, c, h, w = DT[s['mode']], s['c'], s['h'], s['w']
    f32 = dt == torch.float32
    assert lc.n <= 65535 and tuple(TG.routes_for(c, 0, h, w)) == s['routes']
    assert LR.gn_apply_plan(lc.n, c, 0, h, w, f32).kernel == s['apply'] and LR.gn_apply_plan(lc.n, c, 0, h, w, f32, pool=True).kernel == 'grid'
    cs = TG.Case('network_hi', LG.K, c, 0, h, w, True, dtype=dt)
    idx = _begin(lc, extra_bytes=-sum(t.bytes for t in lc.tensors if t.name.startswith('out_')))
    x = LG.tile(TG.nhwc(cs.x1, dt), idx)
    g, b = cs.gamma.to(DEV), cs.beta.to(DEV)
    ss = LG.tile(cs.ss.to(DEV, dt), idx)
    strips = LG.tile(TG.strip_stats(cs.x1).view(LG.K, (h * w) // 64, c, 2), idx).view(-1, c, 2)

    def judge(what, first, pool, extra=0.0):
        return TG.check_out(cs, what, first, cs.ref(pool), extra=extra, what='large rows')

    for route in s['routes']:
        buf, view = LG.guarded((lc.n, h, w, c), dt, DEV)
        coef = None
        if route == 'fused':
            ops._call('dts_gn_fused', x.data_ptr(), c, None, 0, ops.dt_code(dt), lc.n, h * w, cs.groups, float(cs.eps), g.data_ptr(), b.data_ptr(),
                      ss.data_ptr(), ss.stride(0), view.data_ptr(), int(cs.silu))
        else:
            if route == 'split':
                coef = ops.gn_coef(x, cs.groups, cs.eps, g, b, scale_shift=ss)
            else:
                x._gn_stats = strips
                coef = ops._coef_from_strips(x, None, cs.groups, cs.eps, g, b, ss)
                assert coef is not None
            _gn_apply(ops, x, coef, view, cs.silu, False)
        first = _check_rows(lc, route, view, idx, buf)
        ratio = judge(route, TG.nchw64(first), False)
        if coef is not None:
            TG.check_coef(cs, route, _check_rows(lc, route + ' coef', coef, idx), cs.ref(False))
        print(f'  {lc.name} {route}: ratio {ratio:.2f} (limit K = {TG.K})')
        del buf, view
        if route != 'split':
            continue
        # pooled apply (the grid-stride kernel) and, float32, the split-precision image, from the same coefficients
        buf, view = LG.guarded((lc.n, h // 2, w // 2, c), dt, DEV)
        _gn_apply(ops, x, coef, view, cs.silu, True)
        print(f'  {lc.name} pooled: ratio {judge("pool", TG.nchw64(_check_rows(lc, "pooled", view, idx, buf)), True):.2f}')
        del buf, view
        if f32:
            buf, view = LG.guarded((lc.n, h, w, 2 * c), torch.float16, DEV)
            _gn_apply(ops, x, coef, view, cs.silu, False, split=True)
            first = _check_rows(lc, 'split image', view, idx, buf)
            ratio = judge('split image', TG.split_value(ops.SplitAct(first, c)), False, extra=2.0 ** -22)
            print(f'  {lc.name} split image: ratio {ratio:.2f}')
            del buf, view
        del coef
        torch.cuda.empty_cache()


# ---- attention -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lc', _cases('attention'), ids=lambda c: c.name)
def test_attention(ops, lc):
    s = lc.spec
    form, t, heads, d = s['form'], s['t'], s['heads'], s['d']
    c, dt = heads * d, DT[s['mode']]
    scale = 1.0 / math.sqrt(d)
    idx = _begin(lc)
    if form.startswith('x3'):
        x, ref_o, e32 = TA.case32('randn', t, heads, d, n=LG.K)
        image = ops.split2_f16(x.to(DEV))
        assert tuple(image.shape) == (LG.K, t, 6 * c)
        qkv = LG.tile(image, idx)
        buf, view = LG.guarded((lc.n, t, c), torch.float32, DEV)
        ops._call('dts_attention_x3', qkv.data_ptr(), view.data_ptr(), 0, lc.n, t, heads, d, scale)
    else:
        x, ref_o, bound = TA.case16('randn', t, heads, d, dt, n=LG.K)
        qkv = LG.tile(x.to(DEV), idx)
        buf, view = LG.guarded((lc.n, t, c), dt, DEV)
        assert TA.launch(ops, form, qkv, heads, out=view) is view
    first = _check_rows(lc, 'out', view, idx, buf)
    if form.startswith('x3'):
        ratio, limit = float((TA.head_err(first, ref_o, heads) / e32.clamp_min(TA.FLOOR)).max()), TA.K
    else:
        ratio, limit = float(((first.double() - ref_o).abs() / bound).max()), 1.0
    print(f'  {lc.name} {form}: max err / bound = {ratio:.3f} (limit {limit:g})')
    assert ratio <= limit, ratio


# ---- row and element-wise kernels of the lock-step and VAE paths ----------------------------------------------------------------------------
# One function per kernel: (ops, lc, idx) -> None.  Each builds its K base samples from the kernel's reference module (the case builders and
# value ranges of tests/elementwise_reference.py, tests/resample_reference.py, tests/test_gpu_sd_unet_ops.py), tiles them, launches ONCE into a
# guarded output through the C entry point (the ops.* wrapper with a caller-owned output) and judges the K first rows by that module's rule.
ROW_OPS = {}


def row_op(fn):
    ROW_OPS[fn.__name__] = fn
    return fn


def _shape(lc, name):
    return next(t.sample_shape for t in lc.tensors if t.name == name)


def _gen(lc):
    return torch.Generator().manual_seed(sum(ord(ch) for ch in lc.name))


def _exact(lc, what, first, want):
    ndiff = int((first != want).sum())
    print(f'  {lc.name} {what}: {ndiff} of {want.numel()} elements of the {LG.K} reference rows differ (exact)')
    assert first.dtype == want.dtype and first.shape == want.shape and ndiff == 0, ndiff


def _bounded(lc, what, first, ref, bound):
    ratio, err = E.worst(first, ref, bound)
    print(f'  {lc.name} {what}: max err {err:.3e}, max err / bound {ratio:.3f}')
    assert ratio <= 1.0, ratio


@row_op
def cast_from_f32_bf16(ops, lc, idx):
    dt = DT[lc.spec['mode']]
    base = torch.randn((LG.K,) + _shape(lc, 'x'), generator=_gen(lc)) * 3
    x = LG.tile(base.to(DEV), idx)
    buf, view = LG.guarded((lc.n,) + _shape(lc, 'out'), dt, DEV)
    ops._call('dts_cast_from_f32', x.data_ptr(), view.data_ptr(), ops.dt_code(dt), x.numel())
    _exact(lc, 'out', _check_rows(lc, 'out', view, idx, buf), base.to(dt))


@row_op
def cast_to_f32_f16(ops, lc, idx):
    dt = DT[lc.spec['mode']]
    base = (torch.randn((LG.K,) + _shape(lc, 'x'), generator=_gen(lc)) * 3).to(dt)
    x = LG.tile(base.to(DEV), idx)
    buf, view = LG.guarded((lc.n,) + _shape(lc, 'out'), torch.float32, DEV)
    ops._call('dts_cast_to_f32', x.data_ptr(), ops.dt_code(dt), view.data_ptr(), x.numel())
    _exact(lc, 'out', _check_rows(lc, 'out', view, idx, buf), base.float())


@row_op
def quantize_u8_f32(ops, lc, idx):
    m = LG.numel(_shape(lc, 'x'))
    base = E.quantize_random(torch.float32, LG.K * m, seed=90).view((LG.K,) + _shape(lc, 'x'))
    edges = E.quantize_edges(torch.float32)
    base.view(LG.K, -1)[3, :edges.numel()] = edges
    x = LG.tile(base.to(DEV), idx)
    buf, view = LG.guarded((lc.n,) + _shape(lc, 'out'), torch.uint8, DEV)
    ops._call('dts_quantize_u8', x.data_ptr(), 2, view.data_ptr(), x.numel())           # 2: float32 arithmetic (the SD loop's form)
    _exact(lc, 'out', _check_rows(lc, 'out', view, idx, buf), E.quantize_two_step(base))


@row_op
def u8_to_unit_f32(ops, lc, idx):
    base = torch.randint(0, 256, (LG.K,) + _shape(lc, 'img'), generator=_gen(lc), dtype=torch.uint8)
    base.view(LG.K, -1)[2, :256] = torch.arange(256, dtype=torch.uint8)
    x = LG.tile(base.to(DEV), idx)
    buf, view = LG.guarded((lc.n,) + _shape(lc, 'out'), torch.float32, DEV)
    ops._call('dts_u8_to_unit_f32', x.data_ptr(), view.data_ptr(), x.numel())
    _exact(lc, 'out', _check_rows(lc, 'out', view, idx, buf), E.u8_to_unit_ref(base))


@row_op
def brightness(ops, lc, idx):
    c, h, w = _shape(lc, 'img')
    base = E.brightness_images(h * w, LG.K)
    x = LG.tile(base.to(DEV), idx)
    buf, view = LG.guarded((lc.n, 1), torch.float32, DEV)
    ops._call('dts_brightness', x.data_ptr(), view.data_ptr(), lc.n, h * w)
    ref, bound = E.brightness_ref(base)
    _bounded(lc, 'rewards', _check_rows(lc, 'out', view, idx, buf)[:, 0], ref, bound)


@row_op
def cfg_combine_bf16(ops, lc, idx):
    dt, g = DT[lc.spec['mode']], E.GUIDANCE[2]
    gen = _gen(lc)
    u, c = (torch.randn((LG.K,) + _shape(lc, 'out'), generator=gen).to(dt) for _ in range(2))
    ud, cd = LG.tile(u.to(DEV), idx), LG.tile(c.to(DEV), idx)
    buf, view = LG.guarded((lc.n,) + _shape(lc, 'out'), dt, DEV)
    ops._call('dts_cfg_combine', ud.data_ptr(), cd.data_ptr(), float(g), view.data_ptr(), ops.dt_code(dt), ud.numel())
    ref, bound = E.cfg_ref(u, c, g)
    _bounded(lc, f'guidance {g}', _check_rows(lc, 'out', view, idx, buf), ref, E.rounded_bound(ref, bound, dt))


def _layout(ops, lc, idx, entry, cpad=None):
    dt = DT[lc.spec['mode']]
    c, h, w = _shape(lc, 'x')
    base = torch.randn(LG.K, c, h, w, generator=_gen(lc)) * 2
    x = LG.tile(base.to(DEV), idx)
    buf, view = LG.guarded((lc.n,) + _shape(lc, 'out'), dt, DEV)
    ops._call(entry, x.data_ptr(), view.data_ptr(), ops.dt_code(dt), lc.n, c, h, w, *(() if cpad is None else (cpad,)))
    _exact(lc, 'out', _check_rows(lc, 'out', view, idx, buf), E.nchw_to_nhwc_ref(base, dt, cpad))


@row_op
def nchw_to_nhwc_bf16(ops, lc, idx):
    _layout(ops, lc, idx, 'dts_nchw_to_nhwc')


@row_op
def nchw_to_nhwc_pad_f16(ops, lc, idx):
    _layout(ops, lc, idx, 'dts_nchw_to_nhwc_pad', cpad=_shape(lc, 'out')[-1])


@row_op
def nhwc_to_nchw_bf16(ops, lc, idx):
    dt = DT[lc.spec['mode']]
    h, w, c = _shape(lc, 'x')
    base = (torch.randn(LG.K, h, w, c, generator=_gen(lc)) * 2).to(dt)
    x = LG.tile(base.to(DEV), idx)
    buf, view = LG.guarded((lc.n, c, h, w), torch.float32, DEV)
    ops._call('dts_nhwc_to_nchw', x.data_ptr(), ops.dt_code(dt), view.data_ptr(), lc.n, c, h, w)
    _exact(lc, 'out', _check_rows(lc, 'out', view, idx, buf), base.permute(0, 3, 1, 2).float().contiguous())


def _split_image(ops, lc, idx, which):
    h, w, c = _shape(lc, 'x')
    base = torch.randn(LG.K, h, w, c, generator=_gen(lc)) * 2
    base[1] *= 2.0 ** -10          # lo halves near the f16 subnormals
    x = LG.tile(base.to(DEV), idx)
    buf, view = LG.guarded((lc.n, h, w, 2 * c), torch.float16, DEV)
    if which == 3:
        ops._call('dts_split3_f16', x.data_ptr(), c, None, 0, view.data_ptr(), lc.n * h * w)
        want = RS.x3_image(base.numpy())
    else:
        ops._call('dts_split2_f16', x.data_ptr(), c, view.data_ptr(), lc.n * h * w)
        want = RS.x2_image(base.numpy())
    first = _check_rows(lc, 'image', view, idx, buf)
    _exact(lc, 'image bits', first.view(torch.int16), torch.from_numpy(want.view('int16').copy()))


@row_op
def split3_f16(ops, lc, idx):
    _split_image(ops, lc, idx, 3)


@row_op
def split2_f16(ops, lc, idx):
    _split_image(ops, lc, idx, 2)


def _resample(ops, lc, idx, kind, entry, up, fn):
    dt = DT[lc.spec['mode']]
    base64 = RS.lattice(kind, (LG.K,) + _shape(lc, 'x'), seed=sum(ord(ch) for ch in lc.name))
    base = torch.from_numpy(base64).to(dt)
    assert torch.equal(base.double(), torch.from_numpy(base64))
    x = LG.tile(base.to(DEV), idx)
    h, w, c = _shape(lc, 'x')
    buf, view = LG.guarded((lc.n,) + _shape(lc, 'out'), dt, DEV)
    ops._call(entry, x.data_ptr(), view.data_ptr(), ops.dt_code(dt), lc.n, h, w, c, up, *((0,) if entry == 'dts_resample_fir' else ()))
    want = torch.from_numpy(fn(base64))
    assert torch.equal(want.to(dt).double(), want)
    _exact(lc, 'out', _check_rows(lc, 'out', view, idx, buf), want.to(dt))


@row_op
def resample2x_up_bf16(ops, lc, idx):
    _resample(ops, lc, idx, 'box_up', 'dts_resample2x', 1, RS.nearest_up)


@row_op
def resample2x_down_f16(ops, lc, idx):
    _resample(ops, lc, idx, 'box_down', 'dts_resample2x', 0, RS.mean2x2_down)


@row_op
def resample_fir_up_f16(ops, lc, idx):
    _resample(ops, lc, idx, 'fir_up', 'dts_resample_fir', 1, RS.fir_up)


@row_op
def resample_fir_down_bf16(ops, lc, idx):
    _resample(ops, lc, idx, 'fir_down', 'dts_resample_fir', 0, RS.fir_down)


def _sigmas():
    return torch.tensor([E.SIGMAS[k % 4] * (1 + k // 4) for k in range(LG.K)], dtype=torch.float64)


@row_op
def edm_precond_in(ops, lc, idx):
    chw = _shape(lc, 'x')[0]
    base = torch.randn(LG.K, chw, generator=_gen(lc), dtype=torch.float64) * 80
    sig = _sigmas()
    x, sg = LG.tile(base.to(DEV), idx), LG.tile(sig.to(DEV), idx)
    buf, view = LG.guarded((lc.n, chw), torch.float32, DEV)
    cbuf, coef = LG.guarded((lc.n, 4), torch.float32, DEV)
    ops._call('dts_edm_precond_in', x.data_ptr(), sg.data_ptr(), lc.n, 0.5, view.data_ptr(), coef.data_ptr(), lc.n, chw)
    (xin, bx), (cf, bc) = E.precond_in_ref(base, sig, 0.5)
    _bounded(lc, 'xin', _check_rows(lc, 'xin', view, idx, buf), xin, bx)
    _bounded(lc, 'coef', _check_rows(lc, 'coef', coef, idx, cbuf), cf, bc)


@row_op
def edm_precond_out(ops, lc, idx):
    chw = _shape(lc, 'x')[0]
    gen = _gen(lc)
    base, F = torch.randn(LG.K, chw, generator=gen, dtype=torch.float64) * 80, torch.randn(LG.K, chw, generator=gen)
    coef = E.precond_in_ref(base, _sigmas(), 0.5)[1][0].float()
    x, Fd, cd = LG.tile(base.to(DEV), idx), LG.tile(F.to(DEV), idx), LG.tile(coef.to(DEV), idx)
    buf, view = LG.guarded((lc.n, chw), torch.float32, DEV)
    ops._call('dts_edm_precond_out', x.data_ptr(), Fd.data_ptr(), cd.data_ptr(), view.data_ptr(), lc.n, chw)
    ref, bound = E.precond_out_ref(base, F, coef)
    _bounded(lc, 'D', _check_rows(lc, 'D', view, idx, buf), ref, bound)


def _heun_base(lc):
    chw, gen = _shape(lc, 'x_hat')[0], _gen(lc)
    x = 10.0 * torch.arange(1, LG.K + 1, dtype=torch.float64)[:, None] + 0.25 * torch.rand(LG.K, chw, generator=gen, dtype=torch.float64)
    sched = E.sigma_schedule()
    steps = [(0, 3, 8, 12, 15, 16, 1)[k] for k in range(LG.K)]
    th = torch.tensor([E.churned(float(sched[i]))[0] for i in steps], dtype=torch.float64)
    tn = torch.tensor([float(sched[i + 1]) for i in steps], dtype=torch.float64)
    nc = torch.tensor([E.churned(float(sched[i]))[1] for i in steps], dtype=torch.float64)
    return chw, gen, x, th, tn, nc


def _per_row(fn, *rows):
    """a scalar-step reference applied row by row: [(ref, bound), ...] stacked"""
    parts = [fn(k) for k in range(LG.K)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


@row_op
def heun_xhat_rows(ops, lc, idx):
    chw, gen, x, th, tn, nc = _heun_base(lc)
    nc[2] = 0.0                                                                  # a row without churn: its source row, bit for bit
    eps = torch.randn(LG.K, chw, generator=gen)
    xd, ed, cd = LG.tile(x.to(DEV), idx), LG.tile(eps.to(DEV), idx), LG.tile(nc.to(DEV), idx)
    buf, view = LG.guarded((lc.n, chw), torch.float64, DEV)
    ops._call('dts_heun_xhat_rows', xd.data_ptr(), lc.n, 0, ed.data_ptr(), 1, cd.data_ptr(), view.data_ptr(), lc.n, chw)
    first = _check_rows(lc, 'x_hat', view, idx, buf)
    ref, bound = _per_row(lambda k: E.heun_xhat_ref(x[k:k + 1], eps[k:k + 1], float(nc[k]), 1, False))
    _bounded(lc, 'x_hat', first, ref, bound)
    assert torch.equal(first[2], x[2])


@row_op
def heun_euler_rows(ops, lc, idx):
    chw, gen, x, th, tn, nc = _heun_base(lc)
    D = torch.randn(LG.K, chw, generator=gen)
    xd, Dd, thd, tnd = (LG.tile(t.to(DEV), idx) for t in (x, D, th, tn))
    dbuf, dview = LG.guarded((lc.n, chw), torch.float64, DEV)
    xbuf, xview = LG.guarded((lc.n, chw), torch.float64, DEV)
    ops._call('dts_heun_euler_rows', xd.data_ptr(), Dd.data_ptr(), thd.data_ptr(), tnd.data_ptr(), dview.data_ptr(), xview.data_ptr(), lc.n, chw)
    refs = [E.heun_euler_ref(x[k:k + 1], D[k:k + 1], float(th[k]), float(tn[k])) for k in range(LG.K)]
    _bounded(lc, 'd_cur', _check_rows(lc, 'd_cur', dview, idx, dbuf), torch.cat([r[0][0] for r in refs]), torch.cat([r[0][1] for r in refs]))
    _bounded(lc, 'x_next', _check_rows(lc, 'x_next', xview, idx, xbuf), torch.cat([r[1][0] for r in refs]), torch.cat([r[1][1] for r in refs]))


@row_op
def heun_correct_rows(ops, lc, idx):
    chw, gen, x, th, tn, nc = _heun_base(lc)
    D2 = torch.randn(LG.K, chw, generator=gen)
    d_cur = torch.randn(LG.K, chw, generator=gen, dtype=torch.float64)
    x_next = x + (tn - th)[:, None] * d_cur
    xd, Dd, dd, thd, tnd = (LG.tile(t.to(DEV), idx) for t in (x, D2, d_cur, th, tn))
    buf, view = LG.guarded((lc.n, chw), torch.float64, DEV)
    LG.tile(x_next.to(DEV), idx, out=view)                                       # in place on x_next
    assert LG.bands_intact(buf)
    ops._call('dts_heun_correct_rows', xd.data_ptr(), Dd.data_ptr(), dd.data_ptr(), thd.data_ptr(), tnd.data_ptr(), view.data_ptr(), lc.n, chw)
    ref, bound = _per_row(lambda k: E.heun_correct_ref(x[k:k + 1], D2[k:k + 1], d_cur[k:k + 1], float(th[k]), float(tn[k]), x_next[k:k + 1]))
    _bounded(lc, 'x_next', _check_rows(lc, 'x_next', view, idx, buf), ref, bound)


@row_op
def candidate_noise_rows(ops, lc, idx):
    """one candidate of n images (b = n): row s is built from pivot[s], with its own mode and scale"""
    chw, gen = _shape(lc, 'g')[0], _gen(lc)
    pivot, g = (torch.randn(LG.K, chw, generator=gen, dtype=torch.float64) for _ in range(2))
    mode = torch.tensor([1, 0, 1, 1, 0, 1, 1], dtype=torch.int32)
    scale = torch.tensor([0.25, 9.0, 0.0, 2.5, 0.3, 0.731, 12.0], dtype=torch.float32)
    pd, gd, md, sd = (LG.tile(t.to(DEV), idx) for t in (pivot, g, mode, scale))
    buf, view = LG.guarded((lc.n, chw), torch.float64, DEV)
    ops._call('dts_candidate_noise_rows', pd.data_ptr(), gd.data_ptr(), md.data_ptr(), sd.data_ptr(), view.data_ptr(), lc.n, lc.n, chw)
    ref, bound = _per_row(lambda k: E.candidate_noise_ref(pivot[k:k + 1], g[k:k + 1], mode[k:k + 1], scale[k:k + 1]))
    _bounded(lc, 'candidates', _check_rows(lc, 'out', view, idx, buf), ref, bound)


@row_op
def layer_norm_bf16(ops, lc, idx):
    """reference and bound: those of test_gpu_sd_unet_ops.test_layer_norm, row classes included"""
    dt = DT[lc.spec['mode']]
    rows, c = _shape(lc, 'x')
    gen = _gen(lc)
    x = torch.randn(LG.K, rows, c, generator=gen) * 1.5 + 0.3
    x[1, 1] = 100.0 + 0.5 * torch.randn(c, generator=gen)
    x[2, 2] = -3.0e3 + 40.0 * torch.randn(c, generator=gen)
    x[3, 3] = 1e-3 * torch.randn(c, generator=gen)
    x = x.to(dt)
    gamma, beta, eps = 1.0 + 0.3 * torch.randn(c, generator=gen), 0.2 * torch.randn(c, generator=gen), 1e-5
    xd = LG.tile(x.to(DEV), idx)
    buf, view = LG.guarded((lc.n, rows, c), dt, DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    ops._call('dts_layer_norm', xd.data_ptr(), view.data_ptr(), ops.dt_code(dt), lc.n * rows, c, eps, gd.data_ptr(), bd.data_ptr())
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    m = x64.mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + eps)
    xhat = (x64 - m) * r
    ref = xhat * g64 + b64
    u, e32 = TU.U[dt], 2.0 ** -24
    dm = 40 * e32 * x64.abs().amax(-1, keepdim=True)
    bound = u * ref.abs() + g64.abs() * (r * dm * (1 + xhat.abs()) + 2.0 ** -19 * xhat.abs()) + 2.0 ** -22 * (ref.abs() + b64.abs())
    _bounded(lc, 'out', _check_rows(lc, 'out', view, idx, buf), ref, bound)


@row_op
def geglu_f16(ops, lc, idx):
    """reference and bound: those of test_gpu_sd_unet_ops.test_geglu"""
    dt = DT[lc.spec['mode']]
    rows, two_inner = _shape(lc, 'x')
    inner = two_inner // 2
    x = torch.rand(LG.K, rows, two_inner, generator=_gen(lc)) * 20 - 10
    x[0, 0, inner:inner + 8] = torch.tensor([-10.0, 10.0, 0.0, -0.0, -6.0, -1e-3, 1e-3, 3.0])
    x[0, 0, :8] = 10.0
    x = x.to(dt)
    xd = LG.tile(x.to(DEV), idx)
    buf, view = LG.guarded((lc.n, rows, inner), dt, DEV)
    ops._call('dts_geglu', xd.data_ptr(), view.data_ptr(), ops.dt_code(dt), lc.n * rows, inner)
    x64 = x.double()
    a, gate = x64[..., :inner], x64[..., inner:]
    Phi = 0.5 * torch.special.erfc(-gate / math.sqrt(2.0))
    ref = a * gate * Phi
    sens = gate.abs() * (torch.exp(-0.5 * gate * gate) / math.sqrt(2 * math.pi)) / Phi
    bound = (TU.U[dt] + 2.0 ** -19 + 1.5 * 2.0 ** -24 * sens) * ref.abs() + (2.0 ** -25 if dt == torch.float16 else 0.0)
    first = _check_rows(lc, 'out', view, idx, buf)
    err = (first.double() - ref).abs()
    print(f'  {lc.name}: max err {float(err.max()):.3e}, max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}')
    assert bool((err <= bound).all())


@row_op
def xattn_f16_kv_rows(ops, lc, idx):
    """dts_cross_attention with kv_rows over 2 contexts: the context of a row follows its class (k % 2), so classes stay classes"""
    s = lc.spec
    dt, heads, d, tq, tk = DT[s['mode']], s['heads'], s['d'], s['tq'], s['tk']
    c, scale, gen = heads * d, 1.0 / math.sqrt(d), _gen(lc)
    q = (torch.randn(LG.K, tq, c, generator=gen) * 1.5).to(dt)
    kv = torch.randn(s['contexts'], tk, 2 * c, generator=gen).to(dt)
    rows = (torch.arange(LG.K) % s['contexts']).to(torch.int32)
    qd, rd = LG.tile(q.to(DEV), idx), LG.tile(rows.to(DEV), idx)
    buf, view = LG.guarded((lc.n, tq, c), dt, DEV)
    assert ops.cross_attention(qd, kv.to(DEV), heads, scale, kv_rows=rd, out=view) is view
    assert LR.xattn_plan(lc.n, heads, tq)[1] == 8                                # the chunk loop at its widest
    ref, bound = TU.xattn_reference(q, kv, heads, scale, dt, rows)
    first = _check_rows(lc, 'out', view, idx, buf)
    ratio = float(((first.double() - ref).abs() / bound).max())
    print(f'  {lc.name}: max err / bound {ratio:.3f}')
    assert ratio <= 1.0


@pytest.mark.parametrize('lc', _cases('rows'), ids=lambda c: c.name)
def test_row_kernels(ops, lc):
    assert lc.spec['op'] in ROW_OPS
    ROW_OPS[lc.spec['op']](ops, lc, _begin(lc))


def test_every_row_case_has_its_adapter():
    assert {c.spec['op'] for c in _cases('rows')} == set(ROW_OPS)


# ---- gelu, the DDIM / SD candidate builders, and the kernels with documented caps, run just under them ----------------------------------------
def _gelu(ops, lc, idx):
    """reference and bound: those of test_gpu_clip_vision_ops.test_gelu, its special values in every base row"""
    dt, kind = DT[lc.spec['mode']], lc.spec['kind']
    m = _shape(lc, 'x')[0]
    big = torch.finfo(dt).max
    special = torch.tensor([20.0, -20.0, big, -big, 0.0, -0.0, 1.0, -1.0, 6.0, -6.0, 1e-3, -1e-3])
    x = torch.randn(LG.K, m, generator=_gen(lc)) * 2.5
    x[:, :special.numel()] = special
    x[:, -special.numel():] = special.flip(0)
    x = x.to(dt)
    xd = LG.tile(x.to(DEV), idx)
    buf, view = LG.guarded((lc.n, m), dt, DEV)
    assert ops.gelu(xd, kind, out=view) is view
    x64, u = x.double(), TV.U[dt]
    if kind == 'quick_gelu':
        z = 1.702 * x64
        ref = x64 * torch.sigmoid(z)
        sens = z.abs() * torch.sigmoid(-z)
        bound = (u + 2.0 ** -20 + 2 * TV.E32 * sens) * ref.abs() + TV.SUB[dt] + torch.where(z < -87.0, ref.abs(), torch.zeros_like(ref))
    else:
        Phi = 0.5 * torch.special.erfc(-x64 / math.sqrt(2.0))
        ref = x64 * Phi
        phi = torch.exp(-0.5 * x64 * x64) / math.sqrt(2 * math.pi)
        sens = torch.where(Phi > 0, x64.abs() * phi / Phi.clamp_min(1e-300), torch.zeros_like(x64))
        bound = (u + 2.0 ** -19 + 1.5 * TV.E32 * sens) * ref.abs() + TV.SUB[dt] + torch.where(Phi < 2.0 ** -120, ref.abs(), torch.zeros_like(ref))
    first = _check_rows(lc, 'out', view, idx, buf)
    assert bool(torch.isfinite(first).all())
    worst = float(((first.double() - ref).abs() / bound).max())
    print(f'  {lc.name} [{kind}]: max err / bound {worst:.3f}')
    assert worst <= 1.0


@row_op
def gelu_erf_bf16(ops, lc, idx):
    _gelu(ops, lc, idx)


@row_op
def quick_gelu_f16(ops, lc, idx):
    _gelu(ops, lc, idx)


@row_op
def ddim_candidates_groups_bf16(ops, lc, idx):
    """one group per row: x, e [n, m], z and prev [n, ncand, m]"""
    dt, ncand, m, gen = DT[lc.spec['mode']], lc.spec['ncand'], _shape(lc, 'x')[0], _gen(lc)
    at, ap = E.ALPHAS[1]
    st = E.ddim_sigma(at, ap, 1.0)
    x, e = (torch.randn(LG.K, m, generator=gen).to(dt) for _ in range(2))
    z = torch.randn(LG.K, ncand, m, generator=gen).to(dt)
    xd, ed, zd = (LG.tile(t.to(DEV), idx) for t in (x, e, z))
    pbuf, prev = LG.guarded((lc.n, ncand, m), dt, DEV)
    xbuf, x0 = LG.guarded((lc.n, m), dt, DEV)
    got = ops.ddim_candidates_groups(xd, ed, zd, at, ap, st, out=prev, x0_out=x0)
    assert got[0] is prev and got[1] is x0
    fp, fx = _check_rows(lc, 'prev', prev, idx, pbuf), _check_rows(lc, 'x0', x0, idx, xbuf)
    for k in range(LG.K):
        (rp, bp), (rx, bx) = E.ddim_ref(x[k], e[k], z[k], at, ap, st)
        _bounded(lc, f'prev, group {k}', fp[k], rp, E.rounded_bound(rp, bp, dt))
        _bounded(lc, f'x0, group {k}', fx[k], rx, E.rounded_bound(rx, bx, dt))


@row_op
def ddim_candidates_f16(ops, lc, idx):
    """the single-pair form over the whole batch as ONE pair of n * m elements (deterministic step: no z, no x0)"""
    dt, m, gen = DT[lc.spec['mode']], _shape(lc, 'x')[0], _gen(lc)
    at, ap = E.ALPHAS[2]
    x, e = (torch.randn(LG.K, m, generator=gen).to(dt) for _ in range(2))
    xd, ed = LG.tile(x.to(DEV), idx), LG.tile(e.to(DEV), idx)
    buf, view = LG.guarded((lc.n, m), dt, DEV)
    ops._call('dts_ddim_candidates', xd.data_ptr(), ed.data_ptr(), None, view.data_ptr(), None, ops.dt_code(dt), float(at), float(ap), 0.0, 1, xd.numel())
    (rp, bp), _ = E.ddim_ref(x, e, None, at, ap, 0.0)
    _bounded(lc, 'prev', _check_rows(lc, 'prev', view, idx, buf), rp[0], E.rounded_bound(rp[0], bp[0], dt))


def _sd_candidates(lc, rows_form):
    """base rows and the reference expression of test_gpu_sd_rows_ops.sd_rows_case (pipeline_stable_diffusion.py:1377-1379), row by row"""
    dt, shape, gen = DT[lc.spec['mode']], _shape(lc, 'u'), _gen(lc)
    count = LG.numel(shape)
    pivot = torch.randn((LG.K if rows_form else 1,) + shape, generator=gen).to(dt)
    u = torch.randn((LG.K,) + shape, generator=gen).to(dt)
    mode = torch.tensor([1, 0, 1, 1, 0, 1, 1], dtype=torch.int32)
    rands = torch.rand(LG.K, generator=gen).tolist()
    lam, root = 0.15, float(count) ** 0.5
    scale = torch.tensor([[r, lam, root] if mo else [0.0, 0.0, 0.0] for r, mo in zip(rands, mode.tolist())], dtype=torch.float32)
    want = torch.stack([u[k] if mode[k] == 0 else pivot[k if rows_form else 0] + u[k] / torch.norm(u[k]) * rands[k] * lam * root for k in range(LG.K)])
    return dt, shape, pivot, u, mode, scale, want


@row_op
def candidate_noise_sd_rows_f16(ops, lc, idx):
    """n searches of one candidate each: row s reads pivot[s]"""
    dt, shape, pivot, u, mode, scale, want = _sd_candidates(lc, True)
    pd, ud, md, sd = (LG.tile(t.to(DEV), idx) for t in (pivot, u, mode, scale))
    buf, view = LG.guarded((lc.n,) + shape, dt, DEV)
    assert ops.candidate_noise_sd_rows(pd, ud, md, sd, out=view) is view
    _exact(lc, 'candidates (the reference expression in float16)', _check_rows(lc, 'out', view, idx, buf), want)


@row_op
def candidate_noise_sd_f16(ops, lc, idx):
    """one search of n candidates: every row reads the one pivot"""
    dt, shape, pivot, u, mode, scale, want = _sd_candidates(lc, False)
    ud, md, sd = (LG.tile(t.to(DEV), idx) for t in (u, mode, scale))
    pd = pivot.to(DEV)
    buf, view = LG.guarded((lc.n,) + shape, dt, DEV)
    ops._call('dts_candidate_noise_sd', pd.data_ptr(), ud.data_ptr(), md.data_ptr(), sd.data_ptr(), view.data_ptr(), ops.dt_code(dt), lc.n, pd.numel())
    _exact(lc, 'candidates (the reference expression in float16)', _check_rows(lc, 'out', view, idx, buf), want)


@row_op
def jpeg_size_cap(ops, lc, idx):
    """dts_jpeg_size at the most blocks one call takes (n * blocks per image <= 2^24; one more image is refused, asked launch-free on the CPU):
    the workspace passes 2^32 bytes, the bit buffer ends just under it.  Sizes equal Pillow's, as in test_gpu_jpeg.py."""
    import numpy as np
    from diffusion_tts_amd import _lib
    import jpeg_helpers as JH
    h, w = lc.spec['h'], lc.spec['w']
    lib = _lib.load()
    lay = LR.jpeg_layout(lc.n, h, w)
    need = int(lib.dts_jpeg_workspace_bytes(lc.n, h, w))
    assert LR.jpeg_shape_ok(lc.n, h, w) and not LR.jpeg_shape_ok(lc.n + 1, h, w) and lc.n * lay.nb <= lc.spec['cap_blocks'] < (lc.n + 1) * lay.nb
    assert need == lay.bytes > LG.B32 and int(lib.dts_jpeg_workspace_bytes(lc.n + 1, h, w)) == 0
    imgs = np.concatenate([JH.make_images(kind, 2, h, w) for kind in ('noise', 'smooth', 'sat', 'flat')])[:LG.K]
    want = torch.tensor([len(JH.pil_jpeg(im, 80)) for im in imgs], dtype=torch.int32)
    x = LG.tile(torch.from_numpy(imgs).to(DEV), idx)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    qtab = torch.tensor(ops.jpeg_quant_tables(80), dtype=torch.int16).to(DEV)
    buf, view = LG.guarded((lc.n, 1), torch.int32, DEV)
    ops._call('dts_jpeg_size', x.data_ptr(), view.data_ptr(), lc.n, h, w, qtab.data_ptr(), ws.data_ptr(), ws.numel(), None)
    print(f'  {lc.name}: {lc.n * lay.nb} blocks of 2^24; workspace {need} B, bit buffer at [{lay.bitbuf}, {lay.bytes})')
    _exact(lc, 'sizes (Pillow)', _check_rows(lc, 'sizes', view, idx, buf)[:, 0], want)


@row_op
def group_rows_cap(ops, lc, idx):
    """dts_group_rows at its 1024 rows, 4 MiB each: the last 7 rows lie beyond byte 2^32.  Rows of a class differ in a stamp (their index in the
    first 16 bytes), except the 7 rows beyond 2^32 bytes, which are twins of their class's first row: the expected grouping follows from the map."""
    assert lc.n == ops.GROUP_ROWS_MAX == lc.spec['cap_rows']
    m = _shape(lc, 'rows')[0]
    base = torch.randint(-2 ** 31, 2 ** 31 - 1, (LG.K, m), generator=_gen(lc), dtype=torch.int32)
    x = LG.tile(base.to(DEV), idx)
    first_of = LG.first_rows(idx)
    stamp = torch.arange(lc.n, dtype=torch.int32)
    twins = list(range(lc.n - 7, lc.n))
    assert all(t * m * 4 >= LG.B32 for t in twins)
    for t in twins:
        stamp[t] = stamp[first_of[idx[t]]]
    x[:, 0] = stamp.to(DEV)
    earliest = [int(first_of[idx[t]]) if t in twins else t for t in range(lc.n)]
    firsts = [t for t in range(lc.n) if earliest[t] == t]
    number = {t: g for g, t in enumerate(firsts)}
    want_slot = torch.tensor([number[earliest[t]] for t in range(lc.n)], dtype=torch.int32)
    want_reps = torch.tensor(firsts + [-1] * (lc.n - len(firsts)), dtype=torch.int32)
    slot, reps, count = ops.group_rows(x)
    torch.cuda.synchronize()
    print(f'  {lc.name}: {len(firsts)} groups of {lc.n} rows; twins {twins}')
    assert int(count.cpu()) == len(firsts) == lc.n - 7
    assert torch.equal(slot.cpu(), want_slot) and torch.equal(reps.cpu(), want_reps)
