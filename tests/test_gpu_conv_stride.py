"""The stride-2 form of the 3x3 convolution (ops.conv2d(stride=2): dts_conv_args.up == -1, conv_igemm_kernel<.., S2 = true>) by the method of
tests/test_gpu_conv.py, with the float64 helpers of tests/conv_reference.py.

REFERENCE.  The stride-1, padding-1 float64 result (conv_reference.tap_sums of the concatenated input) taken at [..., ::2, ::2], then
conv_reference.epilogue: output pixel (i, j) of a stride-2 padding-1 convolution IS stride-1 pixel (2i, 2j), so nothing here knows of a
stride, and nothing shares code with the kernel.

EXACT LEG (test_exact).  The sparse integer inputs of conv_reference.exact_inputs (activations {0, +-1, +-2}, weights {0, +-1}, integer
epilogue operands) under conv_reference.assert_exact_conditions: the output must EQUAL the reference bit for bit, in float16 and bfloat16,
inside a NaN-guarded buffer (every element written, the bands untouched).  Strip statistics, where the output has whole 64-pixel strips,
equal the float64 moments of the stored output; elsewhere `_gn_stats` is None.  Every case pins its K split and asserts the plan's tile /
waves / ring depth / split, so each of the 12 instantiated forms per type (cout tile 64 | 128 | 192 x 4 | 8 waves x 2- | 3-deep ring) is
known to have run; a forced split first asserts that the reference CHANGES when the last split's weights are zeroed
(conv_reference.last_split_mask), so a launch that skipped its last split cannot pass.

SAME ANSWER AS THE EXISTING ROUTE (test_equals_space_to_depth_route): on two even-sized cases the same inputs through
ops.space_to_depth2 + ops.stride2_conv_weight + ops.conv2d give the identical tensor.

ROUNDING LEG (test_rounding).  Gaussian operands rounded to the storage type, one representative per form (plain, split-K, concat, 8-wave),
per element against the bound tests/test_gpu_conv.py derives (its docstring): |got - o| <= 1.001 u |o| + 2 (K + 8) 2^-24 S.

Record of a run on an MI355X (max err / bound; a record, NOT the source of the bound):
    plain bf16 0.907, f16 0.648; split-K bf16 0.754, f16 0.347; concat bf16 0.780, f16 0.371; 8-wave bf16 0.850, f16 0.389"""
import functools
import math

import pytest
import torch

import conv_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD = 4096
MODES = R.H16
U = {'bf16': 2.0 ** -8, 'f16': 2.0 ** -11}

CASES = {}


def _case(name, n, h, w, c1, cout, c2=0, ep='b', scale=1.0, stats=False, knobs=(), splits=1, form=None):
    """h, w: the INPUT size.  ep as conv_reference._case (b bias, n bias_nc, N bias_nc as a column slice, r residual -- at the OUTPUT size, so
    it is drawn here).  splits: 1 pinned unsplit, s > 1 forced, -1 the launcher's choice.  form: (waves, stages) the plan must name."""
    assert name not in CASES
    knobs = tuple(knobs) + ((('conv_splits', splits),) if splits > 0 else ())
    c = R.Case(name, 'igemm_splitk' if splits > 1 else 'igemm', MODES, n, h, w, c1, c2, cout, 3, False, ep.replace('r', ''), scale, stats, knobs,
               ('int',), False, None, False, splits, '')
    CASES[name] = (c, 'r' in ep, form)


# -- tiles: 2x8x8 -> 4x4 outputs (32 pixels: no strip, `_gn_stats` None)
for _t in (64, 128, 192):
    _case(f'tile{_t}', 2, 8, 8, 64, _t, stats=True)
# -- statistics and whole tiles: 8x32 outputs, the shift path, 256 pixels = 4 strips, residual through the early residual fetch
_case('shift_1x16x64', 1, 16, 64, 64, 128, ep='bnr', scale=0.5, stats=True)
_case('shift_1x16x64_tile64', 1, 16, 64, 64, 64, ep='bnr', scale=0.5, stats=True)
# -- odd and degenerate sizes: the division path, live bottom / right taps where an even size has padding
_case('odd_3x5x7', 3, 5, 7, 64, 64, ep='bnr', stats=True)
_case('odd_2x7x9', 2, 7, 9, 64, 128, ep='br')
_case('image_1x1', 1, 1, 1, 64, 64)
_case('h_is_1', 1, 1, 40, 64, 128)
_case('w_is_1', 2, 9, 1, 64, 64, ep='br', stats=True)
_case('even_odd_1x6x5', 1, 6, 5, 64, 192, ep='bn')
# -- tiles crossing rows and samples: 2 x 12 x 10 = 240 pixels
_case('rows_samples_2x24x20', 2, 24, 20, 64, 128, ep='bn')
# -- grids of 1, 3, 7, 9 and 13 blocks (the XCD remap's remainder branch); outputs 6x9, 12x25, 24x35, 2x12x16, 40x41
_case('grid1', 1, 12, 18, 64, 192)
_case('grid3', 1, 23, 49, 64, 192, ep='bn')
_case('grid7', 1, 47, 69, 64, 128, ep='br')
_case('grid9', 2, 24, 32, 64, 576, ep='bnr', stats=True)
_case('grid13', 1, 79, 81, 64, 128)
# -- concat
_case('cat_64_128', 2, 11, 13, 64, 128, c2=128, ep='br')
_case('cat_128_64', 2, 12, 14, 128, 128, c2=64)
# -- K loop: 9 steps (c 64) and 27 steps (c 192), forced splits 2, 3, 8 (9 steps: 5 + 4, 3 + 3 + 3, unsplit -- nk < 16; 27 steps: 14 + 13,
# 9 + 9 + 9, six of 4 and one of 3); 2x16x16 -> 2 strips
for _s in (2, 3, 8):
    for _nk, _c in ((9, 64), (27, 192)):
        _case(f'split{_s}_nk{_nk}', 2, 16, 16, _c, 128, splits=_s)
        _case(f'split{_s}_nk{_nk}_stats', 2, 16, 16, _c, 128, ep='bnr', scale=0.5, stats=True, splits=_s)
_case('split3_full', 2, 16, 16, 192, 192, ep='bNr', scale=0.5, stats=True, splits=3)
_case('split2_ragged', 3, 9, 13, 128, 64, ep='bnr', stats=True, splits=2)
_case('split2_cat', 2, 16, 16, 64, 128, c2=128, stats=True, splits=2)
# -- the launcher's own choice
_case('auto_c128', 2, 16, 16, 128, 128, ep='bnr', stats=True, splits=-1)
# -- every instantiated form: cout picks the tile, the knobs the waves and the ring depth
for _t in (64, 128, 192):
    for _wv in (4, 8):
        for _st in (2, 3):
            _case(f'form_tile{_t}_waves{_wv}_ring{_st}', 2, 16, 16, 128, _t, ep='br', stats=True, knobs=(('conv_waves', _wv), ('conv_stages', _st)),
                  form=(_wv, _st))
_case('form_waves8_ring3_split3', 2, 16, 16, 192, 192, ep='bnr', stats=True, knobs=(('conv_waves', 8), ('conv_stages', 3)), splits=3, form=(8, 3))
_case('form_waves4_ring2_split2', 2, 15, 17, 128, 128, ep='bn', knobs=(('conv_waves', 4), ('conv_stages', 2)), splits=2, form=(4, 2))
_case('form_ring4_runs_ring3', 2, 16, 16, 128, 128, ep='b', knobs=(('conv_waves', 4), ('conv_stages', 4)), form=(4, 3))
for _t in (64, 128):
    _case(f'knob_tile{_t}', 1, 16, 32, 64, 384, ep='bnr', knobs=(('conv_tile', _t),))


def out_hw(case):
    return (case.h + 1) // 2, (case.w + 1) // 2


def reference(a):
    """the stride-1 float64 tap sums at every second row and column, then the epilogue"""
    o, s = R.tap_sums(R.prepare_input(a['x1'], a['x2']), a['w'].double())
    return R.epilogue(o[..., ::2, ::2], s[..., ::2, ::2], a['bias'], a['bias_nc'], a['residual'], a['out_scale'])


def _with_residual(a, case, has_res, draw):
    if has_res:
        ho, wo = out_hw(case)
        a['residual'] = draw((case.n, case.cout, ho, wo))
    return a


@functools.lru_cache(maxsize=None)
def _exact(name):
    case, has_res, _ = CASES[name]
    gen = torch.Generator().manual_seed(4242 + len(name))
    a = _with_residual(R.exact_inputs(case, 'f16', 0, 'int'), case, has_res, lambda shape: R._ints(gen, shape))
    return a, reference(a)


@functools.lru_cache(maxsize=None)
def _gauss(name, mode):
    case, has_res, _ = CASES[name]
    gen = torch.Generator().manual_seed(99)
    a = _with_residual(R.gaussian_inputs(case, mode), case, has_res, lambda shape: torch.randn(shape, generator=gen).to(R.STORE[mode]).double())
    return a, reference(a)


class _Knobs:
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


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


def _operands(ops, case, mode, a):
    dt = R.STORE[mode]
    dev = lambda t: None if t is None else t.to(dt).to(DEV).contiguous()
    x1 = dev(R.nhwc(a['x1']))
    x2 = None if a['x2'] is None else dev(R.nhwc(a['x2']))
    wp = ops.pack_conv_weight(a['w'].float().to(DEV), dt)
    bias = None if a['bias'] is None else a['bias'].float().to(DEV)
    bnc = None
    if a['bias_nc'] is not None:
        bnc = dev(a['bias_nc_wide'])[:, case.cout:] if 'N' in case.ep else dev(a['bias_nc'])
    res = None if a['residual'] is None else dev(R.nhwc(a['residual']))
    return x1, x2, wp, bias, bnc, res


def _launch(ops, name, mode, a, want_stats):
    """ops.conv2d(stride=2) of the case: (out NCHW on the CPU, statistics or None, the guard buffer, the plan)"""
    case, _, form = CASES[name]
    dt = R.STORE[mode]
    x1, x2, wp, bias, bnc, res = _operands(ops, case, mode, a)
    ho, wo = out_hw(case)
    numel = case.n * ho * wo * case.cout
    buf = torch.full((numel + 2 * GUARD,), float('nan'), dtype=dt, device=DEV)
    view = buf[GUARD:GUARD + numel].view(case.n, ho, wo, case.cout)
    call = dict(x2=x2, bias_nc=bnc, residual=res, out_scale=a['out_scale'], out=view, gn_stats=want_stats, stride=2)
    with _Knobs(case.knobs):
        assert ops.conv_kernel(x1, wp, x2=x2, residual=res, stride=2) == 0
        out = ops.conv2d(x1, wp, bias, **call)
        torch.cuda.synchronize()
        plan = ops.conv_plan(x1, wp, bias, **call)
    assert out.data_ptr() == view.data_ptr() and tuple(out.shape) == (case.n, ho, wo, case.cout)
    # the whole route: kernel, tile, the form the knobs ask for, the K split the table says, who wrote the statistics
    knobs = dict(case.knobs)
    tile = knobs.get('conv_tile', 192 if case.cout % 192 == 0 else 128 if case.cout % 128 == 0 else 64)
    assert (plan['refused'], plan['kernel'], plan['phases'], plan['tile'], plan['pf']) == (0, 0, 0, tile, 1)
    assert plan['n_pt'] == -(-(case.n * ho * wo) // (256 if tile == 64 else 128)) and plan['nblk'] == plan['n_pt'] * (case.cout // tile)
    assert plan['waves'] in (4, 8) and plan['stages'] in (2, 3)
    if form is not None:
        assert (plan['waves'], plan['stages']) == form
    if case.splits > 0:
        assert (plan['splits'], plan['ks_per_split']) == R.effective_splits(case, mode)
    assert plan['stats_written'] == int(out._gn_stats is not None)
    st = out._gn_stats
    return R.nchw(out.cpu()), (None if st is None else st.cpu()), buf.cpu(), plan


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(CASES))
def test_exact(ops, name, mode):
    case, has_res, form = CASES[name]
    a, ref = _exact(name)
    dt = R.STORE[mode]
    ho, wo = out_hw(case)
    want = ref.o.to(dt)
    assert tuple(want.shape) == (case.n, case.cout, ho, wo)
    stats64 = R.strip_stats64(want) if case.stats and (ho * wo) % 64 == 0 else None
    R.assert_exact_conditions(ref, dt, stats64, a)
    splits, per = R.effective_splits(case, mode) if case.splits > 1 else (1, 0)
    if splits > 1:          # zeroing the last split's K steps changes the reference: a launch that skipped that split cannot equal it
        masked = dict(a, w=a['w'] * R.last_split_mask(case, mode).permute(2, 0, 1)[None].double())
        assert not torch.equal(reference(masked).o, ref.o)
    got, st, buf, plan = _launch(ops, name, mode, a, case.stats)
    print(f'{name} [{mode}]: tile {plan["tile"]}, {plan["waves"]} waves, ring {plan["stages"]}, {plan["nblk"]} blocks, K split {plan["splits"]} x {plan["ks_per_split"]},'
          f' statistics by {"the epilogue" if plan["stats_in_kernel"] else "the reduce pass" if plan["stats_in_reduce"] else "nobody"}')
    if name.startswith('grid'):
        assert plan['nblk'] == int(name[4:])
    assert got.dtype == dt
    assert not bool(torch.isnan(got).any()), 'an output element was never written'
    assert torch.equal(got, want), f'{int((got != want).sum())} of {want.numel()} elements differ'
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), 'a store outside the output'
    if stats64 is None:
        assert st is None
    else:
        assert st is not None and tuple(st.shape) == (case.n * ho * wo // 64, case.cout, 2)
        assert torch.equal(st, stats64.float())


def test_every_instantiated_form_has_a_case():
    forms = {(dict(c.knobs).get('conv_tile', 192 if c.cout % 192 == 0 else 128 if c.cout % 128 == 0 else 64),) + f for c, _, f in CASES.values() if f}
    assert forms == {(t, wv, st) for t in (64, 128, 192) for wv in (4, 8) for st in (2, 3)}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['tile128', 'shift_1x16x64'])
def test_equals_space_to_depth_route(ops, name, mode):
    """the existing route -- space_to_depth2, the rearranged weight over 4*C channels (27 of its 36 slots zero), a stride-1 convolution -- on the
    exact inputs: the identical tensor (and the identical statistics)"""
    case, _, _ = CASES[name]
    a, ref = _exact(name)
    dt = R.STORE[mode]
    x1, x2, wp, bias, bnc, res = _operands(ops, case, mode, a)
    call = dict(bias_nc=bnc, residual=res, out_scale=a['out_scale'], gn_stats=case.stats)
    with _Knobs(case.knobs):
        strided = ops.conv2d(x1, wp, bias, stride=2, **call)
        w4 = ops.pack_conv_weight(ops.stride2_conv_weight(a['w'].float().to(DEV)), dt)
        assert tuple(w4.shape) == (case.cout, 3, 3, 4 * case.c1) and tuple(wp.shape) == (case.cout, 3, 3, case.c1)
        s2d = ops.conv2d(ops.space_to_depth2(x1, dt), w4, bias, **call)
        torch.cuda.synchronize()
    assert strided.shape == s2d.shape and torch.equal(strided, s2d)
    assert torch.equal(R.nchw(strided.cpu()), ref.o.to(dt))
    assert (strided._gn_stats is None) == (s2d._gn_stats is None)
    if strided._gn_stats is not None:
        assert torch.equal(strided._gn_stats, s2d._gn_stats)


def test_residual_is_at_the_output_size(ops):
    x = torch.zeros(1, 8, 8, 64, dtype=torch.float16, device=DEV)
    w = torch.zeros(64, 3, 3, 64, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match='residual shape'):
        ops.conv2d(x, w, stride=2, residual=torch.zeros(1, 8, 8, 64, dtype=torch.float16, device=DEV))
    out = ops.conv2d(x, w, stride=2, residual=torch.ones(1, 4, 4, 64, dtype=torch.float16, device=DEV))
    assert tuple(out.shape) == (1, 4, 4, 64) and bool((out == 1).all())
    assert tuple(ops.conv2d(x[:, :7, :5].contiguous(), w, stride=2).shape) == (1, 4, 3, 64)


ROUTES = [('plain', 'shift_1x16x64'), ('split-K', 'split3_full'), ('concat', 'cat_64_128'), ('8-wave', 'form_tile128_waves8_ring3')]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('route,name', ROUTES)
def test_rounding(ops, route, name, mode):
    case, _, _ = CASES[name]
    a, ref = _gauss(name, mode)
    got, st, buf, plan = _launch(ops, name, mode, a, False)
    K = 9 * (case.c1 + case.c2)
    bound = 1.001 * U[mode] * ref.o.abs() + 2.0 * (K + 8) * 2.0 ** -24 * ref.S
    err = (got.double() - ref.o).abs()
    ratio = float((err / bound).max())
    print(f'rounding {route} {name} [{mode}]: {plan["waves"]} waves, ring {plan["stages"]}, K split {plan["splits"]}, max err/bound = {ratio:.3f}')
    assert math.isfinite(ratio) and bool((err <= bound).all()), ratio
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())
