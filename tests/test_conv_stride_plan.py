"""CPU: the stride-2 form of dts_conv2d (dts_conv_args.up == -1: 3x3, zero padding 1, stride 2, hout = (hin + 1) / 2) as the launch plan
sees it -- dts_conv_plan and the queries are host logic, no GPU.  The form always runs on conv_igemm_kernel (kernel 0), its grid is counted in
OUTPUT pixels, the statistics follow hout * wout % 64, a K split appears under conv_splits, everything the form does not take is refused by
name, and ops.conv2d(stride=2) refuses the keyword combinations it cannot run before the library (or a GPU) is needed.  Before the form
existed -1 was read as "upsample": hout = 2 * hin, so every count below failed."""
import ctypes as C

import pytest
import torch

F32, BF16, F16, X3 = 0, 1, 2, 3
CONV_KNOBS = ('conv_tile', 'conv_splits', 'conv_variant', 'conv_stages', 'conv_waves')


@pytest.fixture(scope='module')
def L():
    from diffusion_tts_amd import _lib
    _lib.load()
    return _lib


class Knobs:
    def __init__(self, L, **knobs):
        self.L, self.knobs, self.old = L, knobs, {}

    def __enter__(self):
        lib = self.L.load()
        for k, v in self.knobs.items():
            self.old[k] = int(lib.dts_get_tuning(self.L.KNOBS[k]))
            self.L.set_tuning(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.L.set_tuning(k, v)
        return False


def conv_args(L, n, h, w, c1, cout, dtype=F16, up=-1, ksize=3, c2=0, stats=None, ws=True, **fields):
    """dts_conv_args as ops._conv2d_args fills them: a workspace, stats_out where the OUTPUT has whole 64-pixel strips (stats=None: by that
    rule).  Pointers are never dereferenced by the plan: 16 stands for 'present'."""
    a = L.ConvArgs()
    a.n, a.hin, a.win, a.c1, a.c2, a.cout, a.ksize, a.up, a.dtype = n, h, w, c1, c2, cout, ksize, up, dtype
    a.out_scale = 1.0
    if ws:
        a.workspace, a.workspace_bytes = 16, 96 << 20
    ho, wo = ((h + 1) // 2, (w + 1) // 2) if up == -1 else (h, w)
    if stats if stats is not None else (ho * wo) % 64 == 0:
        a.stats_out = 16
    for k, v in fields.items():
        setattr(a, k, v)
    return a


def plan(L, a):
    info = L.ConvPlanInfo()
    rc = L.load().dts_conv_plan(C.byref(a), C.byref(info))
    return rc, {f: int(getattr(info, f)) for f, _ in L.ConvPlanInfo._fields_}, L.load().dts_last_error().decode()


def queries(L, a):
    lib = L.load()
    return [lib.dts_conv_kernel(C.byref(a)), lib.dts_conv_fuses_gn(C.byref(a)), lib.dts_conv_folds_skip(C.byref(a)), lib.dts_conv_takes_phases(C.byref(a))]


SHAPES = [(2, 8, 8), (1, 16, 64), (3, 5, 7), (2, 7, 9), (1, 1, 1), (1, 1, 40), (2, 9, 1), (1, 6, 5), (2, 24, 20), (2, 64, 64), (1, 33, 31)]


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('cout', [64, 128, 192, 320])
@pytest.mark.parametrize('n,h,w', SHAPES)
def test_grid_and_statistics_are_counted_in_output_pixels(L, n, h, w, cout, dtype):
    ho, wo = (h + 1) // 2, (w + 1) // 2
    with Knobs(L, conv_splits=1):
        a = conv_args(L, n, h, w, 64, cout, dtype)
        rc, p, err = plan(L, a)
        assert rc == 0 and p['refused'] == 0, err
        assert queries(L, a) == [0, 0, 0, 0]
    tile = 192 if cout % 192 == 0 else 128 if cout % 128 == 0 else 64
    assert (p['kernel'], p['tile'], p['pf'], p['phases']) == (0, tile, 1, 0)
    assert p['n_ct'] == cout // tile
    assert p['n_pt'] == -(-(n * ho * wo) // (256 if tile == 64 else 128))
    assert p['nblk'] == p['n_ct'] * p['n_pt']
    assert p['waves'] in (4, 8) and p['stages'] in (2, 3) and p['threads'] == 64 * p['waves']
    assert p['lds_bytes'] == p['stages'] * (tile + (256 if tile == 64 else 128)) * 128
    assert (p['splits'], p['ks_per_split']) == (1, 9)
    assert p['stats_written'] == p['stats_in_kernel'] == int((ho * wo) % 64 == 0)


def test_splits_appear_under_conv_splits(L):
    for c1, s, want in ((64, 2, (2, 5)), (64, 3, (3, 3)), (64, 8, (1, 9)), (192, 2, (2, 14)), (192, 3, (3, 9)), (192, 8, (7, 4))):
        with Knobs(L, conv_splits=s):
            # 1x16x64 -> 8x32: whole strips, so the reduce pass writes the statistics; 3x5x7 -> 3x4: none to write
            rc, p, err = plan(L, conv_args(L, 1, 16, 64, c1, 128))
            assert rc == 0 and p['refused'] == 0 and (p['splits'], p['ks_per_split']) == want, (c1, s, p, err)
            assert (p['stats_in_kernel'], p['stats_in_reduce'], p['stats_written']) == ((1, 0, 1) if want[0] == 1 else (0, 1, 1))
            rc, q, err = plan(L, conv_args(L, 3, 5, 7, c1, 128))
            assert (q['splits'], q['ks_per_split'], q['stats_written']) == want + (0,)
            # no workspace, no split
            rc, r, err = plan(L, conv_args(L, 1, 16, 64, c1, 128, ws=False))
            assert r['splits'] == 1 and r['refused'] == 0
    rc, p, err = plan(L, conv_args(L, 2, 16, 16, 1280, 1280))           # the launcher's own choice on an SD-shaped layer: some split of 180 steps
    assert rc == 0 and p['refused'] == 0 and p['splits'] >= 1 and p['splits'] * p['ks_per_split'] >= 180 > (p['splits'] - 1) * p['ks_per_split']


def test_knobs(L):
    """conv_tile as for stride 1; waves 4 | 8 and ring depth 2 | 3 are the instantiated forms: conv_stages = 4 runs (and reports) the 3-deep ring"""
    for tile in (64, 128):
        with Knobs(L, conv_tile=tile, conv_splits=1):
            rc, p, _ = plan(L, conv_args(L, 1, 16, 32, 64, 384))
            assert (p['refused'], p['kernel'], p['tile'], p['n_ct'], p['n_pt']) == (0, 0, tile, 384 // tile, 1)
    for waves in (4, 8):
        for stages, runs in ((2, 2), (3, 3), (4, 3)):
            with Knobs(L, conv_waves=waves, conv_stages=stages, conv_splits=1):
                rc, p, _ = plan(L, conv_args(L, 2, 8, 8, 128, 128))
                assert (p['refused'], p['waves'], p['stages'], p['threads']) == (0, waves, runs, 64 * waves)
                rc, q, _ = plan(L, conv_args(L, 2, 8, 8, 128, 128, up=0))     # (stride 1 keeps its 4-deep ring with 4 waves)
                assert q['stages'] == (stages if (stages < 4 or waves == 4) else 3)


def test_never_the_ping_pong_kernel(L):
    """shapes the ping-pong kernel takes at stride 1 (16-bit 32x32 input, cout 192 / 128, forced with conv_variant = 1, and a grid large enough
    for its own rule) are kernel 0 at stride 2, whatever the output size"""
    for dtype in (F16, BF16):
        for (n, hw, cout) in ((1, 32, 192), (1, 32, 128), (4, 64, 192), (64, 64, 192)):
            with Knobs(L, conv_variant=1):
                assert queries(L, conv_args(L, n, hw, hw, 192, cout, dtype, up=0))[0] in (6, 4)
                a = conv_args(L, n, hw, hw, 192, cout, dtype)
                assert queries(L, a) == [0, 0, 0, 0]
                rc, p, err = plan(L, a)
                assert rc == 0 and (p['refused'], p['kernel'], p['gn'], p['sk'], p['fuses_gn'], p['folds_skip']) == (0, 0, 0, 0, 0, 0), err
            a = conv_args(L, n, hw, hw, 192, cout, dtype)
            assert queries(L, a) == [0, 0, 0, 0]


REFUSED = [
    (dict(dtype=F32, c1=64), 'DTS_F16 and DTS_BF16'),
    (dict(dtype=X3, c1=64), 'DTS_F16 and DTS_BF16'),
    (dict(ksize=1), 'needs ksize 3'),
    (dict(gn_coef=16), 'takes no gn_coef'),
    (dict(skip_c=64, skip_x=16, skip_w=16), 'takes no skip_*'),
    (dict(skip_c=64), 'takes no skip_*'),
    (dict(out_split2=1, stats=False), 'takes no out_split2'),
    (dict(acc_scale=0.5), 'takes no acc_scale'),
]


@pytest.mark.parametrize('fields,message', REFUSED, ids=[m for _, m in REFUSED])
def test_refusals_by_name(L, fields, message):
    for (n, h, w, cout) in ((2, 8, 8, 128), (1, 32, 32, 192), (3, 5, 7, 64)):
        kw = dict(fields)
        a = conv_args(L, n, h, w, kw.pop('c1', 128), cout, kw.pop('dtype', F16), ksize=kw.pop('ksize', 3), stats=kw.pop('stats', None), **kw)
        rc, p, err = plan(L, a)
        assert rc == 0 and p['refused'] == 1 and p['kernel'] == 0, (p, err)
        assert 'up = -1 (stride 2)' in err and message in err, err
        assert queries(L, a) == [0, 0, 0, 0]
        assert L.load().dts_conv2d(C.byref(a), None) != 0                  # refused before any pointer is looked at
        assert message in L.load().dts_last_error().decode()
    ok = conv_args(L, 2, 8, 8, 128, 128, acc_scale=1.0)                     # (0 and 1 both mean "none")
    assert plan(L, ok)[1]['refused'] == 0
    assert plan(L, conv_args(L, 2, 8, 8, 128, 128, up=-2))[1]['refused'] == 1


def test_second_input_residual_and_epilogue_operands_are_accepted(L):
    a = conv_args(L, 2, 7, 9, 64, 128, c2=128, residual=16, bias=16, bias_nc=16, ld_bias_nc=128, out_scale=0.5)
    rc, p, err = plan(L, a)
    assert rc == 0 and p['refused'] == 0 and p['kernel'] == 0, err
    assert p['splits'] * p['ks_per_split'] >= 27                             # 9 taps x 3 granules of the concat


def test_ops_conv2d_refuses_what_stride_2_cannot_run():
    """raised by _conv2d_args before a pointer is taken: CPU tensors get this far (a good call then stops at 'must be a GPU tensor')"""
    from diffusion_tts_amd import ops
    x = torch.zeros(1, 8, 8, 64, dtype=torch.float16)
    w = torch.zeros(64, 3, 3, 64, dtype=torch.float16)
    xw = ops.X3Weight(torch.zeros(64, 3, 3, 128, dtype=torch.float16), 1.0, (64, 3, 3, 64))
    for kw, what in ((dict(up=True), 'up=True'), (dict(gn_coef=torch.zeros(1, 64, 2)), 'gn_coef'), (dict(skip=(None, None, False)), 'skip'),
                     (dict(out_split2=True), 'out_split2')):
        with pytest.raises(ValueError, match='stride=2 takes no ' + what):
            ops.conv2d(x, w, stride=2, **kw)
        with pytest.raises(ValueError, match='stride=2 takes no ' + what):
            ops.conv_plan(x, w, stride=2, **kw)
    with pytest.raises(ValueError, match='stride=2 takes no a split-precision weight'):
        ops.conv2d(x.float(), xw, stride=2)
    with pytest.raises(ValueError, match='stride=2 takes no float32 activations'):
        ops.conv2d(x.float(), w.float(), stride=2)
    with pytest.raises(ValueError, match='stride=2 takes no a 1x1 weight'):
        ops.conv2d(x, torch.zeros(64, 1, 1, 64, dtype=torch.float16), stride=2)
    for bad in (0, 3, -1, 4, 1.5, None):
        with pytest.raises(ValueError, match='stride'):
            ops.conv2d(x, w, stride=bad)
        with pytest.raises(ValueError, match='stride'):
            ops.conv_kernel(x, w, stride=bad)
    with pytest.raises(RuntimeError, match='GPU tensor'):                    # nothing else stands between a good call and the library
        ops.conv2d(x, w, stride=2)
    assert ops.conv_kernel(x, w, stride=2) == 0 and ops.conv_kernel(x, w) == 0
