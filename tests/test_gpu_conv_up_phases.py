"""The phase form of the nearest-up 3x3 convolution in split precision (dts_conv_args.up == 2: conv_igemm_kernel<.., PH = true>, four 2x2
convolutions over the low-resolution input with summed taps, ops.pack_conv_weight(.., up_phases=True)) against tests/conv_reference.py --
the float64 convolution of the ORIGINAL 3x3 weights over the upsampled input, which shares no code with the library.

EXACT LEG (test_exact).  conv_reference.exact_inputs: activations in {0, +-1, +-2}, weights in {0, +-1}, integer epilogue operands.  A
summed tap is then an integer of magnitude <= 4: exact in float32, and exact in the hi part of its split image (asserted on the CPU before
the launch: the lo plane of the packed phase tensor is zero and hi * phase_acc_scale equals the float64 tap sums).  Every product and
partial sum is an integer multiple of 2^-14 below 2^8 (assert_exact_conditions; sum |x||w'| <= sum |x||w|, the reference's S), so the
output must EQUAL the float64 reference, in a NaN-guarded buffer whose guard bands stay NaN; the per-image sums of the strip statistics
must equal the float64 moments (a phase launch files a wave's 64 low-resolution pixels under strip n * 4S + phase * S + s: only sums per
image are layout-free); ops.conv_plan must report phases == 1, kernel == 0, splits == 1 and the forced waves / ring depth / epilogue.
Every shape runs with 4 and 8 waves, ring depth 2 and 3 and conv_epi32 = 0 and 1.  The K split is pinned with conv_splits = 1 like every
case of tests/test_gpu_conv.py: left alone, the launcher's estimate wants a split for the 16-block grid of `ph_16x16_c192` (nk = 24), which
the phase form does not take -- ops.conv2d then keeps the nine-tap route for such a grid (asserted in test_routing).

ROUNDING LEG (test_rounding).  Gaussian inputs (conv_reference.gaussian_inputs) on the first and the fourth shape, per element against
conv_ref64 of the original 3x3 weights:

    |got - o| <= 1.001 * 2^-24 |o| + 2 (K + 8) 2^-24 S + 3 * 2^-22 prod + 2^-24 prod,        K = 4 * cin

Derivation (written before the first run).  The bound of tests/test_gpu_conv.py for f16x3 is 1.001 u |o| + c (K + 8) 2^-24 S + 3 * 2^-22
sum |x||w| |out_scale| with u = 2^-24, c = 2 and K the number of accumulated products; its derivation holds term by term for the phase form
with the summed weights w' in the place of w.  The phase form accumulates K = 4 * cin products x w', and sum |x||w'| <= sum |x||w| by the
triangle inequality (each w' is a sum of distinct original taps meeting the SAME input pixel), so the reference's S and prod, taken over
the nine original taps, bound the phase form's own.  One rounding is new: a summed tap is formed in float64 and rounded ONCE to float32
before it is split, |fl(w') - w'| <= 2^-24 |w'| <= 2^-24 sum |w_taps|, which moves the result by at most 2^-24 sum |x||w| |out_scale| =
2^-24 prod.
Record of a run on an MI355X (max err / bound; a record, NOT the source of the bound):
    ph_8x8_c64      waves 4: 0.003   waves 8: 0.003
    ph_16x16_c192   waves 4: 0.001   waves 8: 0.001
(network level, same run: max |err| against the float64 forward 1.43e-6 with the route off, 1.38e-6 with it on)

REFUSALS (test_refusals).  up = 2 with a 16-bit or f32 dtype, with x2, gn_coef, skip_*, out_split2 or a forced K split: dts_conv_plan
reports `refused` with a message and dts_conv2d returns an error before it looks at a pointer (nothing is launched).

NETWORK LEVEL (test_network_forward_on_and_off).  A reduced ADM denoiser (one up block, model_channels 64, 16x16, 2 rows) with
conv_up_phases on and off against a float64 evaluation of the oracle's U-Net on the same weights: the error of the `on` run must lie
within 1.5 x the error of the `off` run (both are f32-level reorderings of the same sum, so the `off` run is the yardstick).  Both runs pin
conv_splits = 1: the up block's grid at 2 rows is 4 blocks, which the launcher's estimate would split, i.e. leave to the nine-tap route."""
import ctypes as C
import functools
import itertools
import math
from unittest import mock

import pytest
import torch

import conv_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD = 4096
MODE = 'f16x3'


def _case(name, n, h, w, c1, cout, ep='b', scale=1.0, stats=False):
    return R.Case(name, 'igemm', (MODE,), n, h, w, c1, 0, cout, 3, True, ep, scale, stats, (), ('int',), False, None, False, 1, '')


SHAPES = {c.name: c for c in (
    _case('ph_8x8_c64', 2, 8, 8, 64, 192, stats=True),                # one K step per tap; a 128-pixel tile spanning two images; every border
    _case('ph_4x4_c128', 3, 4, 4, 128, 128),                          # ragged last tile (48 of 128 rows), 128-cout tile
    _case('ph_6x10_c64', 1, 6, 10, 64, 192),                          # non-power-of-two sizes: the division path
    _case('ph_16x16_c192', 1, 16, 16, 192, 384, stats=True),          # two cout tiles, two pixel tiles per image: strip indexing across tiles
    _case('ph_8x8_c64_epi', 2, 8, 8, 64, 192, ep='bnr', scale=0.5, stats=True),     # bias_nc, residual, out_scale != 1
)}
FORMS = list(itertools.product((4, 8), (2, 3), (0, 1)))              # (conv_waves, conv_stages, conv_epi32)


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


class _Knobs:
    """sets tuning knobs around a launch and puts back the values they had, whatever happens"""

    def __init__(self, **knobs):
        self.knobs, self.old = knobs, []

    def __enter__(self):
        from diffusion_tts_amd import _lib
        lib = _lib.load()
        try:
            for k, v in self.knobs.items():
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


@functools.lru_cache(maxsize=None)
def _exact(name):
    a = R.exact_inputs(SHAPES[name], MODE, 0, 'int')
    return a, R.reference(a)


@functools.lru_cache(maxsize=None)
def _gauss(name):
    a = R.gaussian_inputs(SHAPES[name], MODE)
    return a, R.reference(a)


def _device_args(ops, case, a):
    dev = lambda t: None if t is None else t.float().to(DEV).contiguous()
    x = dev(R.nhwc(a['x1']))
    wp = ops.pack_conv_weight(a['w'].float().to(DEV), ops.F16X3, up_phases=True)
    call = dict(bias_nc=dev(a['bias_nc']), residual=None if a['residual'] is None else dev(R.nhwc(a['residual'])), up=True,
                out_scale=a['out_scale'])
    return x, wp, dev(a['bias']), call


def _launch(ops, case, a, want_stats, waves, stages, epi):
    """ops.conv2d(.., up=True) with a phase-packed weight under the forced form: (out NCHW on the CPU, stats or None, guard buffer, plan)"""
    x, wp, bias, call = _device_args(ops, case, a)
    numel = case.n * 4 * case.h * case.w * case.cout
    buf = torch.full((numel + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + numel].view(case.n, 2 * case.h, 2 * case.w, case.cout)
    call.update(out=view, gn_stats=want_stats)
    with _Knobs(conv_splits=1, conv_waves=waves, conv_stages=stages, conv_epi32=epi):
        assert ops.conv_takes_phases(x, wp, bias, **call)
        assert ops.conv_kernel(x, wp, up=True, residual=call['residual'], gn_stats=want_stats) == 0
        plan = ops.conv_plan(x, wp, bias, **call)
        out = ops.conv2d(x, wp, bias, **call)
        torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr()
    st = out._gn_stats
    assert plan['stats_written'] == int(st is not None)
    return R.nchw(out.cpu()), (None if st is None else st.cpu()), buf.cpu(), plan


def _assert_plan(case, plan, waves, stages, epi):
    tile = 192 if case.cout % 192 == 0 else 128
    whole_strips = (case.h * case.w) % 64 == 0          # the row-layout epilogue works in strips of 64 low-resolution pixels
    assert (plan['refused'], plan['phases'], plan['kernel'], plan['splits']) == (0, 1, 0, 1), plan
    assert (plan['tile'], plan['waves'], plan['stages'], plan['pf']) == (tile, waves, stages, 1), plan
    assert plan['epi_rows'] == (epi if whole_strips else 0), plan
    n_pt = -(-(case.n * case.h * case.w) // 128)
    assert (plan['n_ct'], plan['n_pt'], plan['nblk']) == (case.cout // tile, n_pt, 4 * (case.cout // tile) * n_pt), plan
    assert plan['ks_per_split'] == 4 * (case.c1 // 32) and plan['threads'] == 64 * waves


@pytest.mark.parametrize('name', list(SHAPES))
def test_exact(ops, name):
    case = SHAPES[name]
    a, ref = _exact(name)
    want = ref.o.float()
    stats64 = R.image_stats64(want) if case.stats else None
    R.assert_exact_conditions(ref, torch.float32, stats64, a)
    # the summed taps: small integers, exact in float32 and in the hi part of their split image
    wcpu = ops.pack_conv_weight(a['w'].float(), ops.F16X3, up_phases=True)
    hi, lo = ops.split_planes(wcpu.phases, case.c1)
    sums = ops.up_phase_weights(a['w'])
    assert not bool(lo.any()) and torch.equal(hi.double() * wcpu.phase_acc_scale, sums)
    assert float(sums.abs().max()) <= 4.0 and torch.equal(sums, sums.round())
    for waves, stages, epi in FORMS:
        got, st, buf, plan = _launch(ops, case, a, case.stats, waves, stages, epi)
        what = f'{name}: waves {waves}, ring {stages}, conv_epi32 {epi} (epi_rows {plan["epi_rows"]})'
        print(what)
        _assert_plan(case, plan, waves, stages, epi)
        assert got.dtype == torch.float32
        assert not bool(torch.isnan(got).any()), f'{what}: an output element was never written'
        assert torch.equal(got, want), f'{what}: {int((got != want).sum())} of {want.numel()} elements differ'
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), f'{what}: a store outside the output'
        if not case.stats:
            assert st is None
        else:
            assert st is not None and tuple(st.shape) == (case.n * 4 * case.h * case.w // 64, case.cout, 2)
            assert not bool(torch.isnan(st).any())
            assert torch.equal(st.double().view(case.n, -1, case.cout, 2).sum(1), stats64), what


@pytest.mark.parametrize('name', ['ph_8x8_c64', 'ph_16x16_c192'])
def test_rounding(ops, name):
    case = SHAPES[name]
    a, ref = _gauss(name)
    K = 4 * case.c1
    bound = 1.001 * 2.0 ** -24 * ref.o.abs() + 2.0 * (K + 8) * 2.0 ** -24 * ref.S + 3.0 * 2.0 ** -22 * ref.prod + 2.0 ** -24 * ref.prod
    for waves in (4, 8):
        got, st, buf, plan = _launch(ops, case, a, False, waves, 2, 1)
        assert (plan['phases'], plan['kernel'], plan['splits']) == (1, 0, 1)
        err = (got.double() - ref.o).abs()
        ratio = float((err / bound).max())
        print(f'rounding {name}: waves {waves}, max err/bound = {ratio:.3f}')
        assert bool((err <= bound).all()), ratio
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def test_routing(ops):
    """what ops.conv2d does by itself: the phase form where dts_conv_takes_phases says yes, the nine-tap gather (bit-exact too) where the
    grid wants a K split, where the knob is off, and for a weight packed without up_phases"""
    for name in ('ph_8x8_c64', 'ph_16x16_c192'):
        case = SHAPES[name]
        a, ref = _exact(name)
        x, wp, bias, call = _device_args(ops, case, a)
        plain = ops.pack_conv_weight(a['w'].float().to(DEV), ops.F16X3)
        auto = ops.conv_plan(x, wp, bias, gn_stats=True, **call)
        assert auto['refused'] == 0 and ops.conv_takes_phases(x, wp, bias, gn_stats=True, **call) == bool(auto['phases'])
        if name == 'ph_8x8_c64':
            assert auto['phases'] == 1 and auto['splits'] == 1           # nk = 8: no split considered
        else:
            assert auto['phases'] == 0 and auto['splits'] > 1            # 16 blocks, nk = 24: the estimate splits K, the old route's
        with _Knobs(conv_up_phases=0):
            assert not ops.conv_takes_phases(x, wp, bias, **call)
            off = ops.conv_plan(x, wp, bias, **call)
            assert off['phases'] == 0 and off['refused'] == 0
            got_off = ops.conv2d(x, wp, bias, **call)
        assert ops.conv_plan(x, plain, bias, **call)['phases'] == 0 and not ops.conv_takes_phases(x, plain, bias, **call)
        assert ops.conv_plan(x, wp, bias, phases=False, **call)['phases'] == 0
        got_auto = ops.conv2d(x, wp, bias, gn_stats=True, **call)
        torch.cuda.synchronize()
        for got in (got_off, got_auto):
            assert torch.equal(R.nchw(got.cpu()), ref.o.float())


def _plan_args(L, **over):
    a = L.ConvArgs()
    a.n, a.hin, a.win, a.c1, a.c2, a.cout, a.ksize, a.up, a.dtype = 2, 8, 8, 128, 0, 192, 3, 2, L.DTS_F16X3
    a.out_scale, a.workspace, a.workspace_bytes = 1.0, 16, 96 << 20        # (the plan never dereferences a pointer: presence is all it reads)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_refusals():
    from diffusion_tts_amd import _lib as L
    lib = L.load()

    def plan(a):
        info = L.ConvPlanInfo()
        rc = lib.dts_conv_plan(C.byref(a), C.byref(info))
        return rc, info, lib.dts_last_error().decode()

    rc, info, _ = plan(_plan_args(L))
    assert rc == 0 and (info.refused, info.phases, info.kernel, info.splits) == (0, 1, 0, 1)
    assert lib.dts_conv_takes_phases(C.byref(_plan_args(L))) == 1
    assert lib.dts_conv_takes_phases(C.byref(_plan_args(L, up=1))) == 0 and lib.dts_conv_takes_phases(None) == 0
    cases = {
        'bf16': dict(dtype=L.DTS_BF16), 'f16': dict(dtype=L.DTS_F16), 'f32': dict(dtype=L.DTS_F32),
        'x2': dict(c2=64, x2=16), 'gn_coef': dict(gn_coef=16), 'skip': dict(skip_c=128, skip_x=16, skip_w=16),
        'out_split2': dict(out_split2=1), 'cout 64': dict(cout=64), 'ksize 1': dict(ksize=1),
        'statistics over partial strips': dict(hin=4, win=4, stats_out=16),
    }
    for what, over in cases.items():
        a = _plan_args(L, **over)
        rc, info, msg = plan(a)
        assert rc == 0 and info.refused == 1 and info.phases == 0 and msg, (what, msg)
        assert lib.dts_conv_takes_phases(C.byref(a)) == 0, what
        assert lib.dts_conv2d(C.byref(a), None) != 0, what           # refused before any pointer is looked at: nothing is launched
        print(f'{what}: {msg}')
    for knob, value in (('conv_splits', 2), ('conv_up_phases', 0)):
        with _Knobs(**{knob: value}):
            a = _plan_args(L)
            rc, info, msg = plan(a)
            assert rc == 0 and info.refused == 1 and info.phases == 0 and msg, (knob, msg)
            assert lib.dts_conv_takes_phases(C.byref(a)) == 0 and lib.dts_conv2d(C.byref(a), None) != 0
            print(f'{knob}={value}: {msg}')
    # a residual is supported (both f32 epilogues address it through the tile map)
    rc, info, _ = plan(_plan_args(L, residual=16))
    assert rc == 0 and (info.refused, info.phases) == (0, 1)


def _oracle64(cfg, sd, x, sigma, labels):
    """the oracle's EDMPrecond arithmetic (oracle/edm_nets.py EDMPrecondOracle.__call__) evaluated in float64 on the same weights"""
    from oracle import edm_nets as E
    ncfg = E.NetCfg(arch=cfg.arch, img_resolution=cfg.img_resolution, img_channels=cfg.img_channels, label_dim=cfg.label_dim,
                    model_channels=cfg.model_channels, channel_mult=list(cfg.channel_mult), channel_mult_emb=cfg.channel_mult_emb,
                    num_blocks=cfg.num_blocks, attn_resolutions=list(cfg.attn_resolutions), augment_dim=cfg.augment_dim)
    sd64 = {k[len('model.'):]: v.detach().double() for k, v in sd.items() if k.startswith('model.')}
    x, sigma = x.double(), sigma.double().reshape(-1, 1, 1, 1)
    sd2 = ncfg.sigma_data ** 2
    c_skip, c_out, c_in = sd2 / (sigma ** 2 + sd2), sigma * ncfg.sigma_data / (sigma ** 2 + sd2).sqrt(), 1 / (sd2 + sigma ** 2).sqrt()
    # (the oracle's attention weights are float32 like the reference's AttentionOp: the same formula without the casts, for this call)
    att64 = lambda q, k: torch.einsum('ncq,nck->nqk', q, k / math.sqrt(k.shape[1])).softmax(dim=2)
    with torch.no_grad(), mock.patch.object(E, 'attention_weights', att64):
        F_x = E.dhariwal_unet(sd64, ncfg, c_in * x, (sigma.log() / 4).flatten(), labels.double())
    assert F_x.dtype == torch.float64
    return c_skip * x + c_out * F_x


def test_network_forward_on_and_off():
    from diffusion_tts_amd import init as dinit, ops
    from diffusion_tts_amd.config import EDMConfig
    from diffusion_tts_amd.networks import EDMPrecond
    cfg = EDMConfig('adm', 16, 3, 10, 64, [1, 2], 4, 1, [8], 0)      # 16x16 image, model_channels 64, two levels: one up block (8x8 -> 16x16)
    sd, _ = dinit.refill_degenerate(dinit.edm_state_dict(cfg, 0), 0)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 16, 16, generator=g, dtype=torch.float64)
    sigma = torch.tensor([1.5], dtype=torch.float64)
    lab = torch.eye(10, dtype=torch.float64)[torch.tensor([3, 7])]
    want = _oracle64(cfg, sd, x, sigma, lab)
    errs, routed = {}, {}
    for tag, knob in (('off', 0), ('on', 1)):
        with _Knobs(conv_up_phases=knob, conv_splits=1):
            net = EDMPrecond(cfg, sd, device=DEV)                    # (its own forward cache: nothing is replayed from the other setting)
            ups = [(b, net.blocks[b.name].w0) for b in net.dec if b.up]
            assert len(ups) == 1 and ups[0][1].phases is not None
            b, w0 = ups[0]
            probe = torch.zeros(2, 8, 8, b.cin, device=DEV)
            routed[tag] = ops.conv_takes_phases(probe, w0, gn_stats=True)
            got = net(x, sigma, lab).cpu().double()
            torch.cuda.synchronize()
        errs[tag] = float((got - want).abs().max())
    print(f'network forward vs float64 oracle: max |err| phases off {errs["off"]:.3e}, on {errs["on"]:.3e}; phase route taken: {routed}')
    assert routed == {'off': False, 'on': True}
    assert errs['on'] <= 1.5 * errs['off'], errs
