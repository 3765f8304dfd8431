"""GPU: the NCSN++ denoisers (Fourier embedding, residual encoder, [1,3,3,1] resampling) -- the new kernels against float64 references, the
one-launch `aux_residual` convolution against the unfused formula, and the full-size networks and searches against the reference's own outputs
(tests/golden/make_golden_ncsnpp.py)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import ncsnpp_helpers as nh                                            # noqa: E402
from helpers import check_decisions                                    # noqa: E402
from diffusion_tts_amd import init as dinit                            # noqa: E402

DEV = 'cuda'
X3 = 'f16x3'
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TOL = {torch.float32: 2e-5, torch.bfloat16: 2.5e-2, torch.float16: 4e-3}       # tests/test_gpu_ops.py: resample2x / conv2d(+residual) per storage type
TOL_X3 = 3e-6                                                                   # tests/test_gpu_ops.py::test_conv2d_split_precision
torch.set_num_threads(8)


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / max(1e-6, float(ref.double().abs().max())))


def to_nhwc(ops, x, dtype):
    return ops.nchw_to_nhwc(x.to(DEV, torch.float32).contiguous(), dtype)


def from_nhwc(ops, x):
    return ops.nhwc_to_nchw(x).cpu()


def fir_ref(x64, up):
    c = x64.shape[1]
    f2 = dinit.resample_filter_2d([1, 3, 3, 1]).double().tile([c, 1, 1, 1])
    if up:
        return F.conv_transpose2d(x64, f2 * 4, stride=2, padding=1, groups=c)
    return F.conv2d(x64, f2, stride=2, padding=1, groups=c)


def unsplit(ops, act):
    """a SplitAct back to float64 NCHW: hi + lo * 2^-11"""
    hi, lo = act.planes()
    return (hi.double() + lo.double() / 2048.0).permute(0, 3, 1, 2).cpu()


# channel counts: one 16-byte vector, an odd number of vectors (the grid's tail), and the networks' widths
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('res', [8, 16, 32, 64])
@pytest.mark.parametrize('up', [False, True])
def test_resample_fir_matches_float64(ops, dtype, res, up):
    for c in (8, 24, 40, 128 if res >= 32 else 256):
        n = 3 if c < 128 else 2
        x = torch.randn(n, c, res, res, generator=torch.Generator().manual_seed(res + c)).to(dtype).float()
        got = from_nhwc(ops, ops.resample_fir(to_nhwc(ops, x, dtype), up))
        want = fir_ref(x.double(), up)
        assert got.shape == want.shape
        e = rel_err(got, want)
        print(f'resample_fir {"up" if up else "down"} {dtype} {res}x{res} c={c}: rel err {e:.2e}')
        assert e < TOL[dtype], (c, e)


@pytest.mark.parametrize('res', [8, 16, 32, 64])
@pytest.mark.parametrize('up', [False, True])
def test_resample_fir_split_image(ops, res, up):
    """f32 in, split-precision operand image out: the float64 result to the f32 bound, and bit for bit dts_split3_f16 of the f32 pass"""
    for c in (32, 96, 128 if res >= 32 else 256):
        x = torch.randn(2, c, res, res, generator=torch.Generator().manual_seed(7 * res + c)) * (2.0 ** (c % 5 - 2))
        xd = to_nhwc(ops, x, torch.float32)
        sp = ops.resample_fir(xd, up, split_out=True)
        assert sp.data.dtype == torch.float16 and sp.shape[-1] == c and sp.data.shape[-1] == 2 * c
        e = rel_err(unsplit(ops, sp), fir_ref(x.double(), up))
        print(f'resample_fir split {"up" if up else "down"} {res}x{res} c={c}: rel err {e:.2e}')
        assert e < TOL[torch.float32], (c, e)
        assert torch.equal(sp.data, ops.split3_f16(ops.resample_fir(xd, up)))


@pytest.mark.parametrize('dtype', DTYPES + [X3])
def test_space_to_depth2(ops, dtype):
    """exact rearrangement, zero padding, from the f32 NCHW image and from NHWC activations (vector path and the odd-channel path)"""
    adt = ops.act_dtype(dtype)
    for c, nchw in ((3, True), (5, True), (3, False), (8, False), (40, False), (128, False)):
        if not nchw and dtype != X3 and c % (4 if adt == torch.float32 else 8):
            continue                                  # NHWC activations of that type cannot have this channel count at all
        if not nchw and dtype == X3 and c % 4:
            continue
        x = torch.randn(2, c, 12, 8, generator=torch.Generator().manual_seed(c)).to(adt).float()
        src = x.to(DEV).contiguous() if nchw else to_nhwc(ops, x, adt)
        out = ops.space_to_depth2(src, dtype, nchw=nchw)
        g = ops.conv_cin_granule(dtype)
        cpad = -(-4 * c // g) * g
        want = torch.zeros(2, cpad, 6, 4)
        want[:, :4 * c] = x.view(2, c, 6, 2, 4, 2).permute(0, 3, 5, 1, 2, 4).reshape(2, 4 * c, 6, 4)
        if dtype == X3:
            assert out.shape[-1] == cpad
            assert torch.equal(out.data, ops.split3_f16(to_nhwc(ops, want, torch.float32)))
        else:
            assert torch.equal(from_nhwc(ops, out), want), (c, nchw)


# (caux, cout, input resolution): ncsnpp_cifar10 = 3->256 at 32, 256->256 at 16; ncsnpp_ffhq64 = 3->128 at 64, 128->256 at 32, 256->256 at 16
@pytest.mark.parametrize('dtype', DTYPES + [X3])
@pytest.mark.parametrize('caux,cout,res', [(3, 256, 32), (256, 256, 16), (3, 128, 64), (128, 256, 32)])
def test_aux_residual_launch_matches_the_unfused_formula(ops, dtype, caux, cout, res):
    """x = (x + aux_residual(aux)) / sqrt(2) as space-to-depth + ONE conv launch (composed weight, residual, scale, strip statistics) against
    conv2d(aux, w, padding 2) -> [1,3,3,1] filter at stride 2 -> + bias, in float64"""
    adt = ops.act_dtype(dtype)
    g = torch.Generator().manual_seed(caux + cout + res)
    n = 2
    aux = torch.randn(n, caux, res, res, generator=g)
    aux = aux if caux == 3 else aux.to(adt).float()
    w = (torch.rand(cout, caux, 3, 3, generator=g) * 2 - 1) * math.sqrt(6 / (9 * (caux + cout)))        # the constructor's xavier_uniform
    b = (torch.rand(cout, generator=g) * 2 - 1) * 0.1
    xres = torch.randn(n, cout, res // 2, res // 2, generator=g).to(adt).float()
    f2 = dinit.resample_filter_2d([1, 3, 3, 1]).double().tile([cout, 1, 1, 1])
    y = F.conv2d(F.conv2d(aux.double(), w.double(), padding=2), f2, stride=2, groups=cout) + b.double()[None, :, None, None]
    want = (xres.double() + y) / math.sqrt(2)
    src = aux.to(DEV).contiguous() if caux == 3 else to_nhwc(ops, aux, adt)
    s2d = ops.space_to_depth2(src, dtype, nchw=caux == 3)
    wp = ops.pack_conv_weight(ops.fused_down_weight(w.to(DEV), cpad=s2d.shape[-1]), dtype)
    out = ops.conv2d(s2d, wp, b.to(DEV), residual=to_nhwc(ops, xres, adt), out_scale=math.sqrt(0.5), gn_stats=True)
    got = from_nhwc(ops, out)
    e = rel_err(got, want)
    print(f'aux_residual {caux}->{cout} at {res}x{res}, {dtype}: rel err {e:.2e}')
    assert e < (TOL_X3 if dtype == X3 else TOL[dtype]), e
    st = out._gn_stats
    assert st is not None, 'the launch did not emit the strip statistics of the next norm0'
    per = st.view(n, -1, cout, 2).sum(1).cpu().double()
    g64 = got.double()
    ref = torch.stack([g64.sum((2, 3)), (g64 * g64).sum((2, 3))], -1)
    scale = float(g64.abs().max())
    assert torch.allclose(per, ref, rtol=1e-4 if adt == torch.float32 else 2e-2, atol=(1e-3 if adt == torch.float32 else 1.0) * max(1.0, scale) ** 2)


def test_fourier_embedding_matches_float64(ops):
    """cos / sin of c_noise * (2 pi freqs) for c_noise = ln(sigma) / 4 over the sampler's sigma range, with the golden network's frequencies
    (|argument| up to a few hundred radians).  Bound, from the number formats alone: the factor 2*pi*f is formed in f32 (the reference's own
    expression: one rounding, 2^-24, on top of f32(2 pi), 2.8e-8 relative) and multiplied by c_noise in f32 (another 2^-24), so the ARGUMENT is
    off by at most |a| * (2 * 2^-24 + 2.8e-8); cosf / sinf themselves add a few ulp of 1."""
    fr = torch.from_numpy(nh.golden()['ncsnpp_cifar10_freqs'])
    sig = torch.logspace(math.log10(0.002), math.log10(80.0), 257, dtype=torch.float64)
    c = (sig.log() / 4).float()
    want_arg = c.double()[:, None] * (2 * math.pi * fr.double())[None, :]
    f32 = (2 * np.pi * fr).to(DEV)
    got = ops.pos_embedding(c.to(DEV), f32, swap=True).cpu().double()
    want = torch.cat([want_arg.sin(), want_arg.cos()], 1)
    amax = float(want_arg.abs().max())
    tol = amax * (2 * 2.0 ** -24 + 2.8e-8) + 4 * 2.0 ** -24
    err = float((got - want).abs().max())
    print(f'Fourier embedding: max |arg| {amax:.1f} rad, max err {err:.3e} (bound {tol:.3e})')
    assert fr.numel() == 128 and amax > 100 and err <= tol


_NETS = {}


def _net(man, name, dtype):
    from diffusion_tts_amd.networks import EDMPrecond
    if (name, dtype) not in _NETS:
        cfg, sd = nh.preset_weights(man, name)
        _NETS[(name, dtype)] = EDMPrecond(cfg, sd, device=DEV, dtype=dtype)
    return _NETS[(name, dtype)]


def _fwd_inputs(g, man, name):
    x, sigma, D = (torch.from_numpy(g[f'{name}_{k}']) for k in ('x', 'sigma', 'D'))
    idx = g[f'{name}_label_idx']
    lab = torch.eye(man[name]['cfg']['label_dim'])[torch.from_numpy(idx)] if idx.size else None
    return x, sigma, lab, D


@pytest.mark.parametrize('dtype', [torch.float32, X3])
@pytest.mark.parametrize('name', ['ncsnpp_cifar10', 'ncsnpp_ffhq64'])
def test_fullsize_forward_matches_the_reference(name, dtype):
    """the reference EDMPrecond's D on 2 rows with per-row sigma.  Bound: max(3e-6 -- the ADM / DDPM++ forwards' -- , 4 x the reference's own
    fp32-vs-float64 distance on this architecture, from the manifest).  Eager launches and HIP-graph replay alike."""
    g, man = nh.golden(), nh.manifest()
    x, sigma, lab, D = _fwd_inputs(g, man, name)
    net = _net(man, name, dtype)
    bound = max(3e-6, 4 * man[name]['ref_f32_vs_f64'])
    scale = max(1.0, float(D.abs().max()))
    for call in range(4):                               # graphs.SIGHTINGS: the third call of a shape is captured, the fourth replayed
        got = net(x, sigma, lab).cpu()
        assert got.dtype == torch.float32 and got.shape == D.shape
        err = float((got - D).abs().max()) / scale
        e64 = float((got.double() - torch.from_numpy(g[f'{name}_D64'])).abs().max()) / scale
        print(f'{name} forward vs the reference, {dtype}, call {call}: err {err:.3e} (bound {bound:.3e}; vs float64 {e64:.3e}; reference vs float64 {man[name]["ref_f32_vs_f64"]:.3e})')
        assert err <= bound, (call, err, bound)
    assert net._graphs.replays >= 1


@pytest.mark.parametrize('dtype,tol', [(torch.float16, 1e-2), (torch.bfloat16, 6e-2)])
def test_throughput_modes_smoke(dtype, tol):
    """bf16 / f16: finite, and within the bound the tiny DDPM++ forward is held to in these modes (tests/test_gpu_search.py)"""
    g, man = nh.golden(), nh.manifest()
    x, sigma, lab, D = _fwd_inputs(g, man, 'ncsnpp_cifar10')
    got = _net(man, 'ncsnpp_cifar10', dtype)(x, sigma, lab).cpu()
    err = float((got - D).abs().max())
    print(f'ncsnpp_cifar10 forward, {dtype}: max err {err:.3e}')
    assert bool(torch.isfinite(got).all()) and err < tol * max(1.0, float(D.abs().max()))


@pytest.mark.parametrize('dtype', [X3, torch.float32])
def test_searches_against_the_reference_runs(dtype):
    """NAIVE (35 rows) and REJECTION N = 16 with the brightness scorer (560 rows) on the full-size NCSN++ CIFAR network against the reference's
    generate_image_grid runs: the criteria of test_baseline_configs_1_and_2_against_the_reference_runs -- row counts, final state within 1e-3,
    uint8 image within 1 LSB, the 16 rewards, and the kept trajectory where the top-2 margin decides it (helpers.check_decisions)."""
    from diffusion_tts_amd import sampler as sm, scorers as S
    from diffusion_tts_amd.hashing import seed0_scale
    g, m = nh.golden(), nh.manifest()
    net = _net(m, 'ncsnpp_cifar10', dtype)
    kw = dict(seed=m['seed'], num_steps=m['num_steps'], gridw=1, gridh=1, device=torch.device(DEV), scale_fn=seed0_scale, compute_dtype=dtype,
              verbose=False, **m['S'])

    def image_ok(h, ref):
        diff = np.abs(h['image'][0].permute(1, 2, 0).numpy().astype(np.int32) - ref.astype(np.int32))
        return diff.max() <= 1 and (diff > 0).mean() < 0.005
    lat = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(m['naive']['latent_seed']))
    assert np.array_equal(lat.numpy(), g['naive_latents'])
    h = sm.generate_image_grid(net, None, lat, torch.eye(10)[torch.tensor([m['naive']['label']])], sampling_method=sm.SamplingMethod.NAIVE,
                               sampling_params=dict(scorer=S.BrightnessScorer()), **kw)
    e0 = float((h['x'].cpu() - torch.from_numpy(g['naive_x_final'])).abs().max())
    print(f'NCSN++ naive vs the reference run, {dtype}: max |x - x_ref| {e0:.2e}')
    assert h['net_rows'] == m['naive']['net_rows'] == 35 and e0 < 1e-3 and image_ok(h, g['naive_image'])
    assert abs(float(h['final_scores'][0]) - float(g['naive_final_score'][0])) < 5e-5
    lat = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(m['rejection']['latent_seed']))
    assert np.array_equal(lat.numpy(), g['rej_latents'])
    h = sm.generate_image_grid(net, None, lat, torch.eye(10)[torch.tensor([m['rejection']['label']])],
                               sampling_method=sm.SamplingMethod.REJECTION_SAMPLING,
                               sampling_params=dict(scorer=S.BrightnessScorer(), **m['rejection']['params']), **kw)
    rew = h['rewards'][0].reshape(-1).numpy()
    e_r = float(np.abs(rew - g['rej_rewards']).max())
    e1 = float((h['x'].cpu() - torch.from_numpy(g['rej_x_final'])).abs().max())
    print(f'NCSN++ rejection vs the reference run, {dtype}: reward err {e_r:.2e} (top-2 gap {m["rejection"]["top2_gap"]:.1e}), '
          f'kept {int(h["selected"][0][0])} (reference {m["rejection"]["kept"]}), max |x - x_ref| {e1:.2e}')
    assert h['net_rows'] == m['rejection']['net_rows'] == 560 and e_r < 5e-5
    same, _ = check_decisions([torch.from_numpy(g['rej_rewards']).reshape(-1, 1)], [torch.from_numpy(g['rej_kept'])], [h['selected'][0].reshape(-1)],
                              f'NCSN++ rejection ({dtype})')
    assert same and int(h['selected'][0][0]) == m['rejection']['kept'] == int(g['rej_kept'][0])
    assert e1 < 1e-3 and image_ok(h, g['rej_image'])
