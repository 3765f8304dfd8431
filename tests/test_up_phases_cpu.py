"""CPU: the algebra of the phase form of a nearest-up 3x3 convolution, alone.

In the nearest-2x upsampled image every 2x2 cell repeats one input pixel, so an output pixel of phase (py, px) = (y & 1, x & 1) sees a 2x2
neighbourhood of the LOW-resolution input and the nine taps collapse to four whose weights are sums of the original ones
(rows, py = 0: {w0, w1 + w2} at dy in {-1, 0}; py = 1: {w0 + w1, w2} at dy in {0, +1}; columns alike).  The zero padding after the upsample
is the low-resolution out-of-range row / column.  Checked in float64 torch against conv2d(interpolate(x, 2, 'nearest'), w, padding=1) at
1e-12 relative, first with ops.up_phase_weights, then with the tensors ops.pack_conv_weight(.., up_phases=True) packs (on the CPU: hi + lo
of the split image, unscaled), which pins the phase index 2*py + px, the tap order (ty, tx) row-major and the offsets
dy = ty - 1 + py, dx = tx - 1 + px of include/dts.h."""
import torch
import torch.nn.functional as F

N, H, W, CIN, COUT = 2, 4, 6, 3, 5


def _inputs(cin=CIN, cout=COUT, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, cin, H, W, generator=g, dtype=torch.float64), torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)


def _reference(x, w):
    return F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, padding=1)


def _phase_convs(x, ph):
    """out[n, o, 2y + py, 2x + px] = sum over (ty, tx, i) of ph[2*py + px][o][ty][tx][i] * x[n, i, y + ty - 1 + py, x + tx - 1 + px] (zero outside)"""
    n, cin, h, w = x.shape
    cout = ph.shape[1]
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(n, cout, 2 * h, 2 * w, dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            acc = torch.zeros(n, cout, h, w, dtype=torch.float64)
            for ty in range(2):
                for tx in range(2):
                    dy, dx = ty - 1 + py, tx - 1 + px
                    xs = xp[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                    acc += torch.einsum('oi,nihw->nohw', ph[2 * py + px, :, ty, tx, :], xs)
            out[:, :, py::2, px::2] = acc
    return out


def _assert_close(got, want, rel):
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    assert err <= rel * float(want.abs().max()), (err, float(want.abs().max()))


def test_four_phase_convolutions_equal_the_upsampled_3x3():
    from diffusion_tts_amd import ops
    x, w = _inputs()
    ph = ops.up_phase_weights(w)
    assert tuple(ph.shape) == (4, COUT, 2, 2, CIN) and ph.dtype == torch.float64
    _assert_close(_phase_convs(x, ph), _reference(x, w), 1e-12)
    # the rule itself, written out: rows of phase py = 0 are {w0, w1 + w2}, of py = 1 {w0 + w1, w2}; columns alike
    rows = {0: [w[:, :, 0], w[:, :, 1] + w[:, :, 2]], 1: [w[:, :, 0] + w[:, :, 1], w[:, :, 2]]}
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                r = rows[py][ty]                                     # [O][I][kw]
                cols = [r[:, :, 0], r[:, :, 1] + r[:, :, 2]] if px == 0 else [r[:, :, 0] + r[:, :, 1], r[:, :, 2]]
                for tx in range(2):
                    assert torch.allclose(ph[2 * py + px, :, ty, tx, :], cols[tx], rtol=1e-14, atol=0)


def test_packed_phase_tensor_follows_the_same_conventions():
    """pack_conv_weight(F16X3, up_phases=True) on the CPU: `phases` [4][O][2][2][2*I] float16, per 32 input channels hi(32) | lo(32) of the
    summed weights * 2^k.  Weights that are small integers make hi exact and lo zero, so (hi + lo) * phase_acc_scale must reproduce the
    float64 tap sums -- and with them the reference -- exactly; `packed`, `acc_scale` and `shape` are what they are without up_phases."""
    from diffusion_tts_amd import ops
    cin = 32                                                       # one K step of the split image
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randint(-3, 4, (COUT, cin, 3, 3), generator=g).double()
    xw = ops.pack_conv_weight(w.float(), ops.F16X3, up_phases=True)
    plain = ops.pack_conv_weight(w.float(), ops.F16X3)
    assert plain.phases is None
    assert torch.equal(xw.packed, plain.packed) and xw.acc_scale == plain.acc_scale and xw.shape == plain.shape == (COUT, 3, 3, cin)
    assert tuple(xw.phases.shape) == (4, COUT, 2, 2, 2 * cin) and xw.phases.dtype == torch.float16
    hi, lo = ops.split_planes(xw.phases, cin)
    assert not bool(lo.any())
    ph = (hi.double() + lo.double()) * xw.phase_acc_scale
    assert torch.equal(ph, ops.up_phase_weights(w))
    amax = float(ops.up_phase_weights(w).abs().max())
    assert 2.0 ** 13 < amax / xw.phase_acc_scale <= 2.0 ** 14         # the power of two comes from max |w'| of the SUMMED tensor
    _assert_close(_phase_convs(x, ph), _reference(x, w), 1e-12)
    # a general float32 weight: hi + lo carries the summed weight to 2^-22 relative of the tensor's scale
    wf = torch.randn(COUT, cin, 3, 3, generator=g)
    xf = ops.pack_conv_weight(wf, ops.F16X3, up_phases=True)
    hi, lo = ops.split_planes(xf.phases, cin)
    want = ops.up_phase_weights(wf.double())
    got = (hi.double() + lo.double()) * xf.phase_acc_scale
    assert float((got - want).abs().max()) <= 2.0 ** -21 * float(want.abs().max())
