"""GPU: the kernels of the CLIP vision tower's split-precision mode -- dts_layer_norm_x3, dts_gelu_x3, dts_patchify_x3, dts_vit_tokens_f32,
dts_vit_head_f32 -- and the split-precision 1x1 dts_conv2d at the tower's ragged token counts.

Every operand image is compared BIT FOR BIT with ops.split3_f16 of the float32 values it stands for; the float32 values themselves are
compared with float64:
  * LayerNorm (and the head): the yardstick is torch's own float32 F.layer_norm on the same GPU input, measured against the same float64
    reference; the kernel may err at most 2x as much (both are valid float32 evaluation orders);
  * GELU: the float32 formula's own arithmetic (tests/test_gpu_clip_vision_ops.py derives it): quick-GELU (2^-20 + 2 e32 sens) |out|,
    sens = |z| sigmoid(-z), z = 1.702 x; erf GELU (2^-19 + 1.5 e32 sens) |out|, sens = |x| phi(x) / Phi(x); plus what the image keeps of a
    float32 value v = hi + lo: the lo half is an f16 number, 2^-11 relative of |lo| <= 2^-11 |v|, i.e. 2^-22 |v|, and a value below 2^-14
    lives in the lo half alone (the matrix cores flush subnormal hi halves): 2^-11 relative of less than 2^-14, i.e. 2^-25 absolute;
  * tokens: one float32 add: the correctly rounded sum, half an ulp from float64 (asserted at one ulp and bit for bit against torch's add);
  * the convolution: TOL_X3 = 3e-6 relative to max|out|, the bound of tests/test_gpu_ops.py::test_conv2d_split_precision.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
E32 = 2.0 ** -24
TOL_X3 = 3e-6


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


def g(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    return t.contiguous().view(torch.int16)


def image_value(ops, data, c):
    """the float64 value an operand image stands for: hi + lo * 2^11 / 2^11"""
    hi, lo = ops.split_planes(data, c)
    return hi.double() + lo.double() / 2048.0


# ---- LayerNorm -------------------------------------------------------------------------------------
def ln_case(c, rows, kind):
    gen = g(1000 * c + rows)
    x = torch.randn(rows, c, generator=gen)
    if kind == 'mean100':
        x = x + 100.0
    gamma, beta = 1.0 + 0.3 * torch.randn(c, generator=gen), 0.5 * torch.randn(c, generator=gen)
    return x.to(DEV).view(1, rows, c), gamma.to(DEV), beta.to(DEV)


@pytest.mark.parametrize('kind', ['unit', 'mean100'])
@pytest.mark.parametrize('rows', [1, 51, 771])
@pytest.mark.parametrize('c', [64, 320, 1024, 2048])
def test_layer_norm_x3(ops, c, rows, kind):
    x, gamma, beta = ln_case(c, rows, kind)
    eps = 1e-5
    ref = F.layer_norm(x.double(), (c,), gamma.double(), beta.double(), eps)
    t32 = F.layer_norm(x, (c,), gamma, beta, eps)
    out, img = ops.layer_norm_x3(x, gamma, beta, eps, want_f32=True)
    assert out.dtype == torch.float32 and out.shape == x.shape and tuple(img.data.shape) == (1, rows, 1, 2 * c) and img.shape == (1, rows, 1, c)
    err_k, err_t = float((out.double() - ref).abs().max()), float((t32.double() - ref).abs().max())
    print(f'layer_norm_x3 c={c} rows={rows} {kind}: max|kernel - f64| {err_k:.3e}, max|torch f32 - f64| {err_t:.3e}, ratio {err_k / err_t:.3f}')
    assert bool(torch.isfinite(out).all()) and err_t > 0
    assert err_k <= 2 * err_t
    # the image is the split of the float32 rows, and does not depend on whether those are written
    assert torch.equal(bits(img.data), bits(ops.split3_f16(out.view(1, rows, 1, c))))
    only = ops.layer_norm_x3(x, gamma, beta, eps)
    assert torch.equal(bits(only.data), bits(img.data))
    assert torch.equal(ops.layer_norm_x3(x, gamma, beta, eps, want_f32=True, want_split=False), out)
    # a 4-D input [n, t, 1, c] is the same rows
    assert torch.equal(bits(ops.layer_norm_x3(x.view(1, rows, 1, c), gamma, beta, eps).data), bits(img.data))


def test_layer_norm_x3_refusals(ops):
    x = torch.zeros(1, 4, 64, device=DEV)
    one = torch.ones(64, device=DEV)
    with pytest.raises(ValueError, match='layer_norm_x3: x must be a float32'):
        ops.layer_norm_x3(x.half(), one, one)
    with pytest.raises(ValueError, match='layer_norm_x3: 48 channels'):
        ops.layer_norm_x3(torch.zeros(1, 4, 48, device=DEV), one[:48], one[:48])
    with pytest.raises(ValueError, match='layer_norm_x3: 4096 channels'):
        ops.layer_norm_x3(torch.zeros(1, 4, 4096, device=DEV), torch.ones(4096, device=DEV), torch.ones(4096, device=DEV))
    with pytest.raises(ValueError, match='layer_norm_x3: gamma'):
        ops.layer_norm_x3(x, one[:32], one)
    with pytest.raises(ValueError, match='neither'):
        ops.layer_norm_x3(x, one, one, want_f32=False, want_split=False)
    with pytest.raises(ValueError, match=r'not \[n, t, c\]'):
        ops.layer_norm_x3(x.view(4, 64), one, one)


# ---- GELU ------------------------------------------------------------------------------------------
def gelu_inputs():
    """2046 grid points over [-12, 12], +-65504, 2048 tiny values: 4096 = [1, 64, 1, 64]"""
    x = torch.cat([torch.linspace(-12, 12, 2046, dtype=torch.float64).float(), torch.tensor([65504.0, -65504.0]),
                   2e-3 * torch.randn(2048, generator=g(3))])
    return x.view(1, 64, 1, 64).to(DEV)


@pytest.mark.parametrize('kind', ['quick_gelu', 'gelu'])
def test_gelu_x3(ops, kind):
    x = gelu_inputs()
    x64 = x.double()
    if kind == 'quick_gelu':
        z = 1.702 * x64
        ref = x64 * torch.sigmoid(z)
        sens = z.abs() * torch.sigmoid(-z)
        rel = 2.0 ** -20 + 2 * E32 * sens
        whole = z < -87
        f32 = x / (1.0 + torch.exp(-1.702 * x))                      # the kernel's formula, op by op in float32
    else:
        Phi = 0.5 * torch.erfc(-x64 / math.sqrt(2.0))
        ref = x64 * Phi
        phi = torch.exp(-0.5 * x64 * x64) / math.sqrt(2 * math.pi)
        sens = x64.abs() * phi / Phi.clamp_min(1e-300)
        rel = 2.0 ** -19 + 1.5 * E32 * sens
        whole = Phi < 2.0 ** -120
        f32 = x * (0.5 * torch.erfc(x * -0.70710678118654752))
    img = ops.gelu_x3(x, kind)
    assert tuple(img.data.shape) == (1, 64, 1, 128) and img.data.dtype == torch.float16 and img.shape == (1, 64, 1, 64)
    hi, lo = img.planes()
    assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all())                 # finite everywhere, +-65504 included
    got = image_value(ops, img.data, 64)
    bound = (rel + 2.0 ** -22) * ref.abs() + 2.0 ** -25 + torch.where(whole, ref.abs(), torch.zeros_like(ref))
    excess = (got - ref).abs() - bound
    i = int(excess.argmax())
    print(f'gelu_x3 {kind}: max(|image - f64| - bound) {float(excess.max()):.3e} at x = {float(x.flatten()[i]):.6g}; '
          f'max|image - f64| / |f64| on the grid {float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).flatten()[:2046].max()):.3e}')
    assert float(excess.max()) <= 0
    # bit for bit the split of the float32 result of the same formula, wherever that result is well defined (finite)
    ok = torch.isfinite(f32)
    assert int(ok.sum()) >= 4094
    want = ops.split3_f16(torch.where(ok, f32, torch.zeros_like(f32)))
    wh, wl = ops.split_planes(want, 64)
    assert torch.equal(bits(hi)[ok], bits(wh)[ok]) and torch.equal(bits(lo)[ok], bits(wl)[ok])


def test_gelu_x3_refusals(ops):
    with pytest.raises(ValueError, match='gelu_x3: x must be a float32'):
        ops.gelu_x3(torch.zeros(1, 2, 1, 64, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match='gelu_x3: 40 channels'):
        ops.gelu_x3(torch.zeros(1, 2, 1, 40, device=DEV))
    with pytest.raises(ValueError, match='gelu_x3: kind'):
        ops.gelu_x3(torch.zeros(1, 2, 1, 64, device=DEV), 'gelu_new')


# ---- patchify --------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,S,patch,kpad', [(2, 56, 14, 640), (3, 64, 32, 3072)])
def test_patchify_x3(ops, n, S, patch, kpad):
    x = (torch.randn(n, 3, S, S, generator=g(S)) * 1.7).to(DEV)
    assert ops.patch_kpad(patch) == kpad
    K, gr = 3 * patch * patch, S // patch
    rows = F.unfold(x, patch, stride=patch).transpose(1, 2)                                   # [n, g*g, K], columns (c, py, px)
    rows = torch.cat([rows, torch.zeros(n, gr * gr, kpad - K, device=DEV)], 2).contiguous().view(n, gr, gr, kpad)
    img = ops.patchify_x3(x, patch)
    assert img.shape == (n, gr, gr, kpad) and tuple(img.data.shape) == (n, gr, gr, 2 * kpad) and img.data.dtype == torch.float16
    assert torch.equal(bits(img.data), bits(ops.split3_f16(rows)))
    hi, lo = img.planes()
    assert not bits(hi[..., K:]).any() and not bits(lo[..., K:]).any()                        # pad columns: +0 in both halves
    assert torch.equal(bits(ops.patchify_x3(x, patch, kpad).data), bits(img.data))
    buf = torch.empty(x.numel() + 1, device=DEV)                                              # an unaligned source
    buf[1:] = x.flatten()
    assert torch.equal(bits(ops.patchify_x3(buf[1:].view_as(x), patch).data), bits(img.data))


def test_patchify_x3_refusals(ops):
    x = torch.zeros(1, 3, 56, 56, device=DEV)
    with pytest.raises(ValueError, match='patchify_x3: kpad 600'):
        ops.patchify_x3(x, 14, 600)                        # covers 588, but is no multiple of 32
    with pytest.raises(ValueError, match='patchify_x3: kpad 576'):
        ops.patchify_x3(x, 14, 576)                        # a multiple of 32, but short of 588
    with pytest.raises(ValueError, match=r'is not \[n, 3, S, S\]'):
        ops.patchify_x3(torch.zeros(1, 3, 56, 28, device=DEV), 14)
    with pytest.raises(ValueError, match='not a multiple of the patch size'):
        ops.patchify_x3(x, 16)
    with pytest.raises(ValueError, match='patchify_x3: x must be a float32'):
        ops.patchify_x3(x.half(), 14)


# ---- tokens and head -------------------------------------------------------------------------------
def f32_ulp(ref):
    """the float32 ulp at a float64 value"""
    return 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 23)


def check_tokens_f32(ops, c, t):
    """dts_vit_tokens_f32 on n = 3 samples drawn from g(c + t): half an ulp from float64 and bit for bit torch's float32 add.
    -> (tokens, the generator, for the head's parameters)"""
    n, gen = 3, g(c + t)
    patches = torch.randn(n, t - 1, c, generator=gen).to(DEV)
    cls, pos = torch.randn(c, generator=gen).to(DEV), (0.5 * torch.randn(t, c, generator=gen)).to(DEV)
    ref = torch.cat([cls.double().expand(n, 1, c), patches.double()], 1) + pos.double()
    tok = ops.vit_tokens_f32(patches, cls, pos)
    assert tok.dtype == torch.float32 and tuple(tok.shape) == (n, t, c)
    worst = float(((tok.double() - ref).abs() / f32_ulp(ref)).max())
    print(f'vit_tokens_f32 c={c} t={t}: max|tokens - f64| = {worst:.3f} ulp')
    assert worst <= 1.0
    assert torch.equal(tok, torch.cat([cls.expand(n, 1, c), patches], 1) + pos)               # the correctly rounded sum
    return tok, gen


def check_head_f32(ops, tok, gen, c, t):
    """dts_vit_head_f32: LayerNorm of token 0 alone; a class token of mean 3 so that the mean matters.  -> (head, its float64 reference,
    the row it normalises, gamma, beta, eps)"""
    n = tok.shape[0]
    tokens = tok.clone()
    tokens[:, 0] += 3.0
    gamma, beta = (1.0 + 0.3 * torch.randn(c, generator=gen)).to(DEV), (0.5 * torch.randn(c, generator=gen)).to(DEV)
    eps = 1e-5
    x0 = tokens[:, 0].contiguous()
    href = F.layer_norm(x0.double(), (c,), gamma.double(), beta.double(), eps)
    h32 = F.layer_norm(x0, (c,), gamma, beta, eps)
    head = ops.vit_head_f32(tokens, gamma, beta, eps)
    assert head.dtype == torch.float32 and tuple(head.shape) == (n, c)
    err_k, err_t = float((head.double() - href).abs().max()), float((h32.double() - href).abs().max())
    print(f'vit_head_f32 c={c} t={t}: max|kernel - f64| {err_k:.3e}, max|torch f32 - f64| {err_t:.3e}, ratio {err_k / err_t:.3f}')
    assert err_t > 0 and err_k <= 2 * err_t
    tokens[:, 1:] = float('nan')                                                              # the other tokens are not read
    assert torch.equal(ops.vit_head_f32(tokens, gamma, beta, eps), head)
    return head, href, x0, gamma, beta, eps


@pytest.mark.parametrize('t', [2, 17, 257])
@pytest.mark.parametrize('c', [64, 1024])
def test_vit_tokens_and_head_f32(ops, c, t):
    tok, gen = check_tokens_f32(ops, c, t)
    head, _, x0, gamma, beta, eps = check_head_f32(ops, tok, gen, c, t)
    # the same arithmetic as layer_norm_x3 on that row
    assert torch.equal(head, ops.layer_norm_x3(x0.view(1, -1, c), gamma, beta, eps, want_f32=True, want_split=False).view(-1, c))


@pytest.mark.parametrize('t', [2, 17])
def test_vit_tokens_f32_four_channel_vectors(ops, t):
    """c = 68: a multiple of 4 but not of 8 -- the float32 form of vit_tokens_kernel owns 4 channels per thread where the 16-bit forms own 8"""
    check_tokens_f32(ops, 68, t)


@pytest.mark.parametrize('t', [2, 17])
@pytest.mark.parametrize('c', [8, 1544, 2048])
def test_vit_head_f32_widths(ops, c, t):
    """c = 8: one lane holds the row; 1544 = 193 vectors: the fourth register vector (i = 3 of row_norm_kernel) on a single lane; 2048: every
    lane full.  The kernel forms y in float64 and rounds once: half a float32 ulp of the float64 value plus float64 noise, asserted at one
    ulp; the smallest |reference| on these inputs is 2.9e-5, far from where the float64 noise could reach an ulp.
    Measured on an MI355X (a record, not the source of the bound): 0.465 to 0.500 ulp, 0.18 to 0.85 of torch-float32's error."""
    tok, gen = check_tokens_f32(ops, c, t)
    head, href, x0, gamma, beta, eps = check_head_f32(ops, tok, gen, c, t)
    worst = float(((head.double() - href).abs() / f32_ulp(href)).max())
    print(f'vit_head_f32 c={c} t={t}: max|head - f64| = {worst:.3f} ulp')
    assert worst <= 1.0
    if c % 32 == 0:                                                                          # dts_layer_norm_x3 takes multiples of 32 only
        assert torch.equal(head, ops.layer_norm_x3(x0.view(1, -1, c), gamma, beta, eps, want_f32=True, want_split=False).view(-1, c))


def test_vit_tokens_and_head_f32_refusals(ops):
    p = torch.zeros(2, 4, 64, device=DEV)
    with pytest.raises(ValueError, match='vit_tokens_f32: patches must be a float32'):
        ops.vit_tokens_f32(p.half(), torch.zeros(64, device=DEV), torch.zeros(5, 64, device=DEV))
    with pytest.raises(ValueError, match='vit_tokens_f32: cls'):
        ops.vit_tokens_f32(p, torch.zeros(64, device=DEV), torch.zeros(4, 64, device=DEV))
    with pytest.raises(ValueError, match='vit_head_f32: tokens must be a float32'):
        ops.vit_head_f32(p.half(), torch.ones(64, device=DEV), torch.ones(64, device=DEV))
    with pytest.raises(ValueError, match='vit_head_f32: 4096 channels'):
        ops.vit_head_f32(torch.zeros(1, 2, 4096, device=DEV), torch.ones(4096, device=DEV), torch.ones(4096, device=DEV))
    with pytest.raises(ValueError, match='vit_head_f32: gamma'):
        ops.vit_head_f32(p, torch.ones(32, device=DEV), torch.ones(64, device=DEV))


# ---- the split-precision 1x1 convolution at ragged token counts ----------------------------------------
def test_conv1x1_split_precision_takes_an_operand_of_4096_channels(ops):
    """ViT-L/14's fc2 reads 4096 channels: an image row of 8192 f16 = 16 KiB, which the convolution's page of zero rows (the source of the
    pixel rows past a ragged tile's end) has to cover"""
    n, t, c, cout, gen = 1, 17, 4096, 128, g(4096)
    x = torch.randn(n, t, 1, c, generator=gen).to(DEV)
    w = (torch.randn(cout, c, 1, 1, generator=gen) / math.sqrt(c)).to(DEV)
    ref = x.double().view(t, c) @ w.double().view(cout, c).T
    got = ops.conv2d(ops.SplitAct(ops.split3_f16(x), c), ops.pack_conv_weight(w, ops.F16X3))
    e = float((got.double().view(t, cout) - ref).abs().max()) / float(ref.abs().max())
    print(f'conv 1x1 f16x3 t={t} cin={c} cout={cout}: rel err {e:.2e}')
    assert bool(torch.isfinite(got).all()) and e < TOL_X3


@pytest.mark.parametrize('cout', [128, 384])
@pytest.mark.parametrize('t', [17, 257])
def test_conv1x1_split_precision_ragged_tokens(ops, t, cout):
    """[3, t, 1, 128]: 51 / 771 pixel rows, no multiple of 64 (nor of the 16-row MFMA tile), so the last pixel tile is ragged and the f32 output
    leaves through the accumulator-layout epilogue -- with bias, with a float32 residual, from a SplitAct operand, and as the attention's
    operand image (out_split2)."""
    n, c, gen = 3, 128, g(t + cout)
    x = torch.randn(n, t, 1, c, generator=gen).to(DEV)
    w = (torch.randn(cout, c, 1, 1, generator=gen) / math.sqrt(c)).to(DEV)
    bias, res = torch.randn(cout, generator=gen).to(DEV), torch.randn(n, t, 1, cout, generator=gen).to(DEV)
    w3 = ops.pack_conv_weight(w, ops.F16X3)
    lin = x.double().view(n * t, c) @ w.double().view(cout, c).T + bias.double()
    ref_plain, ref_res = lin.view(n, t, 1, cout), lin.view(n, t, 1, cout) + res.double()
    xs = ops.SplitAct(ops.split3_f16(x), c)
    out_res = ops.conv2d(x, w3, bias, residual=res)
    out_res_s = ops.conv2d(xs, w3, bias, residual=res)
    out_plain = ops.conv2d(xs, w3, bias)
    for name, got, ref in (('bias + residual, f32 operand', out_res, ref_res), ('bias + residual, SplitAct operand', out_res_s, ref_res),
                           ('bias, SplitAct operand', out_plain, ref_plain)):
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, t, 1, cout)
        e = float((got.double() - ref).abs().max()) / float(ref.abs().max())
        print(f'conv 1x1 f16x3 t={t} cout={cout} {name}: rel err {e:.2e}')
        assert bool(torch.isfinite(got).all()) and e < TOL_X3, (name, e)
    assert torch.equal(out_res, out_res_s)                                                   # the same image either way
    sq = ops.conv2d(xs, w3, bias, out_split2=True)
    assert isinstance(sq, ops.SplitQKV) and tuple(sq.data.shape) == (n, t, 1, 2 * cout) and sq.data.dtype == torch.float16
    assert torch.equal(bits(sq.data), bits(ops.split2_f16(out_plain)))
