"""GPU: the four kernels of the CLIP vision tower -- dts_patchify, dts_vit_tokens, dts_gelu, dts_vit_head -- in float16 and bfloat16.

patchify and vit_tokens move or add values with ONE rounding, so they are compared bit for bit with torch (`unfold` + `.to(dtype)`;
`(patches.float() + pos).to(dtype)`: an f32 sum rounded to nearest-even is the same number on both sides).

gelu and the head are compared with float64; the bounds are derived here from the number formats and the kernels' documented arithmetic,
and were written before the kernels first ran.  u = unit roundoff of the storage type = 2^-11 (float16) / 2^-8 (bfloat16) = half an ulp
relative; e32 = 2^-24.

gelu, kind 0 (quick-GELU), out = x / (1 + exp(-z)), z = 1.702 x:
  * z carries the representation error of the f32 constant and the product's rounding: <= 2 e32 relative; d log sigmoid(z) / d log z =
    z sigmoid(-z), so sigmoid moves relatively by 2 e32 * sens, sens = |z| sigmoid(-z) (<= 0.28 for z > 0, ~|z| for negative z);
  * expf to 2 ulp (4 e32; on 1 / (1 + e) it weighs e / (1 + e) <= 1), the sum e32, the quotient 2.5 ulp (5 e32): together < 2^-20;
  * the output rounding: u |out| (half an ulp of the storage type); a float16 result below 2^-14 is spaced 2^-24 apart: + 2^-25
    (bfloat16 subnormals: + 2^-134);
  * where exp(-z) leaves the f32 range (z < -87) the kernel returns -0 for a true value below 2^-110 in magnitude: the whole value is
    allowed there.  That is the point of the quotient form: the result is FINITE for every finite input.
  bound = (u + 2^-20 + 2 e32 sens) |out| + subnormal spacing [+ |out| where z < -87].
gelu, kind 1 (erf), out = x Phi(x), Phi(x) = erfc(-x / sqrt 2) / 2: the GEGLU bound of tests/test_gpu_sd_unet_ops.py without the linear
  half: (u + 2^-19 + 1.5 e32 sens) |out| + subnormal spacing, sens = |x| phi(x) / Phi(x); the whole value where Phi < 2^-120 (erfc
  leaves the f32 normal range: -0 is returned).

head, y = (x0 - m) r g + b in f32 from the class token's 16-bit row, then the f32 projection y . W^T:
  * against float64 from the SAME rounded token, the LayerNorm bound of tests/test_gpu_sd_unet_ops.py without its output rounding (the
    head writes f32): |g| (r dm (1 + |xhat|) + 2^-19 |xhat|) + 2^-22 (|y| + |b|), dm = 40 e32 max|x|; the projection adds, for any
    summation order of c products, (c + 1) e32 sum_j |W_ij| |y_j| and carries the error of y through |W|;
  * against float64 from the UNROUNDED token x (x' = x (1 + d), |d| <= u): with e_i = u (|x_i| + mean|x|) and E = u (rms|x| + mean|x|),
    the centred row moves by at most e_i and s = sqrt(var + eps) by at most E (it is a norm: triangle inequality), so
    |xhat' - xhat| <= (e_i + |xhat_i| E) / (s - E); times |g|, plus the arithmetic bound above.
"""
import math

import pytest
import torch

import launch_rules as LR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUB = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}          # half the spacing of the type's subnormals
DTYPES = [torch.float16, torch.bfloat16]
E32 = 2.0 ** -24


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


def g(seed):
    return torch.Generator().manual_seed(seed)


def nan_filled(shape, dtype):
    """a buffer whose every element is a NaN bit pattern of the 16-bit type (0x7FFF)"""
    return torch.full(shape, 0x7FFF, dtype=torch.int16, device=DEV).view(dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,S,patch,kpad', [(2, 56, 14, 640), (3, 64, 32, 3072)])
def test_patchify(ops, dtype, n, S, patch, kpad):
    x = (torch.randn(n, 3, S, S, generator=g(S)) * 1.7).to(DEV)
    assert ops.patch_kpad(patch) == kpad
    K, gg = 3 * patch * patch, (S // patch) ** 2
    out = nan_filled((n, gg, kpad), dtype)
    assert bool(torch.isnan(out).all())
    got = ops.patchify(x, patch, dtype, out=out)
    assert got.data_ptr() == out.data_ptr() and got.dtype == dtype
    ref = torch.nn.functional.unfold(x, patch, stride=patch).transpose(1, 2).to(dtype)        # [n, gg, K], columns (c, py, px)
    assert torch.equal(got[..., :K].contiguous().view(torch.int16), ref.contiguous().view(torch.int16))
    assert not got[..., K:].contiguous().view(torch.int16).any()                              # pad columns: +0 exactly
    assert torch.equal(ops.patchify(x, patch, dtype), got)                                    # the allocating form
    # an unaligned source: the same image one float into its storage
    buf = torch.empty(x.numel() + 1, device=DEV)
    buf[1:] = x.flatten()
    assert torch.equal(ops.patchify(buf[1:].view_as(x), patch, dtype), got)


def test_patchify_refuses_bad_shapes(ops):
    x = torch.zeros(1, 3, 60, 60, device=DEV)
    with pytest.raises(ValueError, match='60'):
        ops.patchify(x, 14, torch.float16)
    with pytest.raises(ValueError, match=r'\[n, 3, S, S\]'):
        ops.patchify(torch.zeros(1, 4, 56, 56, device=DEV), 14, torch.float16)
    with pytest.raises(RuntimeError, match='16-bit'):
        ops.patchify(torch.zeros(1, 3, 56, 56, device=DEV), 14, torch.float32)
    with pytest.raises(RuntimeError, match='kpad'):
        ops.patchify(torch.zeros(1, 3, 56, 56, device=DEV), 14, torch.float16, kpad=584)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('T', [17, 50])
@pytest.mark.parametrize('c', [64, 1024])
def test_vit_tokens(ops, dtype, T, c):
    gen = g(T + c)
    n = 2
    patches = torch.randn(n, T - 1, c, generator=gen).to(DEV, dtype)
    cls = torch.randn(c, generator=gen).to(DEV)
    pos = (0.5 * torch.randn(T, c, generator=gen)).to(DEV)
    got = ops.vit_tokens(patches, cls, pos)
    full = torch.cat([cls.expand(n, 1, c), patches.float()], 1)                               # the class row first
    ref = (full + pos).to(dtype)
    assert got.dtype == dtype and tuple(got.shape) == (n, T, c)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    with pytest.raises(ValueError, match='pos'):
        ops.vit_tokens(patches, cls, pos[:-1].contiguous())
    with pytest.raises(RuntimeError, match='16-bit'):
        ops.vit_tokens(patches.float(), cls, pos)


def gelu_inputs(dtype):
    big = torch.finfo(dtype).max
    special = torch.tensor([20.0, -20.0, big, -big, 0.0, -0.0, 1.0, -1.0, 6.0, -6.0, 1e-3, -1e-3])
    count = 8 * (256 * 3 + 5)                                   # three full blocks of 256 vectors and a last block of 5
    x = torch.randn(count, generator=g(3)) * 2.5
    x[:special.numel()] = special
    x[-special.numel():] = special.flip(0)                      # the tail block sees them too
    return x.to(DEV, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', ['quick_gelu', 'gelu'])
def test_gelu(ops, dtype, kind):
    x = gelu_inputs(dtype)
    assert bool(torch.isfinite(x).all()) and float(x.max()) == torch.finfo(dtype).max
    x64 = x.double()
    u = U[dtype]
    if kind == 'quick_gelu':
        z = 1.702 * x64
        ref = x64 * torch.sigmoid(z)
        sens = z.abs() * torch.sigmoid(-z)
        bound = (u + 2.0 ** -20 + 2 * E32 * sens) * ref.abs() + SUB[dtype] + torch.where(z < -87.0, ref.abs(), torch.zeros_like(ref))
    else:
        Phi = 0.5 * torch.special.erfc(-x64 / math.sqrt(2.0))
        ref = x64 * Phi
        phi = torch.exp(-0.5 * x64 * x64) / math.sqrt(2 * math.pi)
        sens = torch.where(Phi > 0, x64.abs() * phi / Phi.clamp_min(1e-300), torch.zeros_like(x64))
        bound = (u + 2.0 ** -19 + 1.5 * E32 * sens) * ref.abs() + SUB[dtype] + torch.where(Phi < 2.0 ** -120, ref.abs(), torch.zeros_like(ref))
    out = ops.gelu(x, kind)
    err = (out.double() - ref).abs()
    worst = float((err / bound).max())
    print(f'gelu[{kind}] {str(dtype).split(".")[-1]}: max err {float(err.max()):.3e}, max err/bound {worst:.3f}')
    assert out.dtype == dtype and out.shape == x.shape
    assert bool(torch.isfinite(out).all())                                                    # -max -> -0, never inf * 0
    assert worst <= 1.0
    big = torch.finfo(dtype).max
    lo, hi = out[x == -big], out[x == big]
    assert lo.numel() == 2 and not lo.any() and bool((hi == big).all())
    inplace = x.clone()
    assert ops.gelu(inplace, kind, out=inplace) is inplace and torch.equal(inplace, out)


def test_gelu_refuses_bad_arguments(ops):
    with pytest.raises(ValueError, match='gelu_new'):
        ops.gelu(torch.zeros(8, dtype=torch.float16, device=DEV), 'gelu_new')
    with pytest.raises(RuntimeError, match='multiple of 8'):
        ops.gelu(torch.zeros(12, dtype=torch.float16, device=DEV))
    with pytest.raises(RuntimeError, match='16-bit'):
        ops.gelu(torch.zeros(8, device=DEV))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c', [8, 128, 1024, 1544, 2048])
def test_head(ops, dtype, c):
    """c = 8: one lane holds the row; 1544 = 193 vectors: the fourth register vector (i = 3 of row_norm_kernel) on a single lane; 2048: all
    four whole (launch_rules.LAYER_NORM_WIDTHS).
    Measured on an MI355X (err/bound of the LayerNorm, float16 / bfloat16; a record, not the source of any bound): against the rounded token
    c = 8: 0.010 / 0.013, c = 1544: 0.010 / 0.009, c = 2048: 0.018 / 0.015; against the unrounded token 0.160 / 0.220, 0.297 / 0.301,
    0.294 / 0.325; the projection stays below 0.02 (0.16 against the unrounded token at c = 8)."""
    if c in LR.LAYER_NORM_WIDTHS:
        assert LR.layer_norm_vectors(c) == LR.LAYER_NORM_WIDTHS[c]
    gen = g(40 + c)
    n, T, proj = 3, 5, 96
    xf = torch.randn(n, T, c, generator=gen) * 1.5 + 0.3
    xf[1, 0] = 30.0 + 0.5 * torch.randn(c, generator=gen)                 # a class token with a large mean and a small variance
    tokens = xf.to(DEV, dtype)
    gamma = (1.0 + 0.3 * torch.randn(c, generator=gen)).to(DEV)
    beta = (0.2 * torch.randn(c, generator=gen)).to(DEV)
    W = (torch.randn(proj, c, generator=gen) / math.sqrt(c)).to(DEV)
    eps, u = 1e-5, U[dtype]
    g64, b64, W64 = gamma.double(), beta.double(), W.double()

    def ln64(x):
        m = x.mean(-1, keepdim=True)
        s = torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps)
        xhat = (x - m) / s
        return xhat, s, xhat * g64 + b64

    # (a) float64 from the token the kernel reads: f32 arithmetic only
    x_r = tokens[:, 0].double()
    xhat, s, y_ref = ln64(x_r)
    dm = 40 * E32 * x_r.abs().amax(-1, keepdim=True)
    bound_y = g64.abs() * (dm / s * (1 + xhat.abs()) + 2.0 ** -19 * xhat.abs()) + 2.0 ** -22 * (y_ref.abs() + b64.abs())
    y = ops.vit_head(tokens, gamma, beta, eps)
    assert y.dtype == torch.float32 and tuple(y.shape) == (n, c)
    err_y = (y.double() - y_ref).abs()
    out = ops.linear(y, W)
    out_ref = y_ref @ W64.T
    bound_out = bound_y @ W64.abs().T + (c + 1) * E32 * (y_ref.abs() @ W64.abs().T)
    err_out = (out.double() - out_ref).abs()
    print(f'head {str(dtype).split(".")[-1]} c={c}: LayerNorm max err {float(err_y.max()):.3e} (err/bound {float((err_y / bound_y).max()):.3f}), '
          f'projected max err {float(err_out.max()):.3e} (err/bound {float((err_out / bound_out).max()):.3f})')
    assert float((err_y / bound_y).max()) <= 1.0 and float((err_out / bound_out).max()) <= 1.0

    # (b) float64 from the token before its 16-bit rounding
    x_u = xf[:, 0].to(DEV).double()
    xhat_u, s_u, y_u = ln64(x_u)
    mean_abs = x_u.abs().mean(-1, keepdim=True)
    e_i = u * (x_u.abs() + mean_abs)
    E = u * (torch.sqrt((x_u * x_u).mean(-1, keepdim=True)) + mean_abs)
    assert bool((E < 0.5 * s_u).all())
    bound_in = g64.abs() * (e_i + xhat_u.abs() * E) / (s_u - E)
    bound_yu = bound_in + bound_y
    err_yu = (y.double() - y_u).abs()
    bound_outu = bound_yu @ W64.abs().T + (c + 1) * E32 * (y_ref.abs() @ W64.abs().T)
    err_outu = (out.double() - y_u @ W64.T).abs()
    print(f'   against the unrounded token: LayerNorm err/bound {float((err_yu / bound_yu).max()):.3f}, projected {float((err_outu / bound_outu).max()):.3f}')
    assert float((err_yu / bound_yu).max()) <= 1.0 and float((err_outu / bound_outu).max()) <= 1.0

    # the other tokens are not read: poisoning them changes nothing
    poisoned = tokens.clone()
    poisoned[:, 1:] = float('nan')
    assert torch.equal(ops.vit_head(poisoned, gamma, beta, eps), y)


def test_head_refuses_bad_shapes(ops):
    with pytest.raises(RuntimeError, match='channels'):
        ops.vit_head(torch.zeros(2, 3, 4096, dtype=torch.float16, device=DEV), torch.ones(4096, device=DEV), torch.zeros(4096, device=DEV))
    with pytest.raises(RuntimeError, match='16-bit'):
        ops.vit_head(torch.zeros(2, 3, 64, device=DEV), torch.ones(64, device=DEV), torch.zeros(64, device=DEV))
    with pytest.raises(ValueError, match='gamma'):
        ops.vit_head(torch.zeros(2, 3, 64, dtype=torch.float16, device=DEV), torch.ones(32, device=DEV), torch.zeros(64, device=DEV))
