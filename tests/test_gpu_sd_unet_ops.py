"""GPU: the three kernels of the SD U-Net's transformer blocks -- dts_cross_attention, dts_layer_norm, dts_geglu -- each against a torch
float64 reference computed from the SAME 16-bit-rounded inputs.  The bounds are derived below from the number formats and the kernels'
documented arithmetic (f32 accumulation, P stored in 16 bits); they were written before the kernels first ran and are not fitted to them.

Notation: u = unit roundoff of the storage type = 2^-8 (bfloat16, 8 significant bits) or 2^-11 (float16, 11 significant bits); e32 = 2^-24.

Cross-attention, one output o = sum_i p_i v_i / sum_i p_i with p_i = exp((s_i - max s) * scale), s_i = q.k_i:
  * 16-bit x 16-bit products are exact in f32; the f32 accumulation of s, the fused multiply-add that forms the exponent and exp2 (1 ulp)
    leave a relative error in p_i of at most ~ln2 * |exponent| * (a few e32) -- below 2^-16 for |exponent| <= 64; the f32 accumulation of
    P.V over <= 128 keys adds 128 e32 = 2^-17.  Together: <= 2^-15 * A, A = sum_i w_i |v_i| (w = softmax weights) >= |o|.
  * P is stored in 16 bits for the matrix core: p_i (1 + d_i), |d_i| <= u, in the numerator AND (the kernel sums the rounded P) in the
    denominator: |error| <= u * A (numerator) + u * |o| (denominator) <= 2 u A.
  * float16 only, an ALLOWANCE rather than an established property of this kernel: a p_i below 2^-14 (max p = 1 exactly) is a subnormal
    float16, and the project's convolution tests found the matrix cores to flush subnormal float16 inputs (csrc/dts_common.h, x3_split;
    tests/test_gpu_ops.py::test_conv2d_split_precision[tiny_values]).  Should such a p_i count as zero, the error is at most the sum over
    those keys of w_i (|v_i| + |o|); if the hardware keeps it, the term only loosens the bound, and with these inputs it is a few 1e-5 of
    the softmax mass.  (bfloat16 has f32's exponent range: no such term.)
  * the output is rounded once: u * |o|.
  bound = u |o| + 2 u A + 2^-15 A + flush.

LayerNorm, y = (x - m) r g + b with m, r = 1/sqrt(var + eps) in f32 from a row held in registers (two passes, no E[x^2] - m^2):
  * the mean of c values summed as <= 32 per lane and a 6-level tree: |dm| <= 40 e32 max|x|; it shifts x - m directly and the variance to
    first order by 2 sqrt(var) dm, i.e. r relatively by <= r dm; the sum of squares adds 40 e32 relative to var, r by half of that, and
    the square root and division 2 e32: |d xhat| <= r dm (1 + |xhat|) + |xhat| 2^-19;
  * the affine step in f32 and the final rounding: (u + 2^-22) |y| + 2^-22 |b|.
  bound = u |y| + |g| (r dm (1 + |xhat|) + 2^-19 |xhat|) + 2^-22 (|y| + |b|).

GEGLU, out = a * g * Phi(g), Phi(g) = erfc(-g / sqrt 2) / 2 (the exact erf GELU without the cancellation of 1 + erf for negative g):
  * the argument -g * f32(1/sqrt 2) carries the constant's representation error (e32 / 2) and the product's rounding (e32): 1.5 e32
    relative, which moves Phi relatively by 1.5 e32 * sens(g), sens(g) = |g| phi(g) / Phi(g) (~g^2 for negative g: 100 at g = -10, where
    Phi = 7.6e-24; below 0.5 for positive g);
  * erfc of the device library is specified to 16 ulp (OpenCL's bound) and three multiplies add 3: < 32 e32 = 2^-19 relative;
  * the output rounding adds u, and a float16 result below 2^-14 is spaced 2^-24 apart: + 2^-25.
  bound = (u + 2^-19 + 1.5 e32 sens(g)) |out| + [float16] 2^-25.
"""
import math

import pytest
import torch

import launch_rules as LR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = [torch.float16, torch.bfloat16]


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


def g(seed):
    return torch.Generator().manual_seed(seed)


def xattn_reference(q, kv, heads, scale, dtype, kv_rows=None):
    """float64 on the device from the rounded inputs: (o, bound) per output element"""
    n, tq, c = q.shape
    d = c // heads
    q64, kv64 = q.double(), kv.double()
    if kv_rows is not None:
        kv64 = kv64[kv_rows.long()]
    tk = kv64.shape[1]
    qh = q64.view(n, tq, heads, d).permute(0, 2, 1, 3)                    # [n, h, tq, d]
    kh = kv64[..., :c].reshape(n, tk, heads, d).permute(0, 2, 1, 3)
    vh = kv64[..., c:].reshape(n, tk, heads, d).permute(0, 2, 1, 3)
    s = torch.einsum('nhqd,nhkd->nhqk', qh, kh) * scale
    p = torch.exp(s - s.amax(-1, keepdim=True))                           # max p = 1, as in the kernel
    w = p / p.sum(-1, keepdim=True)
    o = torch.einsum('nhqk,nhkd->nhqd', w, vh)
    A = torch.einsum('nhqk,nhkd->nhqd', w, vh.abs())
    u = U[dtype]
    bound = u * o.abs() + 2 * u * A + 2.0 ** -15 * A
    if dtype == torch.float16:
        wf = torch.where(p < 2.0 ** -14 * (1 + 2.0 ** -10), w, torch.zeros_like(w))
        bound = bound + torch.einsum('nhqk,nhkd->nhqd', wf, vh.abs()) + wf.sum(-1, keepdim=True) * o.abs()
    back = lambda t: t.permute(0, 2, 1, 3).reshape(n, tq, c)
    return back(o), back(bound)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('d', [64, 128, 256])
@pytest.mark.parametrize('tq', [1, 64, 4096])
@pytest.mark.parametrize('tk', [1, 11, 77, 128])
def test_cross_attention(ops, dtype, d, tq, tk):
    n, heads = 2, 2
    gen = g(1000 * tk + tq + d)
    c = heads * d
    q = (torch.randn(n, tq, c, generator=gen) * 1.5).to(DEV, dtype)
    kv = torch.randn(n, tk, 2 * c, generator=gen).to(DEV, dtype)
    scale = 1.0 / math.sqrt(d)
    ref, bound = xattn_reference(q, kv, heads, scale, dtype)
    out = ops.cross_attention(q, kv, heads, scale)
    assert out.dtype == dtype and tuple(out.shape) == (n, tq, c)
    err = (out.double() - ref).abs()
    worst = float((err / bound).max())
    print(f'cross_attention {str(dtype).split(".")[-1]} d={d} tq={tq} tk={tk}: max err {float(err.max()):.3e}, max err/bound {worst:.3f}')
    assert torch.isfinite(out).all() and worst <= 1.0


@pytest.mark.parametrize('dtype', DTYPES)
def test_cross_attention_shared_contexts_padded_heads_and_odd_lengths(ops, dtype):
    """The SD U-Net's use: 6 rows over 2 distinct text contexts through kv_rows (no expanded copy), 8 heads of true dim 40 zero-padded to
    64 with scale 1/sqrt(40), 77 keys, a query count that is not a multiple of 16; and every ragged key length around the 32-key steps."""
    gen = g(7)
    heads, d, dt_, n = 8, 64, 40, 6
    c = heads * d
    pad = torch.zeros(heads, d)
    pad[:, :dt_] = 1
    pad = pad.reshape(c)
    q = (torch.randn(n, 100, c, generator=gen) * 2 * pad).to(DEV, dtype)
    kv = (torch.randn(2, 77, 2 * c, generator=gen) * torch.cat([pad, pad])).to(DEV, dtype)
    rows = torch.tensor([0, 0, 0, 1, 1, 1], dtype=torch.int32, device=DEV)
    scale = 1.0 / math.sqrt(dt_)
    ref, bound = xattn_reference(q, kv, heads, scale, dtype, kv_rows=rows)
    out = ops.cross_attention(q, kv, heads, scale, kv_rows=rows)
    assert float(((out.double() - ref).abs() / bound.clamp_min(1e-300)).max()) <= 1.0
    assert torch.equal(out, ops.cross_attention(q, kv[rows.long()].contiguous(), heads, scale))         # the map is only an indirection
    assert not out.view(n, 100, heads, d)[..., dt_:].any()                                              # padded value channels stay zero
    for tk in (2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127):
        kv2 = torch.randn(1, tk, 2 * c, generator=gen).to(DEV, dtype)
        q2 = torch.randn(1, 37, c, generator=gen).to(DEV, dtype)
        ref, bound = xattn_reference(q2, kv2, heads, 0.125, dtype)
        out = ops.cross_attention(q2, kv2, heads, 0.125)
        assert float(((out.double() - ref).abs() / bound).max()) <= 1.0, tk


GUARD = 4096


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', LR.XATTN_CHUNK_LOOP, ids=lambda c: f'n{c.n}-h{c.heads}-d{c.d}-tq{c.tq}-tk{c.tk}')
def test_cross_attention_chunk_loop(ops, dtype, case):
    """The loop `for (qc = 0; qc < qchunks; ++qc)` of cross_attention_kernel at qchunks = 2, 4 and 8 (every other test of this file runs it
    at 1; the SD U-Net at 16 candidates runs 8): q0 = (qblk * qchunks + qc) * 64 + wid * 16 for qc > 0, a ragged last chunk, and a last
    block whose chunks run past tq (the wave-uniform break).  Nothing reports which form ran: launch_rules.xattn_plan restates the
    launcher's rule and the table says what each shape must reach (asserted here and, without a GPU, in tests/test_launch_rules.py).
    The output is the middle of a NaN-filled buffer: every row written, nothing outside.  xattn_reference and its bound, unchanged.
    Measured on an MI355X (a record, not the source of the bound): max err/bound 0.34 .. 0.40 over the ten cases (the older cases of this
    file: the same range), 0.30 .. 0.40 in every chunk slot of a block."""
    n, heads, d, tq, tk = case.n, case.heads, case.d, case.tq, case.tk
    assert LR.xattn_plan(n, heads, tq) == (case.chunks, case.qchunks, case.qblocks) and case.qchunks > 1
    gen = g(1000 * tk + tq + d + n)
    c = heads * d
    q = (torch.randn(n, tq, c, generator=gen) * 1.5).to(DEV, dtype)
    m = n if case.contexts is None else case.contexts
    kv = torch.randn(m, tk, 2 * c, generator=gen).to(DEV, dtype)
    rows = None if case.contexts is None else (torch.arange(n, dtype=torch.int32) * 7 % m).to(DEV)
    scale = 1.0 / math.sqrt(d)
    buf = torch.full((n * tq * c + 2 * GUARD,), float('nan'), dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n * tq * c].view(n, tq, c)
    out = ops.cross_attention(q, kv, heads, scale, kv_rows=rows, out=view)
    assert out is view
    assert not bool(torch.isnan(out).any()), 'an output row was never written'
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), 'a store outside the output'
    ref, bound = xattn_reference(q, kv, heads, scale, dtype, kv_rows=rows)
    ratio = (out.double() - ref).abs() / bound
    del ref, bound
    worst = float(ratio.max())
    # per chunk position inside a block: a fault in the q0 of one qc shows there
    per_qc = [float(ratio[:, [t for t in range(tq) if (t // 64) % case.qchunks == qc]].max()) for qc in range(case.qchunks)]
    print(f'cross_attention chunk loop {str(dtype).split(".")[-1]} n={n} heads={heads} d={d} tq={tq} tk={tk}: qchunks {case.qchunks}, qblocks '
          f'{case.qblocks}; max err/bound {worst:.3f}; per chunk slot {" ".join(f"{r:.3f}" for r in per_qc)}')
    assert worst <= 1.0
    if rows is not None:
        assert rows.unique().numel() == m


def test_cross_attention_out_argument(ops):
    """out=: the op writes and returns the caller's tensor, and refuses one of another shape, type or layout"""
    q = torch.randn(2, 70, 128, generator=g(3)).to(DEV, torch.float16)
    kv = torch.randn(2, 9, 256, generator=g(4)).to(DEV, torch.float16)
    out = torch.empty_like(q)
    assert ops.cross_attention(q, kv, 2, 0.125, out=out) is out and torch.equal(out, ops.cross_attention(q, kv, 2, 0.125))
    for bad in (torch.empty(2, 70, 64, dtype=torch.float16, device=DEV), torch.empty(2, 70, 128, dtype=torch.bfloat16, device=DEV),
                torch.empty(2, 70, 128, dtype=torch.float16), torch.empty(2, 70, 256, dtype=torch.float16, device=DEV)[..., ::2]):
        with pytest.raises(ValueError):
            ops.cross_attention(q, kv, 2, 0.125, out=bad)


def test_cross_attention_refuses_what_it_cannot_compute(ops):
    c = 128
    q = torch.zeros(1, 16, c, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match=r'\(-3\).*129 keys'):                   # DTS_ERR_UNSUPPORTED, with a message
        ops.cross_attention(q, torch.zeros(1, 129, 2 * c, dtype=torch.float16, device=DEV), 2, 0.125)
    with pytest.raises(RuntimeError, match='head dim 32'):
        ops.cross_attention(q, torch.zeros(1, 8, 2 * c, dtype=torch.float16, device=DEV), 4, 0.125)
    with pytest.raises(RuntimeError, match='16-bit'):
        ops.cross_attention(q.float(), torch.zeros(1, 8, 2 * c, device=DEV), 2, 0.125)
    with pytest.raises(ValueError):
        ops.cross_attention(q, torch.zeros(2, 8, 2 * c, dtype=torch.float16, device=DEV), 2, 0.125)   # 2 kv rows, 1 sample, no map


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c', [8, 64, 320, 1280, 1544, 2048])
def test_layer_norm(ops, dtype, c):
    """c = 8: one lane holds the row; 1544 = 193 vectors: the fourth register vector (i = 3) on a single lane; 2048: all four whole
    (launch_rules.LAYER_NORM_WIDTHS).  The widths up to 1280 stay inside three.
    Measured on an MI355X (float16 / bfloat16; a record, not the source of the bound, which the output rounding u |y| nearly fills by
    itself): c = 8: 0.928 / 0.943, c = 1544: 0.956 / 0.991, c = 2048: 0.983 / 0.990."""
    if c in LR.LAYER_NORM_WIDTHS:
        assert LR.layer_norm_vectors(c) == LR.LAYER_NORM_WIDTHS[c]
    gen = g(20 + c)
    rows = 37
    x = torch.randn(rows, c, generator=gen) * 1.5 + 0.3
    x[1] = 100.0 + 0.5 * torch.randn(c, generator=gen)            # large mean, small variance (the storage type's spacing at 100 is coarse)
    x[2] = -3.0e3 + 40.0 * torch.randn(c, generator=gen)
    x[3] = 1e-3 * torch.randn(c, generator=gen)
    x = x.to(DEV, dtype)
    gamma = (1.0 + 0.3 * torch.randn(c, generator=gen)).to(DEV)
    beta = (0.2 * torch.randn(c, generator=gen)).to(DEV)
    eps = 1e-5
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    m = x64.mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(x64.var(-1, unbiased=False, keepdim=True) + eps)
    xhat = (x64 - m) * r
    ref = xhat * g64 + b64
    u, e32 = U[dtype], 2.0 ** -24
    dm = 40 * e32 * x64.abs().amax(-1, keepdim=True)
    bound = u * ref.abs() + g64.abs() * (r * dm * (1 + xhat.abs()) + 2.0 ** -19 * xhat.abs()) + 2.0 ** -22 * (ref.abs() + b64.abs())
    out = ops.layer_norm(x.view(1, rows, c), gamma, beta, eps).view(rows, c)
    err = (out.double() - ref).abs()
    worst = float((err / bound).max())
    print(f'layer_norm {str(dtype).split(".")[-1]} c={c}: max err {float(err.max()):.3e}, max err/bound {worst:.3f}')
    assert out.dtype == dtype and worst <= 1.0


def test_layer_norm_refuses_bad_shapes(ops):
    with pytest.raises(RuntimeError, match='channels'):
        ops.layer_norm(torch.zeros(4, 20, dtype=torch.float16, device=DEV), torch.ones(20, device=DEV), torch.zeros(20, device=DEV))
    with pytest.raises(RuntimeError, match='16-bit'):
        ops.layer_norm(torch.zeros(4, 64, device=DEV), torch.ones(64, device=DEV), torch.zeros(64, device=DEV))


@pytest.mark.parametrize('dtype', DTYPES)
def test_geglu(ops, dtype):
    gen = g(31)
    rows, inner = 50, 1280
    x = (torch.rand(rows, 2 * inner, generator=gen) * 20 - 10)
    x[0, inner:inner + 8] = torch.tensor([-10.0, 10.0, 0.0, -0.0, -6.0, -1e-3, 1e-3, 3.0])
    x[0, :8] = 10.0
    x = x.to(DEV, dtype)
    x64 = x.double()
    a, gate = x64[:, :inner], x64[:, inner:]
    ref = a * gate * (0.5 * torch.special.erfc(-gate / math.sqrt(2.0)))
    same = a * (0.5 * gate * (1.0 + torch.erf(gate / math.sqrt(2.0))))                       # the erf form of the definition
    assert float((ref - same).abs().max()) < 1e-13
    phi, Phi = torch.exp(-0.5 * gate * gate) / math.sqrt(2 * math.pi), 0.5 * torch.special.erfc(-gate / math.sqrt(2.0))
    sens = gate.abs() * phi / Phi
    bound = (U[dtype] + 2.0 ** -19 + 1.5 * 2.0 ** -24 * sens) * ref.abs() + (2.0 ** -25 if dtype == torch.float16 else 0.0)
    out = ops.geglu(x.view(2, rows // 2, 2 * inner)).view(rows, inner)
    err = (out.double() - ref).abs()
    ok = err <= bound
    print(f'geglu {str(dtype).split(".")[-1]}: max err {float(err.max()):.3e}, max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}')
    assert out.dtype == dtype and bool(ok.all())
    with pytest.raises(RuntimeError, match='inner'):
        ops.geglu(torch.zeros(4, 24, dtype=dtype, device=DEV))
