"""Cross-attention at the head dims of SD-1.x, 40 / 80 / 160, stored unpadded (csrc/transformer.hip: cross_attention_kernel with a head
dim in memory below its on-chip K width).  q [n, tq, heads * d], kv [m, tk, 2 * heads * d] (k | v), out [n, tq, heads * d], all at the TRUE
head dim; three heads, so that head offsets of 80 h, 160 h and 320 h bytes all occur.

Every case is held to the float64 reference and bound of tests/test_gpu_sd_unet_ops.py (xattn_reference, restated here unchanged:
bound = u |o| + 2 u A + 2^-15 A + [float16] flush, derived there from the number formats before the kernel first ran), at scale
1 / sqrt(d) of the true head dim -- and to the padded route bit for bit: the same values zero-padded per head to 64 / 128 / 256 through the
kernel of that head dim.  A zero tail adds exact zeros to the f32 scores and the value tiles that hold a channel < d see the same P and the
same keys in the same order, so the outputs are equal and the padded channels zero."""
import math

import pytest
import torch

import launch_rules as LR

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTYPES = [torch.float16, torch.bfloat16]
DIMS = [40, 80, 160]
PADDED = {40: 64, 80: 128, 160: 256}
N, HEADS = 2, 3


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


def g(seed):
    return torch.Generator().manual_seed(seed)


def name(dtype):
    return str(dtype).split('.')[-1]


def xattn_reference(q, kv, heads, scale, dtype, kv_rows=None):
    """float64 on the device from the rounded inputs: (o, bound) per output element (tests/test_gpu_sd_unet_ops.py's, restated)"""
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


def pad_heads(x, heads, d, dp, blocks):
    """[n, t, blocks * heads * d] -> [n, t, blocks * heads * dp]: every head's d channels followed by dp - d zeros"""
    n, t, _ = x.shape
    out = torch.zeros((n, t, blocks, heads, dp), dtype=x.dtype, device=x.device)
    out[..., :d] = x.view(n, t, blocks, heads, d)
    return out.view(n, t, blocks * heads * dp)


def equals_padded_route(ops, out, q, kv, heads, d, kv_rows=None):
    dp = PADDED[d]
    n, tq, _ = q.shape
    pad = ops.cross_attention(pad_heads(q, heads, d, dp, 1), pad_heads(kv, heads, d, dp, 2), heads, 1.0 / math.sqrt(d), kv_rows=kv_rows)
    pad = pad.view(n, tq, heads, dp)
    return torch.equal(out.view(n, tq, heads, d), pad[..., :d]) and not bool(pad[..., d:].any())


@pytest.mark.parametrize('dtype', DTYPES, ids=name)
@pytest.mark.parametrize('d', DIMS)
def test_against_float64_and_the_padded_route(ops, dtype, d):
    bad = []
    c = HEADS * d
    scale = 1.0 / math.sqrt(d)
    for tq in (1, 37, 100):
        for tk in (1, 11, 77, 128):
            gen = g(1000 * tk + tq + d)
            q = (torch.randn(N, tq, c, generator=gen) * 1.5).to(DEV, dtype)
            kv = torch.randn(N, tk, 2 * c, generator=gen).to(DEV, dtype)
            ref, bound = xattn_reference(q, kv, HEADS, scale, dtype)
            out = ops.cross_attention(q, kv, HEADS, scale)
            assert out.dtype == dtype and tuple(out.shape) == (N, tq, c)
            worst = float(((out.double() - ref).abs() / bound).max()) if bool(torch.isfinite(out).all()) else math.inf
            same = equals_padded_route(ops, out, q, kv, HEADS, d)
            print(f'cross_attention native {name(dtype)} d={d} tq={tq} tk={tk}: max err/bound {worst:.3f}, bit-identical to the padded route: {same}')
            if not (worst <= 1.0 and same):
                bad.append((tq, tk, worst, same))
    assert not bad, bad


@pytest.mark.parametrize('dtype', DTYPES, ids=name)
def test_shared_contexts_as_the_sd_unet_uses_them(ops, dtype):
    """6 rows over 2 distinct text contexts through kv_rows, 8 heads of 40, 77 keys, a query count that is not a multiple of 16"""
    gen = g(7)
    heads, d, n = 8, 40, 6
    c = heads * d
    q = (torch.randn(n, 100, c, generator=gen) * 2).to(DEV, dtype)
    kv = torch.randn(2, 77, 2 * c, generator=gen).to(DEV, dtype)
    rows = torch.tensor([0, 0, 0, 1, 1, 1], dtype=torch.int32, device=DEV)
    scale = 1.0 / math.sqrt(d)
    ref, bound = xattn_reference(q, kv, heads, scale, dtype, kv_rows=rows)
    out = ops.cross_attention(q, kv, heads, scale, kv_rows=rows)
    worst = float(((out.double() - ref).abs() / bound).max())
    print(f'cross_attention native {name(dtype)} 6 rows over 2 contexts, 8 heads of 40: max err/bound {worst:.3f}')
    assert bool(torch.isfinite(out).all()) and worst <= 1.0
    assert torch.equal(out, ops.cross_attention(q, kv[rows.long()].contiguous(), heads, scale))         # the map is only an indirection
    assert equals_padded_route(ops, out, q, kv, heads, d, kv_rows=rows)


GUARD = 4096


@pytest.mark.parametrize('dtype', DTYPES, ids=name)
def test_chunk_loop(ops, dtype):
    """two chunks of 64 queries per block (q0 of the second chunk, a ragged last chunk, a last block whose second chunk lies past tq) at
    head dim 40; the output is the middle of a NaN-filled buffer: every row written, nothing outside"""
    n, heads, d, tq, tk = 8, 16, 40, 1030, 77
    assert LR.xattn_plan(n, heads, tq) == (17, 2, 9)
    gen = g(1000 * tk + tq + d + n)
    c = heads * d
    q = (torch.randn(n, tq, c, generator=gen) * 1.5).to(DEV, dtype)
    kv = torch.randn(n, tk, 2 * c, generator=gen).to(DEV, dtype)
    scale = 1.0 / math.sqrt(d)
    buf = torch.full((n * tq * c + 2 * GUARD,), float('nan'), dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n * tq * c].view(n, tq, c)
    out = ops.cross_attention(q, kv, heads, scale, out=view)
    assert out is view
    assert not bool(torch.isnan(out).any()), 'an output element was never written'
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), 'a store outside the output'
    ref, bound = xattn_reference(q, kv, heads, scale, dtype)
    ratio = (out.double() - ref).abs() / bound
    del ref, bound
    per_qc = [float(ratio[:, [t for t in range(tq) if (t // 64) % 2 == qc]].max()) for qc in range(2)]
    print(f'cross_attention native chunk loop {name(dtype)} n={n} heads={heads} d={d} tq={tq} tk={tk}: max err/bound per chunk slot '
          + ' '.join(f'{r:.3f}' for r in per_qc))
    assert max(per_qc) <= 1.0


@pytest.mark.parametrize('dtype', DTYPES, ids=name)
@pytest.mark.parametrize('d', DIMS)
def test_neighbouring_heads_are_never_read_into_a_result(ops, dtype, d):
    """per (sample, head): with NaN in every channel of the other two heads of q and kv and in the whole other sample, that head's output
    is the clean run's bit for bit -- a 16-byte chunk loaded past d would be the next head's, a store past d would land in its output"""
    tq, tk = 37, 77
    c = HEADS * d
    gen = g(d)
    q = torch.randn(N, tq, c, generator=gen).to(DEV, dtype)
    kv = torch.randn(N, tk, 2 * c, generator=gen).to(DEV, dtype)
    scale = 1.0 / math.sqrt(d)
    clean = ops.cross_attention(q, kv, HEADS, scale)
    assert bool(torch.isfinite(clean).all())
    for s in range(N):
        for h in range(HEADS):
            keep = torch.zeros(HEADS, d, dtype=torch.bool, device=DEV)
            keep[h] = True
            qp, kvp = q.clone(), kv.clone()
            qp[:, :, ~keep.view(c)] = math.nan
            kvp[:, :, ~torch.cat([keep.view(c), keep.view(c)])] = math.nan
            qp[1 - s] = math.nan
            kvp[1 - s] = math.nan
            got = ops.cross_attention(qp, kvp, HEADS, scale)
            assert torch.equal(got[s, :, h * d:(h + 1) * d], clean[s, :, h * d:(h + 1) * d]), (s, h)


def test_refusals_stay_loud(ops):
    for d in (32, 48):
        q = torch.zeros(1, 16, 2 * d, dtype=torch.float16, device=DEV)
        kv = torch.zeros(1, 8, 4 * d, dtype=torch.float16, device=DEV)
        with pytest.raises(RuntimeError, match=f'head dim {d}'):
            ops.cross_attention(q, kv, 2, 0.1)
