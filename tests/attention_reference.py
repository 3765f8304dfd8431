"""Self-attention in float64, written from the definition; the per-element error bound of the 16-bit kernels, derived from the number
formats and the kernels' documented arithmetic; an emulation of that arithmetic in torch; and the seeded input classes the attention
tests run on.  Torch on the CPU only: nothing here imports diffusion_tts_amd or the oracle, so the kernels are measured against
something that shares no code with them (tests/test_attention_reference.py pins this file; tests/test_gpu_attention.py uses it).

Layout, as csrc/attention.hip: qkv [n, t, 3 * heads * d] = q | k | v blocks of heads * d channels, head-major inside a block;
out [n, t, heads * d]."""
import math
import types

import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}       # unit roundoff of the storage type (8 / 11 significant bits)
LOG2E = 1.4426950408889634
FLUSH_BELOW = 2.0 ** -13        # float16: a P below this (one binade above the smallest normal, 2^-14) may count as zero
KINDS = ('randn', 'sharp', 'flat', 'all_negative', 'rising', 'falling')


def heads_of(x, heads):
    """[n, t, heads * d] -> [n, heads, t, d]"""
    n, t, c = x.shape
    return x.reshape(n, t, heads, c // heads).permute(0, 2, 1, 3)


def tokens_of(x):
    """[n, heads, t, d] -> [n, t, heads * d]"""
    n, h, t, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(n, t, h * d)


def split_qkv(qkv, heads):
    c = qkv.shape[-1] // 3
    return (heads_of(qkv[..., i * c:(i + 1) * c], heads) for i in range(3))


def att_ref64(qkv, heads, scale):
    """softmax(q k^T * scale) v in float64 on the values qkv holds (already rounded to the storage type).  Returns a namespace:
    o [n, t, c]; A = sum_i w_i |v_i| [n, t, c] (>= |o|); w [n, h, t, t] the softmax weights; p [n, h, t, t] = exp(s - max s) (max p = 1,
    relative to the FINAL row maximum); vabs [n, h, t, d]; mb = the largest |row maximum| in base-2 units (|max s| * log2 e)."""
    q, k, v = split_qkv(qkv.double(), heads)
    s = torch.einsum('nhqd,nhkd->nhqk', q, k) * scale
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    w = p / p.sum(-1, keepdim=True)
    o = torch.einsum('nhqk,nhkd->nhqd', w, v)
    A = torch.einsum('nhqk,nhkd->nhqd', w, v.abs())
    return types.SimpleNamespace(o=tokens_of(o), A=tokens_of(A), w=w, p=p, vabs=v.abs(), mb=float(m.abs().max()) * LOG2E, t=qkv.shape[1])


def bound16(ref, dtype):
    """Per-element bound on |kernel - ref.o| for attention16_kernel; returns (bound, flush), both [n, t, c], flush being the float16
    allowance that `bound` already includes (zeros for bfloat16).

        bound = u |o| + 2 u A + (2^-15 + t 2^-23) A + [float16] flush          u = 2^-8 (bfloat16) / 2^-11 (float16)

    One output is o = sum_i p_i v_i / sum_i p_i over the t keys of its row, p_i = exp2(e_i), e_i = (s_i - m) sc2, s_i = q.k_i accumulated
    in f32 from exact 16-bit x 16-bit products, sc2 = scale * log2 e, m the maximum of the keys seen so far (key tiles of 64); when m
    rises, the accumulated numerator and denominator are multiplied by alpha = exp2((m_old - m_new) sc2).  With e32 = 2^-24:
      * p_i.  The exponent is ONE fused multiply-add, fma(s_i, sc2, -mb), mb = f32(m sc2).  Its inputs carry |mb| e32 (the rounding of
        mb) and 2 |e_i| e32 (sc2 as an f32, itself an f32 product), its result |e_i| e32, and exp2 is good to 1 ulp (2 e32).
        Relative error d_i of p_i: ln2 (|mb| + 3 |e_i| + |ds_i sc2| / e32) e32 + 2 e32, ds_i the error of the f32 score.  It moves o by
        sum_i w_i d_i (v_i - o), at most max|d_i| (A + |o|) <= 2 max|d_i| A: the term is 2^-15 A if max|d_i| <= 2^-16, i.e. if the
        bracket stays below 2^-16 / (ln2 e32) - 3 = 366.
        CONDITION on the inputs (asserted below): the exponent-sized numbers stay small -- |mb| <= 128 for every row (the issue that
        asked for this bound says "|exponent| <= 64"; the `sharp` class it also asks for has row maxima of 16 sigma-units * 4.7 * log2 e
        = 108, so the limit here is the next power of two and the budget below is done with it).  A key with |e_i| <= 32 then uses
        128 + 96 = 224 of the 366 and leaves 142 e32 for the score, whose magnitude is <= 160: the f32 score must be good to 0.9 e32
        of itself.  d products of random sign accumulated on the matrix core meet that in the typical case, not in the worst case;
        tests/test_attention_reference.py runs the emulation (f32 scores) on every input the kernels get to show the bound is met by
        this arithmetic.  A key with |e_i| > 32 has p_i < 2^-32, eight binades below what the f32 accumulators of a row whose largest
        p is 1 resolve: it contributes nothing to either side as long as A is not itself that small against |v| (asserted:
        A >= 2^-30 max|v|).
      * f32 accumulation of numerator and denominator over t keys, 32 at a time on the matrix core, and one multiplication by alpha per
        key tile: at most t e32 relative to A in each of the two: t 2^-23 A.
      * P is rounded to the storage type for the matrix core, p_i (1 + d_i), |d_i| <= u, and the SAME rounded P is summed for the
        denominator: u A (numerator) + u |o| (denominator) <= 2 u A.
      * one rounding of the result: u |o|.
      * float16 only, an ALLOWANCE rather than an established property (the cross-attention test has the same): a p_i below 2^-14 is a
        subnormal float16 and the matrix cores may flush it.  Should such a key count as zero the error is at most w_i (|v_i| + |o|),
        summed over those keys.  The threshold is taken one binade higher, p_i < 2^-13, so that exp2's ulp or the rounding of P cannot tip
        a value across the line unallowed.  The kernel rounds P relative to the RUNNING maximum, which is <= the final one: its P is
        >= the p_i used here, so it flushes a subset of the keys allowed here -- the allowance is conservative.  (bfloat16 has f32's
        exponent range: no such term.)"""
    u, t = U[dtype], ref.t
    assert ref.mb <= 128.0, f'input outside the bound\'s condition: |row maximum| * log2(e) = {ref.mb:.1f} > 128'
    assert bool((ref.A >= 2.0 ** -30 * float(ref.vabs.max())).all()), 'input outside the bound\'s condition: A vanishes against |v|'
    bound = u * ref.o.abs() + 2 * u * ref.A + (2.0 ** -15 + t * 2.0 ** -23) * ref.A
    flush = torch.zeros_like(bound)
    if dtype == torch.float16:
        wf = torch.where(ref.p < FLUSH_BELOW, ref.w, torch.zeros_like(ref.w))
        flush = tokens_of(torch.einsum('nhqk,nhkd->nhqd', wf, ref.vabs)) + tokens_of(wf.sum(-1, keepdim=True).expand(-1, -1, -1, ref.vabs.shape[-1])) * ref.o.abs()
    return bound + flush, flush


def emulate16(qkv, heads, scale, dtype, flush, mutation=None):
    """attention16_kernel's documented arithmetic in torch: f32 scores; key tiles of 64; online maximum; exp2(fma(s, sc2, -m sc2)); P
    rounded to `dtype`, float16 subnormals kept (flush=False) or zeroed (flush=True); numerator AND denominator accumulated in f32 from
    the rounded P, both rescaled by exp2((m_old - m_new) sc2); one final rounding.  Returns `dtype` [n, t, c].
    mutation (tests/test_attention_reference.py, "the net has teeth"): 'pad' = one zero key and value counted past the end of the last
    tile; ('skip', kt) = the rescale skipped on key tile kt; 'heads' = the value rows of heads 0 and 1 swapped."""
    n, t, c3 = qkv.shape
    q, k, v = (x.float().contiguous() for x in split_qkv(qkv, heads))
    if mutation == 'heads':
        v = torch.cat([v[:, 1:2], v[:, 0:1], v[:, 2:]], 1)
    sc2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    m = torch.full((n, heads, t), -math.inf)
    l = torch.zeros(n, heads, t)
    o = torch.zeros(n, heads, t, q.shape[-1])
    for kt, key0 in enumerate(range(0, t, 64)):
        kk, vv = k[:, :, key0:key0 + 64], v[:, :, key0:key0 + 64]
        if mutation == 'pad' and key0 + 64 > t:
            kk, vv = (torch.cat([x, torch.zeros_like(x[:, :, :1])], 2) for x in (kk, vv))
        s = q @ kk.transpose(-1, -2)
        m_new = torch.maximum(m, s.amax(-1))
        alpha = torch.exp2((m - m_new) * sc2)
        if mutation == ('skip', kt):
            alpha = torch.ones_like(alpha)
        mb = m_new * sc2
        e = torch.exp2((s.double() * sc2.double() - mb.double()[..., None]).float())       # the fused multiply-add: one rounding
        p = e.to(dtype)
        if flush and dtype == torch.float16:
            p = torch.where(p < 2.0 ** -14, torch.zeros_like(p), p)
        p = p.float()
        o = o * alpha[..., None] + p @ vv
        l = l * alpha + p.sum(-1)
        m = m_new
    return tokens_of(o * (1.0 / l)[..., None]).to(dtype)


def inputs(kind, n, t, heads, d, dtype):
    """Seeded qkv [n, t, 3 * heads * d] of one class, rounded to `dtype` (the softmax scale is 1 / sqrt(d) throughout):
      randn         unit normal: logits ~ N(0, 1).
      sharp         x 4: logits ~ N(0, 16^2), +-60 and beyond; a handful of keys per row carry all the weight and, in float16, most
                    probabilities lie below the normal range.
      flat          x 0.01: a uniform softmax over tiny operands.
      all_negative  q = b + 0.1 noise, k = -b + 0.1 noise, one direction b per (sample, head) with |b|^2 / sqrt(d) = 16: every valid
                    logit is -16 +- 0.5 and the softmax near uniform, so ONE zero-padded key counted by mistake (logit 0) would take
                    e^16 times the weight of a valid key -- all of the mass.
      rising        q = b + 0.1 noise, k = b * ramp(key) + 0.1 noise, ramp 0.2 -> 2 over the sequence, |b|^2 / sqrt(d) = 4: logits climb
                    from 0.8 to 8, the maximum rises in EVERY key tile (every tile rescales), and the range 7.2 < ln 2^13 keeps every
                    probability a normal float16.
      falling       ramp 2 -> 0.2: the maximum sits in the first tile and never moves again (alpha == 1 for whole waves)."""
    assert kind in KINDS
    c = heads * d
    gen = torch.Generator().manual_seed(1000003 * KINDS.index(kind) + 7919 * t + 31 * d + 7 * n + heads)
    noise = torch.randn(n, t, 3 * c, generator=gen, dtype=torch.float64)
    if kind in ('randn', 'sharp', 'flat'):
        x = noise * {'randn': 1.0, 'sharp': 4.0, 'flat': 0.01}[kind]
    else:
        b = torch.randn(n, 1, heads, d, generator=gen, dtype=torch.float64)
        b = b / b.norm(dim=-1, keepdim=True) * math.sqrt((16.0 if kind == 'all_negative' else 4.0) * math.sqrt(d))
        b = b.expand(n, t, heads, d).reshape(n, t, c)
        x = noise * 0.1
        x[..., 2 * c:] = noise[..., 2 * c:]                       # values: unit normal
        x[..., :c] += b
        if kind == 'all_negative':
            x[..., c:2 * c] -= b
        else:
            ramp = torch.linspace(0.2, 2.0, t, dtype=torch.float64) if t > 1 else torch.tensor([2.0], dtype=torch.float64)
            if kind == 'falling':
                ramp = ramp.flip(0)
            x[..., c:2 * c] += b * ramp[None, :, None]
    return x.to(dtype)


# the sequence lengths of tests/test_gpu_attention.py.  A block is 64 queries (one query tile per wave) or 128 (two), a key tile 64 keys.
ONE_T = (1, 15, 17, 64, 65, 129, 200)        # below / across one MFMA tile of 16, a full key tile, one key past it, three and four tiles
TWO_T = (65, 128, 145, 200, 257, 300)        # 145: a wave's second query tile lies wholly past the end; 257: a block holds one query
T512 = (1, 65, 200)


def shapes():
    """every (n, t, heads, d) the GPU tests launch: two samples and two heads, so that both offsets matter (head dim 512: one head)"""
    out = [(2, t, 2, 64) for t in sorted(set(ONE_T + TWO_T))]
    out += [(2, t, 2, d) for d in (128, 256) for t in ONE_T]
    return out + [(2, t, 1, 512) for t in T512]
