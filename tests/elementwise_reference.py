"""References, per-element bounds and input builders for the kernels of csrc/elementwise.hip: the code that turns a network output into the
next sampler state, an 8-bit image or a reward.  Torch / numpy on the CPU only; nothing here imports diffusion_tts_amd, so the kernels are
measured against something that shares no arithmetic with them.  tests/test_elementwise_reference.py pins this file (the bounds hold for a
model of the kernel's own arithmetic and exclude the plausible mistakes); tests/test_gpu_elementwise.py holds the kernels to it.

Every `*_ref` returns (reference, bound) as float64 CPU tensors of the output's shape, the bound per element, built from

    u   = unit roundoff of the storage type: 2^-8 bfloat16, 2^-11 float16, 0 for float32 storage (the store is exact)
    e32 = 2^-24, e64 = 2^-53  (unit roundoff of one float32 / float64 operation)

and the kernel's documented order of operations.  A multiply followed by an add may or may not be contracted to a fused multiply-add by
the compiler; a bound counts both roundings, so either form stays inside it (only the quantiser pins the two roundings, because there a
single ulp changes a byte).  Device-library functions: the ROCm device-library documentation is not shipped with the toolchain, so the
OpenCL 3.0 full-profile figures are used, as tests/test_gpu_sd_unet_ops.py does for erfc: expf 3 ulp, logf 3 ulp, sinf / cosf 4 ulp,
sqrtf 3 ulp, x / y 2.5 ulp (1 ulp = 2 e32 relative).  __expf(x) is v_exp_f32(x * f32(log2 e)): the product carries 1.5 e32 relative to an
exponent of |x| log2 e, i.e. 1.5 ln2 log2e |x| e32 < 2 |x| e32 relative to the result, and the instruction is documented to 1 ulp; taken
as EXPF_FAST(x) = 2^-22 + |x| 2^-23.

Reductions: a block of B threads sums L terms as ceil(L / B) serial additions per thread, a 6-level butterfly over the 64 lanes and (B = 256)
three more additions of the four wave partials; for terms of one sign, or measured against sum |terms|, the relative error is at most
(ceil(L / B) + 9) e.  One wave per row (B = 64): ceil(L / 64) + 6.
"""
import math
from fractions import Fraction

import numpy as np
import torch

E32, E64 = 2.0 ** -24, 2.0 ** -53
U = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
ULP = 2 * E32                                   # one float32 ulp, relative
EXP_ULPS, LOG_ULPS, SINCOS_ULPS, SQRT_ULPS, DIV_ULPS = 3, 3, 4, 3, 2.5
WRAP = 524288 + 257                             # one element past 2048 blocks of 256 and then some: the second trip of a grid-stride loop
WRAP_SHAPE = (1, 5, 49, 2141)                   # n, c, h, w with n*c*h*w == WRAP exactly (5 * 7 * 7 * 2141)
assert WRAP_SHAPE[1] * WRAP_SHAPE[2] * WRAP_SHAPE[3] == WRAP


def gen(seed):
    return torch.Generator().manual_seed(seed)


def expf_fast_rel(x):
    """relative error allowed to __expf(x) (see the module docstring)"""
    return 2.0 ** -22 + x.abs() * 2.0 ** -23


def silu64(x):
    return x / (1.0 + torch.exp(-x))


def silu_rel(x):
    """silu_f(x) = x / (1 + __expf(-x)): d silu / silu = -E dE / (1 + E) with E = exp(-x), so the exponential's relative error enters with a
    factor E / (1 + E) <= 1; the addition adds e32 and the division 2.5 ulp"""
    return expf_fast_rel(x) + (1 + 2 * DIV_ULPS) * E32


# ---- quantiser: exact ----------------------------------------------------------------------------------------------------------------
def quantize_two_step(x):
    """the reference's expression, two tensor operations (oracle/sampler.py::to_uint8, oracle/sd_loop.py::to_u8), in x's own type"""
    return (x * 127.5 + 128).clip(0, 255).to(torch.uint8)


def quantize_model(x, fused=False):
    """numpy model of the quantise kernels in x's type (float32: quantize_f32math_kernel; float64: quantize_kernel): the product rounded,
    then the sum rounded -- or, fused=True, the mistake: one rounding of the exact x * 127.5 + 128.  NaN-free input."""
    x = np.asarray(x)
    if not fused:
        v = x * x.dtype.type(127.5)
        v = v + x.dtype.type(128.0)
    elif x.dtype == np.float32:
        # exact in float64 for the magnitudes that matter (a 32-bit product below 256 plus 128 needs far fewer than 53 bits); where it is
        # not exact (|x| < 2^-20) both forms give 128 +- less than a level
        v = (x.astype(np.float64) * 127.5 + 128.0).astype(np.float32)
    else:
        v = np.array([float(Fraction(float(t)) * Fraction(255, 2) + 128) if np.isfinite(t) else float(t) * 127.5 for t in x.ravel()],
                     dtype=np.float64).reshape(x.shape)                      # Fraction -> float rounds once, correctly
    with np.errstate(invalid='ignore'):
        v = np.where(v < 0, 0, np.where(v > 255, 255, v))
    return v.astype(np.uint8)                                                 # truncation


def _neighbours(centre, reach, np_dtype):
    """the 2 * reach + 1 floats within +- reach ulp of `centre` (non-zero, far from the subnormals), by integer steps on the bit pattern"""
    it = np.int32 if np_dtype == np.float32 else np.int64
    c = np.array([centre], dtype=np_dtype)
    bits = c.view(it)[0]
    step = np.arange(-reach, reach + 1, dtype=it)
    return (bits + (step if centre > 0 else -step)).astype(it).view(np_dtype)       # sign-magnitude: a larger pattern is a larger magnitude


def quantize_witnesses(dtype):
    """Inputs on which a fused multiply-add and the two-step form truncate to different bytes: for each level k in 1 .. 255 (k = 128 is left
    out: its threshold is 0, where both forms are exact) the 65 floats within +- 32 ulp of (k - 128) / 127.5.  torch tensor of `dtype`."""
    nd = np.float32 if dtype == torch.float32 else np.float64
    cand = np.concatenate([_neighbours((k - 128) / 127.5, 32, nd) for k in range(1, 256) if k != 128])
    differ = quantize_model(cand, fused=True) != quantize_model(cand, fused=False)
    return torch.from_numpy(cand[differ].copy())


def quantize_edges(dtype):
    """every threshold (k - 128) / 127.5, k = 0 .. 256, with its +- 4 ulp neighbours; +-1, +-(1 + 2^-20), +-3, +-inf, +-0.0"""
    nd = np.float32 if dtype == torch.float32 else np.float64
    parts = [_neighbours((k - 128) / 127.5, 4, nd) for k in range(0, 257) if k != 128]
    extra = np.array([1.0, -1.0, 1 + 2.0 ** -20, -(1 + 2.0 ** -20), 3.0, -3.0, np.inf, -np.inf, 0.0, -0.0], dtype=nd)
    tiny = np.array([np.finfo(nd).tiny, -np.finfo(nd).tiny, np.finfo(nd).eps, -np.finfo(nd).eps], dtype=nd)      # k = 128's neighbourhood
    return torch.from_numpy(np.concatenate(parts + [extra, tiny]))


def quantize_random(dtype, count=WRAP, seed=90):
    """N(0, 0.6) values: about a tenth beyond [-1, 1] (clipped levels 0 and 255), and enough of them to wrap the grid-stride loop"""
    return (torch.randn(count, generator=gen(seed), dtype=torch.float64) * 0.6).to(dtype)


# ---- u8 -> [0, 1], brightness ------------------------------------------------------------------------------------------------------------
LUMA = (0.2126, 0.7152, 0.0722)


def u8_to_unit_ref(img):
    return img.float() / 255.0                   # IEEE float32 division, which the kernel's `(float)p / 255.0f` is too: equality


def brightness_ref(img):
    """img uint8 [n, 3, h, w].  The reference (oracle/scorers.py::BrightnessOracle) forms r = f32(p / 255) and the weighted channel sum in
    float32; the kernel does the same per pixel (three products, two sums: at most 5 roundings of positive terms, relative to lum), sums the
    pixels in FLOAT64 (hw terms, (ceil(hw / 256) + 9) e64) and rounds the mean once to float32: bound = (6 e32 + (hw / 256 + 10) e64) m.
    An all-zero image has bound 0: exactly 0.  The result is clamped to [0, 1] like the reference's."""
    n, c, h, w = img.shape
    r = (img.float() / 255.0).double()
    wts = torch.tensor(LUMA, dtype=torch.float32).double().view(1, 3, 1, 1)
    m = (r * wts).sum(1).mean((1, 2))
    bound = (6 * E32 + (h * w / 256 + 10) * E64) * m
    return m.clamp(0.0, 1.0), bound


def block_sum(terms, threads, dtype, drop_partial=None):
    """numpy model of the kernels' block reduction over the last axis: thread t adds terms t, t + threads, ... in order, a butterfly
    (lane ^ 32, 16, ... 1) sums each wave of 64, the wave partials are added left to right.  drop_partial: a wave partial left out (the mistake)."""
    terms = np.asarray(terms, dtype=dtype)
    L = terms.shape[-1]
    trips = -(-L // threads)
    pad = np.zeros(terms.shape[:-1] + (trips * threads - L,), dtype=dtype)             # adding +0 is exact
    t = np.concatenate([terms, pad], -1).reshape(terms.shape[:-1] + (trips, threads))
    acc = np.zeros(terms.shape[:-1] + (threads,), dtype=dtype)
    for i in range(trips):
        acc = acc + t[..., i, :]
    lane = np.arange(threads)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ o]
    parts = [acc[..., wv * 64] for wv in range(threads // 64) if wv != drop_partial]
    tot = parts[0]
    for p in parts[1:]:
        tot = tot + p
    return tot


def brightness_model(img, drop_partial=None, f32_accumulate=False):
    p = img.numpy().astype(np.float32)
    n, _, h, w = p.shape
    r, g_, b = (p[:, i].reshape(n, -1) / np.float32(255.0) for i in range(3))
    lum = r * np.float32(LUMA[0]) + g_ * np.float32(LUMA[1]) + b * np.float32(LUMA[2])
    acc = np.float32 if f32_accumulate else np.float64
    tot = block_sum(lum.astype(acc), 256, acc, drop_partial)
    m = (tot / acc(h * w)).astype(np.float32)
    return torch.from_numpy(np.minimum(np.maximum(m, np.float32(0)), np.float32(1)))


def brightness_images(hw, n, seed=91):
    """uint8 [n, 3, h, w] with h * w == hw: image 0 is the 0 .. 255 ramp repeated, the others random"""
    h = next(d for d in range(int(math.isqrt(hw)), 0, -1) if hw % d == 0)
    img = torch.randint(0, 256, (n, 3, h, hw // h), generator=gen(seed + hw), dtype=torch.uint8)
    img[0] = (torch.arange(3 * hw) % 256).to(torch.uint8).view(3, h, hw // h)
    return img


# ---- softmax_gather ------------------------------------------------------------------------------------------------------------------------
SOFTMAX_FLOOR = 2.0 ** -125


def softmax_gather_ref(logits, target):
    """p = expf(x_t - mx) / sum_j expf(x_j - mx), float32, mx the row maximum (exact).  d_j = x_j - mx carries e32 |d_j|, which the exponential
    turns into a relative e32 |d_j|; expf adds 3 ulp: each exponential is good to (6 + |d_j|) e32.  The denominator's error is the weighted
    mean of that, sum_j w_j (6 + |d_j|) e32, plus the block reduction's (ceil(k / 256) + 9) e32; the division adds 2.5 ulp.
    An exponential below 2^-126 may be flushed to zero, and so may the result: an absolute floor of 2^-125 (the denominator is >= 1)."""
    x = logits.double()
    n, k = x.shape
    d = x - x.amax(1, keepdim=True)
    e = torch.exp(d)
    s = e.sum(1)
    wts = e / s[:, None]
    idx = torch.arange(n)
    dt = d[idx, target.long()]
    dabs = torch.where(torch.isinf(d), torch.zeros_like(d), d.abs())                 # exp(-inf) = 0 exactly: no term
    rel = E32 * ((6 + dt.abs()) + (wts * (6 + dabs)).sum(1) + (-(-k // 256) + 9) + 2 * DIV_ULPS)
    p = e[idx, target.long()] / s
    return p, rel * p + SOFTMAX_FLOOR


def softmax_gather_model(logits, target, subtract_max=True):
    x = logits.numpy()
    n, k = x.shape
    mx = x.max(1, keepdims=True) if subtract_max else np.zeros((n, 1), dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.exp((x - mx).astype(np.float32)).astype(np.float32)
        s = block_sum(e, 256, np.float32)
        t = e[np.arange(n), target.numpy()]
        return torch.from_numpy((t / s).astype(np.float32))


def softmax_cases(k, seed=92):
    """(logits float32 [rows, k], target int32 [rows]): targets first / last / at the maximum, rows shifted by +-1e4, a row whose other logits
    are all -inf, a row whose target probability is below 1e-30 (k > 1).  Targets always inside the row."""
    g_ = gen(seed + k)
    rows = 8
    x = torch.randn(rows, k, generator=g_) * 3
    x[3] += 1e4
    x[4] -= 1e4
    tgt = torch.tensor([0, k - 1, 0, k // 2, k // 3, 0, k - 1, min(5, k - 1)], dtype=torch.int32)
    tgt[2] = int(x[2].argmax())
    x[5] = -math.inf
    x[5, 0] = 1.5
    if k > 1:
        x[6, k - 1] = -40.0                                            # against a maximum of +40: exp(-80) = 1.8e-35, a normal float32
        x[6, 0] = 40.0
    return x, tgt


# ---- cosine_rows -----------------------------------------------------------------------------------------------------------------------------
def cosine_rows_ref(a, b):
    """out = sum_i (a_i / na) (b_i / nb), na = sqrtf(sum a_i^2) (one wave per row, all float32).  A sum of squares of d terms is good to
    g = (ceil(d / 64) + 7) e32 (one product rounding + the reduction), its root to g / 2 + 3 ulp: dn.  Each term carries both norms' errors,
    two divisions (2.5 ulp each) and the product's rounding, the sum the reduction's (ceil(d / 64) + 6) e32:
        bound = (2 dn + 4 * 2.5 e32 + e32 + (ceil(d / 64) + 6) e32) * sum |a_i b_i| / (|a| |b|)."""
    a64, b64 = a.double(), b.double()
    n, d = a64.shape
    b64 = b64.expand(n, d)
    na, nb = a64.pow(2).sum(1).sqrt(), b64.pow(2).sum(1).sqrt()
    ref = (a64 * b64).sum(1) / (na * nb)
    trips = -(-d // 64)
    dn = (trips + 7) * E32 / 2 + SQRT_ULPS * ULP
    rel = 2 * dn + 2 * DIV_ULPS * ULP + E32 + (trips + 6) * E32
    return ref, rel * (a64 * b64).abs().sum(1) / (na * nb)


def cosine_rows_model(a, b):
    x, y = a.numpy(), np.broadcast_to(b.numpy(), a.shape)
    na = np.sqrt(block_sum(x * x, 64, np.float32))[:, None]
    nb = np.sqrt(block_sum(y * y, 64, np.float32))[:, None]
    return torch.from_numpy(block_sum((x / na) * (y / nb), 64, np.float32))


def cosine_cases(d, b_rows_one, seed=93):
    """a [8, d], b [8, d] or [1, d]: random rows; rows 1 / 2 / 3 of `a` parallel, antiparallel and orthogonal to their b row; row 4 scaled by
    1e-3, row 5 by 1e3 (and the b rows by the opposite factor when b has a row per a row)"""
    g_ = gen(seed + d + 1000 * b_rows_one)
    a = torch.randn(8, d, generator=g_)
    b = torch.randn(1 if b_rows_one else 8, d, generator=g_)
    bb = b.expand(8, d)
    a[1] = 0.7 * bb[1]
    a[2] = -1.9 * bb[2]
    if d > 1:                                                           # remove the component along b: orthogonal up to rounding
        a[3] = a[3] - (a[3].double() @ bb[3].double() / (bb[3].double() @ bb[3].double())).float() * bb[3]
    a[4] *= 1e-3
    a[5] *= 1e3
    if not b_rows_one:
        b[4] *= 1e3
        b[5] *= 1e-3
    return a, b


# ---- linear ----------------------------------------------------------------------------------------------------------------------------------
def linear_takes_vector_kernel(x, w, k):
    """the documented dispatch condition of dts_linear: 16-byte loads iff k % 4 == 0, ldx % 4 == 0 and both base addresses 16-byte aligned"""
    return k % 4 == 0 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0


def linear_ref(x, w, bias=None, prior=None, act_in=False, act_out=False):
    """y = [silu](sum_i [silu](x_i) w_i + bias [+ prior]) in float32, one wave per output: a lane takes every 64th term (the 16-byte form four
    consecutive terms of every 256: at most ceil(k / 64) + 4 per lane), then the 6-level butterfly.  With S = sum |x_i w_i|:
        products and accumulation: (ceil(k / 64) + 4 + 6 + 1) e32 S;  + bias and + prior: one rounding of the running value each, 2 e32 (S + |bias| + |prior|);
        act_in: each silu(x_i) relatively silu_rel(x_i): sum_i silu_rel(x_i) |silu(x_i) w_i|;
        act_out: |silu'| <= 1.1 carries the error of v, and silu(v) adds silu_rel(v) |silu(v)| (taken at |v| + its bound)."""
    x64, w64 = x.double(), w.double()
    m, k = x64.shape
    xs = silu64(x64) if act_in else x64
    S = xs.abs() @ w64.abs().T
    b64 = torch.zeros(w.shape[0], dtype=torch.float64) if bias is None else bias.double()
    p64 = torch.zeros(m, w.shape[0], dtype=torch.float64) if prior is None else prior.double()
    v = xs @ w64.T + b64 + p64
    bound = (-(-k // 64) + 11) * E32 * S + 2 * E32 * (S + b64.abs() + p64.abs())
    if act_in:
        bound = bound + (silu_rel(x64) * xs.abs()) @ w64.abs().T
    if act_out:
        ref = silu64(v)
        bound = 1.1 * bound + silu_rel(v.abs() + bound) * ref.abs()
        v = ref
    return v, bound


def _silu_model(x):
    with np.errstate(over='ignore'):
        return (x / (np.float32(1) + np.exp(-x).astype(np.float32))).astype(np.float32)


def linear_model(x, w, bias=None, prior=None, act_in=False, act_out=False, vector=False, drop_ragged_trip=False):
    """numpy float32 model of linear_kernel (vector=False) / linear4_kernel; drop_ragged_trip: the mistake of a k loop that stops at the last
    whole trip (64 terms, 256 for the vector form)"""
    xn, wn = x.numpy().astype(np.float32), w.numpy().astype(np.float32)
    m, k = xn.shape
    if act_in:
        xn = _silu_model(xn)
    per = 256 if vector else 64
    kk = (k // per) * per if drop_ragged_trip else k
    prod = (xn[:, None, :kk] * wn[None, :, :kk]).astype(np.float32)                # [m, n, k]
    if vector:                                                                    # lane l adds terms 4l .. 4l + 3 of every 256
        trips = -(-kk // 256)
        pad = np.zeros(prod.shape[:-1] + (trips * 256 - kk,), dtype=np.float32)
        t = np.concatenate([prod, pad], -1).reshape(prod.shape[:-1] + (trips, 64, 4))
        acc = np.zeros(prod.shape[:-1] + (64,), dtype=np.float32)
        for i in range(trips):
            for j in range(4):
                acc = acc + t[..., i, :, j]
        v = block_sum(acc, 64, np.float32)
    else:
        v = block_sum(prod, 64, np.float32) if kk else np.zeros(prod.shape[:-1], dtype=np.float32)
    v = v + (np.float32(0) if bias is None else bias.numpy()[None, :])
    if prior is not None:
        v = v + prior.numpy()
    if act_out:
        v = _silu_model(v.astype(np.float32))
    return torch.from_numpy(np.asarray(v, dtype=np.float32))


def linear_inputs(m, n, k, act, seed=94):
    """x [m, k], w [n, k], bias [n], prior [m, n]; with an activation the arguments of SiLU reach +-20 (x itself for act_in; the first two
    outputs through a large bias for act_out)"""
    g_ = gen(seed + 7 * m + 131 * n + 1009 * k)
    x = torch.randn(m, k, generator=g_) * (4.0 if act else 1.0)
    w = torch.randn(n, k, generator=g_) / math.sqrt(k)
    bias = torch.randn(n, generator=g_)
    prior = torch.randn(m, n, generator=g_)
    if act:
        x.view(-1)[0] = 20.0
        x.view(-1)[-1] = -20.0
        bias[0] = 20.0
        bias[-1] = -20.0
    return x, w, bias, prior


# ---- pos_embedding ---------------------------------------------------------------------------------------------------------------------------
POS_BOUND = SINCOS_ULPS * ULP                    # 4 ulp of a result of magnitude <= 1, absolute


def pos_embedding_ref(v, freqs, swap):
    """[cos(a) | sin(a)] (swap: [sin | cos]) of a = the FLOAT32 product v_n f_j, which the reference forms too (torch.outer in float32): the
    argument is shared exactly, so only sinf / cosf's 4 ulp remain -- absolute 4 * 2^-23, whatever the argument's size."""
    a = (v[:, None] * freqs[None, :]).double()                        # float32 product, one rounding, then widened
    c, s = torch.cos(a), torch.sin(a)
    ref = torch.cat([s, c] if swap else [c, s], 1)
    return ref, torch.full_like(ref, POS_BOUND)


def pos_embedding_model(v, freqs, swap, f64_product=False):
    a = v.numpy().astype(np.float64)[:, None] * freqs.numpy().astype(np.float64)[None, :] if f64_product else \
        (v.numpy()[:, None] * freqs.numpy()[None, :]).astype(np.float32)
    c, s = np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)
    return torch.from_numpy(np.concatenate([s, c] if swap else [c, s], 1))


POS_VALUES = (0.0, -0.0, 1e-4, -1.3, 1.09, 80.0, 999.0)


def pos_freqs(half):
    return (1 / 10000) ** (torch.arange(half, dtype=torch.float32) / half)


# ---- EDM preconditioning -------------------------------------------------------------------------------------------------------------------
def precond_in_ref(x, sigma, sigma_data):
    """From sg = f32(sigma) and sd = f32(sigma_data), in float64: c_skip = sd^2 / (sg^2 + sd^2), c_out = sg sd / sqrt(sg^2 + sd^2), c_in =
    1 / sqrt(sg^2 + sd^2), c_noise = log(sg) / 4, xin = c_in x.  The kernel's float32 steps: two squares and their sum (3 e32), sqrtf (half of
    that + 3 ulp), a product, a division (2.5 ulp): every one of c_skip, c_out, c_in within 16 e32 relative; c_noise is logf's 3 ulp (the
    division by 4 is exact); xin adds the rounding of x to float32 and one product: 18 e32 |xin|.
    Returns (xin, bound), (coef [n, 4], bound)."""
    n = x.shape[0]
    sg = sigma.float().double().expand(n) if sigma.numel() == 1 else sigma.float().double()
    sd = float(np.float32(sigma_data))
    q = sg * sg + sd * sd
    coef = torch.stack([sd * sd / q, sg * sd / q.sqrt(), 1.0 / q.sqrt(), sg.log() / 4.0], 1)
    cb = torch.cat([16 * E32 * coef[:, :3].abs(), LOG_ULPS * ULP * coef[:, 3:].abs()], 1)
    xin = coef[:, 2].view(n, *([1] * (x.dim() - 1))) * x.double()
    return (xin, 18 * E32 * xin.abs()), (coef, cb)


def precond_in_model(x, sigma, sigma_data):
    n = x.shape[0]
    sg = np.broadcast_to(sigma.numpy().astype(np.float32), (n,))
    sd = np.float32(sigma_data)
    s2, d2 = sg * sg, sd * sd
    c_in = np.float32(1) / np.sqrt(d2 + s2)
    coef = np.stack([d2 / (s2 + d2), sg * sd / np.sqrt(s2 + d2), c_in, np.log(sg) / np.float32(4)], 1).astype(np.float32)
    xin = c_in.reshape(n, *([1] * (x.dim() - 1))) * x.numpy().astype(np.float32)
    return torch.from_numpy(xin.astype(np.float32)), torch.from_numpy(coef)


def precond_out_ref(x, F, coef):
    """D = c_skip f32(x) + c_out F from the float32 coefficients it is GIVEN (exact inputs here): four roundings (x, two products, the sum),
    each at most e32 of |c_skip x| + |c_out F|: 4 e32 (|c_skip x| + |c_out F|)."""
    n = x.shape[0]
    sh = (n,) + (1,) * (x.dim() - 1)
    t0, t1 = coef[:, 0].double().view(sh) * x.double(), coef[:, 1].double().view(sh) * F.double()
    return t0 + t1, 4 * E32 * (t0.abs() + t1.abs())


def precond_out_model(x, F, coef):
    sh = (x.shape[0],) + (1,) * (x.dim() - 1)
    c = coef.numpy()
    return torch.from_numpy((c[:, 0].reshape(sh) * x.numpy().astype(np.float32) + c[:, 1].reshape(sh) * F.numpy()).astype(np.float32))


# ---- Heun / Euler step, float64 --------------------------------------------------------------------------------------------------------------
HEUN_K = 8        # "a few": the kernel's <= 4 roundings per result and the float64 reference's own, each relative to the terms it combines


def row_map(nb, xb, interleave, wrong=False):
    """source row of x_cur for each of nb rows: Tensor.repeat order (row % xb) or repeat_interleave order (row // (nb / xb)); wrong=True swaps
    the two rules (the mistake)"""
    rows = torch.arange(nb)
    return rows // (nb // xb) if (interleave != wrong) else rows % xb


def heun_xhat_ref(x_cur, eps, coef, nb, interleave, wrong_map=False):
    """x_hat = x_cur[src] + coef eps, two float64 steps: bound 8 e64 (|x| + |coef eps|)"""
    src = row_map(nb, x_cur.shape[0], interleave, wrong_map)
    t = coef * eps.double()
    xs = x_cur[src]
    return xs + t, HEUN_K * E64 * (xs.abs() + t.abs())


def heun_euler_ref(x_hat, D, t_hat, t_next):
    """d = (x_hat - D) / t_hat; x_next = x_hat + (t_next - t_hat) d.  bounds: 8 e64 (|x_hat| + |D|) / t_hat and 8 e64 (|x_hat| + |dt| (|x_hat| + |D|) / t_hat)"""
    dt = t_next - t_hat
    mag = (x_hat.abs() + D.double().abs()) / abs(t_hat)
    d = (x_hat - D.double()) / t_hat
    return (d, HEUN_K * E64 * mag), (x_hat + dt * d, HEUN_K * E64 * (x_hat.abs() + abs(dt) * mag))


def heun_correct_ref(x_hat, D2, d_cur, t_hat, t_next, x_next):
    """d' = (x_next - D2) / t_next; out = x_hat + dt (0.5 d + 0.5 d'): 8 e64 (|x_hat| + |dt| (0.5 |d| + 0.5 (|x_next| + |D2|) / t_next))"""
    dt = t_next - t_hat
    dp = (x_next - D2.double()) / t_next
    mag = 0.5 * d_cur.abs() + 0.5 * (x_next.abs() + D2.double().abs()) / abs(t_next)
    return x_hat + dt * (0.5 * d_cur + 0.5 * dp), HEUN_K * E64 * (x_hat.abs() + abs(dt) * mag)


def sigma_schedule(num_steps=18, sigma_min=0.002, sigma_max=80.0, rho=7.0):
    """the EDM schedule (float64), t_N = 0 appended"""
    i = torch.arange(num_steps, dtype=torch.float64)
    t = (sigma_max ** (1 / rho) + i / (num_steps - 1) * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho
    return torch.cat([t, torch.zeros(1, dtype=torch.float64)])


# ---- candidate_noise (float64) -------------------------------------------------------------------------------------------------------------
def candidate_noise_ref(pivot, g_, mode, scale):
    """Row r = cn * b + sample: mode[cn] == 0 -> g_[r] (a copy, bit for bit); else pivot[sample] + scale[cn] * g_[r] / |g_[r]|_2.  The sum of
    squares of chw terms (256 threads, float64) is good to (ceil(chw / 256) + 10) e64, the root to half of that + e64, then a division, a product
    and a sum: bound = 2 e64 |pivot| + (ceil(chw / 256) + 16) e64 |scale g / norm| (the reference's own pairwise float64 sum included)."""
    b = pivot.shape[0]
    nb = g_.shape[0]
    chw = pivot[0].numel()
    cn = torch.arange(nb) // b
    sample = torch.arange(nb) % b
    sh = (nb,) + (1,) * (g_.dim() - 1)
    nrm = g_.reshape(nb, -1).pow(2).sum(1).sqrt().view(sh)
    t = scale.double()[cn].view(sh) * (g_ / nrm)
    ref = pivot[sample] + t
    bound = 2 * E64 * pivot[sample].abs() + (-(-chw // 256) + 16) * E64 * t.abs()
    keep = (mode[cn] == 0).view(sh)
    return torch.where(keep, g_, ref), torch.where(keep, torch.zeros_like(ref), bound)


def candidate_noise_model(pivot, g_, mode, scale, drop_partial=None):
    b, nb = pivot.shape[0], g_.shape[0]
    gn = g_.numpy().reshape(nb, -1)
    nrm = np.sqrt(block_sum(gn * gn, 256, np.float64, drop_partial))[:, None]
    cn, sample = np.arange(nb) // b, np.arange(nb) % b
    out = pivot.numpy().reshape(b, -1)[sample] + scale.numpy().astype(np.float64)[cn][:, None] * (gn / nrm)
    out = np.where((mode.numpy()[cn] == 0)[:, None], gn, out)
    return torch.from_numpy(out.reshape(g_.shape))


# ---- DDIM candidates, classifier-free guidance ---------------------------------------------------------------------------------------------
def _f32(v):
    return float(np.float32(v))


def ddim_ref(x, e, z, alpha_t, alpha_prev, sigma_t):
    """From the storage-rounded x, e, z and the float32-rounded scalars, in float64:
        x0 = (x - sb e) / sa,  prev_c = sp x0 + dirc e + sigma_t z_c;  sa = sqrt(a_t), sb = sqrt(1 - a_t), sp = sqrt(a_prev), dirc = sqrt(1 - a_prev - sigma_t^2).
    The kernel computes the four coefficients with sqrtf (3 ulp) of a float32 argument: sa, sb, sp within dc = 8 e32; dirc's argument
    1 - a_prev - sigma_t^2 cancels, 3 e32 (1 + a_prev + sigma_t^2) absolute, so ddirc = 1.5 e32 (1 + a_prev + sigma_t^2) / dirc^2 + 6 e32.  Then
        num = x - sb e:         (dc + e32) |sb e| + e32 |num|
        x0  = num / sa:         that / sa  (the 1 / sqrt(a_t) amplification)  + (dc + 5 e32) |x0|;          stored: + u |x0|
        base = sp x0 + dirc e:  sp * (error of x0) + (dc + e32) |sp x0| + (ddirc + e32) |dirc e| + e32 |base|
        prev = base + sigma z:  + e32 |sigma z| + e32 |prev|;                                                  stored: + u |prev|
    (base is formed from the unrounded float32 x0).  Returns (prev [ncand, ...], bound), (x0, bound) -- bounds without the u term, which the
    caller adds for its storage type (rounded_bound)."""
    at, ap, st = _f32(alpha_t), _f32(alpha_prev), _f32(sigma_t)
    sa, sb, sp = math.sqrt(at), math.sqrt(1 - at), math.sqrt(ap)
    d2 = 1 - ap - st * st
    dirc = math.sqrt(d2)
    dc = 8 * E32
    assert d2 > 0.0, 'the cases keep dirc away from an exact zero'
    ddirc = 1.5 * E32 * (1 + ap + st * st) / d2 + 6 * E32
    x64, e64 = x.double(), e.double()
    num = x64 - sb * e64
    x0 = num / sa
    bx0 = ((dc + E32) * (sb * e64).abs() + E32 * num.abs()) / sa + (dc + 5 * E32) * x0.abs()
    base = sp * x0 + dirc * e64
    bbase = sp * bx0 + (dc + E32) * (sp * x0).abs() + (ddirc + E32) * (dirc * e64).abs() + E32 * base.abs()
    if z is None:
        prev = base[None]
        bprev = bbase[None] + E32 * prev.abs()
    else:
        t = st * z.double()
        prev = base[None] + t
        bprev = bbase[None] + E32 * t.abs() + E32 * prev.abs()
    return (prev, bprev), (x0, bx0)


def rounded_bound(ref, bound, dtype):
    """+ the storage rounding of the float32 result v, |v - ref| <= bound: u |v| <= u (|ref| + bound) (and, float16, half the spacing 2^-24
    of its subnormals)"""
    return bound + U[dtype] * (ref.abs() + bound) + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def ddim_model(x, e, z, alpha_t, alpha_prev, sigma_t, dtype):
    f = np.float32
    at, ap, st = f(alpha_t), f(alpha_prev), f(sigma_t)
    sa, sb, sp, dirc = np.sqrt(at), np.sqrt(f(1) - at), np.sqrt(ap), np.sqrt(f(1) - ap - st * st)
    xv, ev = x.float().numpy(), e.float().numpy()
    x0 = (xv - sb * ev) / sa
    base = sp * x0 + dirc * ev
    zz = np.zeros((1,) + xv.shape, dtype=f) if z is None else z.float().numpy()
    prev = base[None] + st * zz
    return torch.from_numpy(prev.astype(f)).to(dtype), torch.from_numpy(x0.astype(f)).to(dtype)


def ddim_sigma(alpha_t, alpha_prev, eta):
    return eta * math.sqrt((1 - alpha_prev) / (1 - alpha_t) * (1 - alpha_t / alpha_prev))


def cfg_ref(uncond, cond, guidance):
    """out = u + g (c - u) in float32 from the stored values: three roundings, 3 e32 (|u| + |g (c - u)|); the caller adds the storage rounding.
    At g = 0 the bound is 3 e32 |u|, but the kernel owes more there: out == u bit for bit (the test asserts it separately)."""
    g_ = _f32(guidance)
    u64, c64 = uncond.double(), cond.double()
    t = g_ * (c64 - u64)
    return u64 + t, 3 * E32 * (u64.abs() + t.abs())


def cfg_model(uncond, cond, guidance, dtype):
    uv, cv = uncond.float().numpy(), cond.float().numpy()
    return torch.from_numpy((uv + np.float32(guidance) * (cv - uv)).astype(np.float32)).to(dtype)


# ---- attention-pool tokens -------------------------------------------------------------------------------------------------------------------
def attnpool_tokens_ref(x, pos, cls_shift=0):
    """x [n, hw, c] (storage type), pos float32 [c, hw + 1] -> tokens [n, hw + 1, c]: token 0 = mean_p x[p] + pos[:, 0], token 1 + p = x[p] +
    pos[:, 1 + p], in float32.  The mean is a SERIAL float32 sum of hw values ((hw - 1) e32 sum |x|), one division (2.5 ulp), one sum:
        token 0: ((hw - 1) + 5) e32 * sum |x| / hw + e32 |tok|;  others: e32 |tok|;  the caller adds the storage rounding.
    cls_shift = 1: the mistake of reading pos one token off (pos[:, t + 1 mod (hw + 1)])."""
    x64 = x.double()
    n, hw, c = x64.shape
    p64 = pos.double().T                                                   # [hw + 1, c]
    if cls_shift:
        p64 = torch.roll(p64, -cls_shift, 0)
    mean = x64.sum(1, keepdim=True) / hw
    ref = torch.cat([mean, x64], 1) + p64[None]
    bound = E32 * ref.abs()
    bound[:, 0] += (hw + 4) * E32 * x64.abs().sum(1) / hw
    return ref, bound


def attnpool_tokens_model(x, pos, dtype):
    xv = x.float().numpy()
    n, hw, c = xv.shape
    s = np.zeros((n, c), dtype=np.float32)
    for p in range(hw):
        s = s + xv[:, p]
    pv = pos.numpy().T
    tok = np.concatenate([(s / np.float32(hw))[:, None] + pv[None, :1], xv + pv[None, 1:]], 1)
    return torch.from_numpy(tok.astype(np.float32)).to(dtype)


# ---- layout: plain index arithmetic ------------------------------------------------------------------------------------------------------------
def nchw_to_nhwc_ref(x, dtype, cpad=None):
    y = x.permute(0, 2, 3, 1).to(dtype)
    if cpad is not None:
        y = torch.cat([y, torch.zeros(y.shape[:3] + (cpad - y.shape[3],), dtype=dtype)], 3)
    return y.contiguous()


def pack_conv_weight_ref(w, dtype, perm=None):
    """OIHW float32 -> [O][kh][kw][I] in dtype, output row o taken from source row perm[o]"""
    src = w if perm is None else w[perm.long()]
    return src.permute(0, 2, 3, 1).to(dtype).contiguous()


def worst(got, ref, bound):
    """(max err / bound, max err): the one comparison of the bounded tests.  A zero bound asks for equality (0 / 0 counts as 0)."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-320))
    return float(ratio.max()), float(err.max())


# ---- the cases both test files run (the CPU file on the models, the GPU file on the kernels) ---------------------------------------------------
SIGMAS = (0.002, 0.3, 1.0, 80.0)


def precond_cases():
    """(x float64 [n, chw], sigma float64 [1] or [n], F float32 [n, chw]); x is scaled by 80 (the largest noise level's states)"""
    for n in (1, 3):
        for chw in (1, 192, 257):
            for nsigma in sorted({1, n}):
                for first in range(len(SIGMAS) if nsigma == 1 else 2):
                    g_ = gen(95 + 10 * n + chw + first)
                    sig = torch.tensor([SIGMAS[(first + j) % 4] for j in range(nsigma)], dtype=torch.float64)
                    if nsigma == n and n > 1 and first == 1:
                        sig = sig.flip(0)
                    yield (torch.randn(n, chw, generator=g_, dtype=torch.float64) * 80, sig, torch.randn(n, chw, generator=g_))


def heun_cases():
    """(x_cur float64 [xb, chw], eps [nb, chw] float64 or float32, nb, interleave, step index of the 18-step schedule).  Row r of x_cur is
    within 0.25 of the constant 10 (r + 1), so a wrong source row is off by about 10."""
    k = 0
    for xb, nb in ((1, 1), (1, 3), (3, 3), (1, 6), (2, 6), (6, 6), (3, 18)):
        for interleave in (False, True):
            for chw in (1, 192, 3 * 32 * 32):
                k += 1
                g_ = gen(96 + k)
                x = 10.0 * torch.arange(1, xb + 1, dtype=torch.float64)[:, None] + 0.25 * torch.rand(xb, chw, generator=g_, dtype=torch.float64)
                eps = torch.randn(nb, chw, generator=g_, dtype=torch.float64)
                yield (x, eps.float() if k % 2 else eps, nb, interleave, (0, 8, 17)[k % 3])


def churned(t_cur, num_steps=18, s_churn=40.0, s_min=0.05, s_max=50.0, s_noise=1.003):
    """(t_hat, noise coefficient) of the EDM sampler's churn at noise level t_cur"""
    gamma = min(s_churn / num_steps, math.sqrt(2) - 1) if s_min <= t_cur <= s_max else 0.0
    t_hat = t_cur + gamma * t_cur
    return t_hat, math.sqrt(max(t_hat ** 2 - t_cur ** 2, 0.0)) * s_noise


def candidate_cases():
    """(pivot float64 [b, chw], g float64 [N * b, chw], mode int32 [N], scale float32 [N])"""
    for chw in (1, 192, 257, 3 * 32 * 32):
        for b in (1, 2):
            for modes, sc in (([0, 0, 0], [0.3, 0.5, 0.7]), ([1, 1, 1], [0.1, 0.731, 12.0]), ([1, 0, 1, 1], [0.25, 9.0, 0.0, 2.5])):
                g_ = gen(97 + chw + b + len(modes) + sum(modes))
                yield (torch.randn(b, chw, generator=g_, dtype=torch.float64), torch.randn(len(modes) * b, chw, generator=g_, dtype=torch.float64),
                       torch.tensor(modes, dtype=torch.int32), torch.tensor(sc, dtype=torch.float32))


ALPHAS = ((0.9991, 0.9995), (0.3, 0.45), (0.0047, 0.0100))
STORAGE = (torch.float32, torch.float16, torch.bfloat16)


def ddim_cases(dtype):
    """(x, e [count] in dtype, z [ncand, count] or None, alpha_t, alpha_prev, sigma_t, want_x0)"""
    k = 0
    for at, ap in ALPHAS:
        for count in (1, 255, 4 * 64 * 64):
            for eta, ncand in ((0.0, 1), (1.0, 1), (1.0, 3)):
                k += 1
                g_ = gen(98 + k)
                x, e = torch.randn(count, generator=g_).to(dtype), torch.randn(count, generator=g_).to(dtype)
                z = None if eta == 0.0 else torch.randn(ncand, count, generator=g_).to(dtype)
                yield (x, e, z, at, ap, ddim_sigma(at, ap, eta), k % 4 != 0)


GUIDANCE = (0.0, 1.0, 7.5)


def cfg_cases(dtype):
    for count in (1, 255, 4 * 64 * 64):
        g_ = gen(99 + count)
        yield torch.randn(count, generator=g_).to(dtype), torch.randn(count, generator=g_).to(dtype)


def attnpool_cases(dtype):
    """(x [n, hw, c] in dtype, pos float32 [c, hw + 1])"""
    for hw in (1, 16, 64):
        for c in (8, 64, 320, 2048):
            n = 1 + (hw + c) % 2 if c != 320 else 2
            g_ = gen(100 + hw + c)
            yield (torch.randn(n, hw, c, generator=g_) + 0.5).to(dtype), torch.randn(c, hw + 1, generator=g_)
