"""References, per-element bounds, kernel models and input builders for dts_precond_in (csrc/elementwise.hip): the VP, VE and iDDPM
preconditioners of edm/training/networks.py:495-625.  numpy / Fraction on the CPU only; nothing here imports diffusion_tts_amd, so the kernel
is measured against something that shares no arithmetic with it.  tests/test_precond_reference.py pins this file (the bounds hold for a
float32 model of the kernel's own steps and exclude the planted mistakes); tests/test_gpu_precond.py holds the kernel to it.

coef_ref returns (reference, bound), float64 [n, 4] = (c_skip, c_out, c_in, c_noise) per row, from s = f32(sigma) -- the value both the
reference module and the kernel start from -- and the Python-scalar sub-expressions rounded to float32 once (`scalars`), as torch rounds a
Python scalar that meets a float32 tensor.  With e32 = 2^-24 per float32 operation, 1 ulp = 2 e32 relative, and the OpenCL full-profile
figures tests/elementwise_reference.py uses for the device library (logf 3 ulp, sqrtf 3 ulp, x / y 2.5 ulp):

  c_skip = 1, c_out = -s (VE: s), VE's c_in = 1: exact, bound 0.
  c_in = 1 / sqrt(s^2 + 1):  s^2 carries e32, relative to the sum at most e32 again, the sum its own e32; the root halves those 2 e32 and adds
         3 ulp; the division adds 2.5 ulp:  (1 + 6 + 5) e32 = 12 e32 relative.
  (The kernel takes its two logarithms in double and rounds once, i.e. to half an ulp; the bounds keep a float32 library logf's 3 ulp, which
  is also what the reference module's own host evaluation is entitled to: test_precond_reference.py holds its recorded c_noise to them.)
  VE c_noise = log(0.5 s): the product is exact (a power of two), so only logf's 3 ulp of the result.
  VP c_noise = (M-1) * ((sqrt(beta_min^2 + 2 beta_d * log(a)) - beta_min) / beta_d) with a = f32(1 + f32(s^2)): `a` is computed here in
         float32 exactly as on either side (two IEEE operations), and the reference is the float64 value of the rest FROM THAT a.  Absolute
         errors, step by step:  L = log a: 3 ulp |L|;  t = 2 beta_d L: 2 beta_d dL + e32 |t|;  q = beta_min^2 + t: dt + e32 |q|;
         r = sqrt q: dq / (2 r) + 3 ulp r;  d = r - beta_min: dr + e32 |d|;  e = d / beta_d: dd / beta_d + 2.5 ulp |e|;  c = (M-1) e:
         (M-1) de + e32 |c|.  At small sigma d -> 0 while dr stays near 3 ulp of beta_min, so the bound is ABSOLUTE there (about 1.8e-6 for the
         defaults) and no relative tolerance of c_noise itself could stand in for it.  The first-order sum is widened by 1 % for the
         second-order terms.
  iDDPM c_noise = (M-1) - j, j the index of the nearest table entry to s: exact, bound 0.  The reference index does not scan: the table is
         strictly decreasing, so the nearest entry is one of the two that bracket s, and those two distances are compared as Fractions (first
         index on a tie).
  xin = c_in * f32(x): c_in's relative bound + e32.
"""
from fractions import Fraction

import numpy as np

E32 = 2.0 ** -24
ULP = 2 * E32
LOG_ULPS, SQRT_ULPS, DIV_ULPS = 3, 3, 2.5
C_IN_REL = (1 + 2 * SQRT_ULPS + 2 * DIV_ULPS) * E32
F = np.float32
MISTAKES = ('c_out_sign', 'M_not_M1', 'last_tie', 'row0_sigma')
WRAP_CHW = 3 * 256 * 256                        # with n = 3: n * chw > 2048 blocks * 256 threads, the second trip of the grid-stride loop


def scalars(M=1000, beta_d=19.9, beta_min=0.1):
    """(M-1, beta_min^2, 2 beta_d, beta_min, beta_d): evaluated in double, rounded to float32 once"""
    return tuple(F(v) for v in (M - 1, beta_min ** 2, 2 * beta_d, beta_min, beta_d))


def f32_sigma(sigma):
    return np.asarray(sigma, dtype=np.float64).reshape(-1).astype(F)


def nearest_index(s32, u):
    """exact argmin_j |s - u[j]| over a strictly decreasing float32 table, first index on a tie: bracket by comparison, decide by Fraction"""
    u = np.asarray(u, dtype=F)
    assert np.all(u[1:] < u[:-1])
    out = np.empty(len(s32), dtype=np.int64)
    for i, s in enumerate(np.asarray(s32, dtype=F)):
        k = int(np.sum(u > s))                  # entries above s: u[k-1] > s >= u[k]
        if k == 0:
            out[i] = 0
        elif k == len(u):
            out[i] = len(u) - 1
        else:
            above, below = Fraction(float(u[k - 1])) - Fraction(float(s)), Fraction(float(s)) - Fraction(float(u[k]))
            out[i] = k - 1 if above <= below else k
    return out


def coef_ref(kind, sigma, M=1000, beta_d=19.9, beta_min=0.1, u=None):
    """(reference, bound) float64 [n, 4]; see the module docstring"""
    s32 = f32_sigma(sigma)
    s = s32.astype(np.float64)
    m1, bmin2, bd2, bmin, bd = (float(v) for v in scalars(M, beta_d, beta_min))
    n = len(s)
    ref, bound = np.zeros((n, 4)), np.zeros((n, 4))
    ref[:, 0] = 1.0
    if kind == 've':
        ref[:, 1], ref[:, 2] = s, 1.0
        ref[:, 3] = np.log(0.5 * s)
        bound[:, 3] = LOG_ULPS * ULP * np.abs(ref[:, 3]) + 2.0 ** -149
        return ref, bound
    ref[:, 1] = -s
    ref[:, 2] = 1.0 / np.sqrt(s * s + 1.0)
    bound[:, 2] = C_IN_REL * ref[:, 2]
    if kind == 'iddpm':
        ref[:, 3] = m1 - nearest_index(s32, u)
        return ref, bound
    assert kind == 'vp'
    a = (F(1.0) + s32 * s32).astype(np.float64)                 # float32 arithmetic on float32 arrays: the value both sides share
    L = np.log(a)
    t = bd2 * L
    q = bmin2 + t
    r = np.sqrt(q)
    d = r - bmin
    e = d / bd
    c = m1 * e
    dL = LOG_ULPS * ULP * np.abs(L)
    dt = bd2 * dL + E32 * np.abs(t)
    dq = dt + E32 * np.abs(q)
    dr = dq / (2 * r) + SQRT_ULPS * ULP * r
    dd = dr + E32 * np.abs(d)
    de = dd / bd + DIV_ULPS * ULP * np.abs(e)
    ref[:, 3] = c
    bound[:, 3] = 1.01 * (m1 * de + E32 * np.abs(c))
    return ref, bound


def coef_model(kind, sigma, M=1000, beta_d=19.9, beta_min=0.1, u=None, mistake=None):
    """float32 numpy model of precond_coef_kernel's steps, one rounding per line; `mistake`: one of MISTAKES planted"""
    assert mistake is None or mistake in MISTAKES
    s = f32_sigma(sigma)
    if mistake == 'row0_sigma':
        s = np.full_like(s, s[0])
    m1, bmin2, bd2, bmin, bd = scalars(M + 1 if mistake == 'M_not_M1' else M, beta_d, beta_min)
    out = np.zeros((len(s), 4), dtype=F)
    out[:, 0] = 1
    s2 = s * s
    if kind == 've':
        out[:, 1], out[:, 2] = s, 1
        out[:, 3] = np.log(F(0.5) * s)
    else:
        out[:, 1] = -s
        out[:, 2] = F(1) / np.sqrt(s2 + F(1))
        if kind == 'vp':
            a = F(1) + s2
            t = bd2 * np.log(a)
            r = np.sqrt(bmin2 + t)
            out[:, 3] = m1 * ((r - bmin) / bd)
        else:
            d = np.abs(s.astype(np.float64)[:, None] - np.asarray(u, dtype=np.float64)[None, :])      # the kernel's distances: in double
            j = d.argmin(1)                                                                           # first index on a tie
            if mistake == 'last_tie':
                j = d.shape[1] - 1 - d[:, ::-1].argmin(1)
            out[:, 3] = m1 - j.astype(F)
    if mistake == 'c_out_sign':
        out[:, 1] = -out[:, 1]
    assert out.dtype == F
    return out


def xin_ref(kind, x, sigma, **kw):
    """(reference, bound) of xin = c_in * f32(x), x [n, ...] float64, sigma [1] or [n]"""
    x32 = np.asarray(x, dtype=np.float64).astype(F).astype(np.float64)
    n = x32.shape[0]
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64).reshape(-1), (n,))
    ref, bound = coef_ref(kind, sig, **kw)
    shape = (n,) + (1,) * (x32.ndim - 1)
    want = ref[:, 2].reshape(shape) * x32
    rel = 0.0 if kind == 've' else C_IN_REL + E32
    return want, rel * np.abs(want)


def check(got, ref, bound):
    """the largest excess of |got - ref| over the bound, as (excess, flat index); <= 0 means every element is inside"""
    ex = np.abs(np.asarray(got, dtype=np.float64) - ref) - bound
    i = int(np.argmax(ex))
    return float(ex.reshape(-1)[i]), i


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def sigma_sweep(lo, hi, count=257):
    """log-spaced float64 sigmas across a network's range, end points included"""
    return np.exp(np.linspace(np.log(lo), np.log(hi), count))


def table_midpoints(u):
    """(sigmas, the lower index of each pair): the midpoints (u[j] + u[j+1]) / 2 that are exactly representable in float32 -- exact ties,
    where the first index j must win"""
    u64 = np.asarray(u, dtype=F).astype(np.float64)
    mid = (u64[:-1] + u64[1:]) / 2                              # exact in float64
    ok = mid.astype(F).astype(np.float64) == mid
    return mid[ok], np.nonzero(ok)[0]


def index_cases(u):
    """every table entry, the representable midpoints, sigmas above u[0] and below u[M-1], and 0"""
    u64 = np.asarray(u, dtype=F).astype(np.float64)
    mids, _ = table_midpoints(u)
    extra = np.array([u64[0] * 1.5, u64[0] * 1e6, 1.0e18, u64[-2] * 0.75, u64[-2] * 0.5, u64[-2] * 0.49, u64[-2] * 1e-3, 1e-30, 0.0])
    return np.concatenate([u64, mids, extra])
