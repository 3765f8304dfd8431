"""References and bounds for the plain samplers (diffusion_tts_amd/plain.py) and the general ODE step kernels (csrc/elementwise.hip, K9b).
numpy / torch on the CPU only; nothing here imports the code under test.

1. The three kernel expressions in float64 torch with the project's standing bound for the float64 step kernels
   (elementwise_reference.heun_*_ref): 8 e64 x the sum of the magnitudes of the terms of each expression -- the kernel's <= 5 roundings per
   result and the reference's own, contracted or not.  x_in = x / s is held to more than that: float64 division is correctly rounded on both
   sides, so x_in must EQUAL (the x the kernel stored) / s bit for bit.  A multiplication by the reciprocal is 1 to 2 roundings off, inside
   any bound of the 8 e64 kind; only equality tells it from a division.

2. The schedule and the per-step host scalars of edm/generate.py:78-165 restated in float64 with a RUNNING ERROR BOUND (class V: a value and
   a bound on its distance from the exact result of the same expression on the same inputs).  Every arithmetic operation adds one rounding,
   e64 |result|, to the first-order propagation of its operands' bounds -- |b| ea + |a| eb for a product, ea + eb for a sum (which is where
   cancellation shows: the bound stays, the value shrinks), |f'(a)| ea for a function -- and a library function (exp, log, pow, sin) adds
   LIBM_ULPS = 4 ulp of its result instead of half an ulp: torch's CPU kernels call the host's vector library, whose documented accuracy is
   1 ulp for the variants torch uses; 4 allows for another library on another host.  sqrt is correctly rounded.  So the bound of a quantity
   is its operation count weighted by its conditioning, and two hosts' float64 evaluations of it differ by at most twice the bound.
   A square root of a difference that may vanish (the noise coefficient when nothing is churned: sigma(sigma_inv(sigma(t))) against
   sigma(t)) is bounded through the root's values at the two ends of [value - bound, value + bound], not by a first-order term that would
   divide by zero.
   The iDDPM table takes alpha_bar in FLOAT32 (a python float times an integer tensor): 15 e32 relative per entry as
   precond_helpers.iddpm_table_f64 counts it (three float32 operations, a 2 ulp sine, the square).
"""
import math

import numpy as np
import torch

E32, E64 = 2.0 ** -24, 2.0 ** -53
ODE_K = 8
LIBM_ULPS = 4


# ---- 1. kernels ------------------------------------------------------------------------------------------------------------------------
def ode_xhat_ref(x_cur, eps, ratio, coef, s_hat):
    """(x_hat, bound), (x_in, bound): x_hat = ratio x + coef eps, 8 e64 (|ratio x| + |coef eps|); x_in = x_hat / s_hat, the same over |s_hat|"""
    t0 = ratio * x_cur
    t1 = torch.zeros_like(x_cur) if eps is None else coef * eps.double()
    mag = ODE_K * E64 * (t0.abs() + t1.abs())
    return (t0 + t1, mag), ((t0 + t1) / s_hat, mag / abs(s_hat))


def ode_slope_ref(x, D, a, b, base, step, s_out):
    """(d, bound), (x_out, bound), (x_in, bound): d = a x - b D, 8 e64 (|a x| + |b D|) =: 8 e64 m; x_out = base + step d, 8 e64 (|base| + |step| m)"""
    t0, t1 = a * x, b * D.double()
    m = t0.abs() + t1.abs()
    d = t0 - t1
    out = base + step * d
    bo = ODE_K * E64 * (base.abs() + abs(step) * m)
    return (d, ODE_K * E64 * m), (out, bo), (out / s_out, bo / abs(s_out))


def ode_correct_ref(x_hat, x_prime, D2, d_cur, a, b, h, w0, w1):
    """x_next = x_hat + h (w0 d_cur + w1 (a x' - b D')): 8 e64 (|x_hat| + |h| (|w0 d_cur| + |w1| (|a x'| + |b D'|)))"""
    t0, t1 = a * x_prime, b * D2.double()
    dp = t0 - t1
    m = (w0 * d_cur).abs() + abs(w1) * (t0.abs() + t1.abs())
    return x_hat + h * (w0 * d_cur + w1 * dp), ODE_K * E64 * (x_hat.abs() + abs(h) * m)


def ode_xhat_model(x_cur, eps, ratio, coef, s_hat, reciprocal=False):
    """numpy float64 model of the kernel (products and sums rounded one by one); reciprocal=True: the mistake x_in = x_hat * (1 / s_hat)"""
    v = np.float64(ratio) * x_cur.numpy()
    if eps is not None:
        v = v + np.float64(coef) * eps.double().numpy()
    x_in = v * (np.float64(1.0) / np.float64(s_hat)) if reciprocal else v / np.float64(s_hat)
    return torch.from_numpy(v), torch.from_numpy(x_in)


def ode_slope_model(x, D, a, b, base, step, s_out, b_without_s=None):
    """b_without_s = s: the mistake of b = sigma'/sigma instead of sigma' s / sigma (the caller passes the s that was left out)"""
    bb = np.float64(b) / np.float64(b_without_s) if b_without_s is not None else np.float64(b)
    d = np.float64(a) * x.numpy() - bb * D.double().numpy()
    out = base.numpy() + np.float64(step) * d
    return torch.from_numpy(d), torch.from_numpy(out), torch.from_numpy(out / np.float64(s_out))


def ode_correct_model(x_hat, x_prime, D2, d_cur, a, b, h, w0, w1, swap_weights=False):
    if swap_weights:
        w0, w1 = w1, w0
    dp = np.float64(a) * x_prime.numpy() - np.float64(b) * D2.double().numpy()
    return torch.from_numpy(x_hat.numpy() + np.float64(h) * (np.float64(w0) * d_cur.numpy() + np.float64(w1) * dp))


def true_div(x, s):
    """x / s by an IEEE division per element.  (torch divides a tensor by a scalar by multiplying with its reciprocal, on the CPU and on the
    GPU -- so does the reference's x_hat / s(t_hat); numpy divides.)"""
    return torch.from_numpy(x.detach().cpu().numpy() / np.float64(s))


def worst(got, ref, bound):
    """max err / bound (0 / 0 counts as 0) and max err"""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-320))
    return float(ratio.max()), float(err.max())


def ode_inputs(count, seed, scale=300.0):
    """x, base, d_cur float64 (states of the size the tiny networks' trajectories reach), D float32, eps float64"""
    g = torch.Generator().manual_seed(seed)
    r = lambda dt=torch.float64: torch.randn(count, generator=g, dtype=dt)
    return dict(x=r() * scale, base=r() * scale, d=r() * scale, D=r(torch.float32) * 3, eps=r())


# ---- 2. schedule ---------------------------------------------------------------------------------------------------------------------------
class V:
    """value (numpy float64, any shape) with a bound on its distance from the exact result"""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def _r(self, v, e, ulps=0.5):
        return V(v, e + 2 * ulps * E64 * np.abs(v))

    def __add__(self, o):
        o = V.of(o)
        return self._r(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __neg__(self):
        return V(-self.v, self.e)

    def __sub__(self, o):
        return self + (-V.of(o))

    def __rsub__(self, o):
        return V.of(o) + (-self)

    def __mul__(self, o):
        o = V.of(o)
        return self._r(self.v * o.v, np.abs(o.v) * self.e + np.abs(self.v) * o.e + self.e * o.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        lo = np.maximum(np.abs(o.v) - o.e, 1e-300)
        with np.errstate(divide='ignore', invalid='ignore'):
            return self._r(self.v / o.v, self.e / lo + np.abs(self.v / o.v) * o.e / lo)

    def __rtruediv__(self, o):
        return V.of(o) / self

    def sqrt(self):
        v = np.maximum(self.v, 0.0)
        with np.errstate(invalid='ignore'):
            # no first-order step: the root's own values at the two ends of [v - e, v + e] (concave: the lower end moves furthest, until it is cut at 0)
            e = np.maximum(np.sqrt(v) - np.sqrt(np.maximum(v - self.e, 0.0)), np.sqrt(v + self.e) - np.sqrt(v))
        return self._r(np.sqrt(v), np.where(self.e == 0, 0.0, e))

    def exp(self):
        r = np.exp(self.v)
        return self._r(r, r * np.expm1(self.e), LIBM_ULPS)

    def log(self):
        return self._r(np.log(self.v), self.e / np.maximum(np.abs(self.v) - self.e, 1e-300), LIBM_ULPS)

    def pow(self, p):
        """self ** p, p an exact constant (p = 2, 3: products would be tighter; a library call covers them)"""
        r = self.v ** p
        with np.errstate(divide='ignore', invalid='ignore'):
            rel = np.where(self.v == 0, 0.0, abs(p) * self.e / np.maximum(np.abs(self.v) - self.e, 1e-300))
        return self._r(r, np.abs(r) * rel, LIBM_ULPS)

    def clip0(self):
        return V(np.maximum(self.v, 0.0), self.e)

    def __getitem__(self, i):
        return V(self.v[i], self.e[i])


def iddpm_table(M, C_1, C_2, drop_clip=False):
    """the u recursion of edm/generate.py:110-114 as V: alpha_bar in float32 (15 e32 relative), everything after it in float64"""
    j = np.arange(M + 1)
    arg = (np.float32(0.5 * np.pi) * j.astype(np.float32) / np.float32(M) / np.float32(C_2 + 1)).astype(np.float32)
    ab32 = (np.sin(arg).astype(np.float32) ** 2).astype(np.float32)
    ab = V(ab32.astype(np.float64), 15 * E32 * ab32.astype(np.float64))
    u = [None] * (M + 1)
    u[M] = V(0.0)
    for k in range(M, 0, -1):
        with np.errstate(divide='ignore', invalid='ignore'):
            r32 = np.float32(ab32[k - 1]) / np.float32(ab32[k])                           # the reference divides the two float32 values
        ratio = V(float(r32), float(r32) * 31 * E32)
        if not drop_clip:
            ratio = V(max(float(ratio.v), C_1), ratio.e)
        with np.errstate(divide='ignore', invalid='ignore'):
            u[k - 1] = ((u[k] * u[k] + 1) / ratio - 1).sqrt()
    return V(np.array([float(t.v) for t in u]), np.array([float(t.e) for t in u]))


class Schedule:
    """sigma, sigma', sigma^-1, s, s' of one (schedule, scaling) choice over V"""

    def __init__(self, schedule, scaling, beta_d, beta_min):
        self.kind, self.scaling, self.bd, self.bm = schedule, scaling, beta_d, beta_min

    def vp_sigma(self, t, bd=None, bm=None):
        bd, bm = (self.bd if bd is None else bd), (self.bm if bm is None else bm)
        return ((0.5 * bd * (t * t) + bm * t).exp() - 1).sqrt()

    def sigma(self, t):
        return self.vp_sigma(t) if self.kind == 'vp' else t.sqrt() if self.kind == 've' else t

    def sigma_deriv(self, t):
        if self.kind == 'vp':
            sg = self.sigma(t)
            return 0.5 * (self.bm + self.bd * t) * (sg + 1 / sg)
        return 0.5 / t.sqrt() if self.kind == 've' else V(1.0)

    def sigma_inv(self, sg):
        if self.kind == 'vp':
            return ((self.bm * self.bm + 2 * self.bd * (sg * sg + 1).log()).sqrt() - self.bm) / self.bd
        return sg * sg if self.kind == 've' else sg

    def s(self, t):
        if self.scaling == 'none':
            return V(1.0)
        sg = self.sigma(t)
        return 1 / (1 + sg * sg).sqrt()

    def s_deriv(self, t):
        if self.scaling == 'none':
            return V(0.0)
        st = self.s(t)
        return -(self.sigma(t) * self.sigma_deriv(t) * (st * st * st))


def schedule_ref(net_min, net_max, round_sigma, num_steps, sigma_min=None, sigma_max=None, rho=7, solver='heun', discretization='edm',
                 schedule='linear', scaling='none', epsilon_s=1e-3, C_1=0.001, C_2=0.008, M=1000, alpha=1, S_churn=0, S_min=0,
                 S_max=float('inf'), S_noise=1, drop_clip=False, floor_index=False):
    """edm/generate.py:78-165 over V.  round_sigma: V -> V (the identity, or the network's table with its margin check).  Returns a dict of
    V arrays: t_steps [num_steps + 1] and, per step, t_hat, sigma_hat, ratio, noise_coef, a, b, h.  drop_clip / floor_index: the mistakes."""
    paper = Schedule('vp', 'none', 19.9, 0.1)
    if sigma_min is None:
        sigma_min = {'vp': paper.vp_sigma(V(epsilon_s)), 've': V(0.02), 'iddpm': V(0.002), 'edm': V(0.002)}[discretization]
    if sigma_max is None:
        sigma_max = {'vp': paper.vp_sigma(V(1.0)), 've': V(100.0), 'iddpm': V(81.0), 'edm': V(80.0)}[discretization]
    sigma_min, sigma_max = V.of(sigma_min), V.of(sigma_max)
    if float(sigma_min.v) < net_min:
        sigma_min = V(net_min)
    if float(sigma_max.v) > net_max:
        sigma_max = V(net_max)
    lmin, lmax = (sigma_min * sigma_min + 1).log(), (sigma_max * sigma_max + 1).log()
    beta_d = 2 * (lmin / epsilon_s - lmax) / (epsilon_s - 1)
    beta_min = lmax - 0.5 * beta_d
    sch = Schedule(schedule, scaling, beta_d, beta_min)
    idx = V(np.arange(num_steps, dtype=np.float64))
    frac = idx / (num_steps - 1)
    if discretization == 'vp':
        sigma_steps = sch.vp_sigma(1 + frac * (epsilon_s - 1), beta_d, beta_min)
    elif discretization == 've':
        q = sigma_min * sigma_min / (sigma_max * sigma_max)
        lq = q.log()
        pw = (lq * frac).exp()                                                             # q ** frac
        sigma_steps = (sigma_max * sigma_max * pw).sqrt()
    elif discretization == 'iddpm':
        u = iddpm_table(M, C_1, C_2, drop_clip)
        keep = np.logical_and(u.v >= float(sigma_min.v), u.v <= float(sigma_max.v))
        kept = V(u.v[keep], u.e[keep])
        pos = (len(kept.v) - 1) / (num_steps - 1) * np.arange(num_steps)
        take = (np.floor(pos) if floor_index else np.round(pos)).astype(np.int64)         # np.round: half to even, as torch
        sigma_steps = kept[take]
    else:
        a_, b_ = sigma_max.pow(1 / rho), sigma_min.pow(1 / rho)
        sigma_steps = (a_ + frac * (b_ - a_)).pow(rho)
    t = sch.sigma_inv(round_sigma(sigma_steps))
    t_steps = V(np.concatenate([t.v, [0.0]]), np.concatenate([t.e, [0.0]]))
    keys = ('t_hat', 'sigma_hat', 'ratio', 'noise_coef', 'a', 'b', 'h')
    rows = {k: [] for k in keys}
    for i in range(num_steps):
        t_cur, t_next = t_steps[i], t_steps[i + 1]
        sc = sch.sigma(t_cur)
        churned = S_min <= float(sc.v) <= S_max
        gamma = min(S_churn / num_steps, math.sqrt(2) - 1) if churned else 0
        t_hat = sch.sigma_inv(round_sigma(sc + gamma * sc))
        sh, s_hat = sch.sigma(t_hat), sch.s(t_hat)
        vals = dict(t_hat=t_hat, sigma_hat=sh, ratio=s_hat / sch.s(t_cur), noise_coef=(sh * sh - sc * sc).clip0().sqrt() * s_hat * S_noise,
                    a=sch.sigma_deriv(t_hat) / sh + sch.s_deriv(t_hat) / s_hat, b=sch.sigma_deriv(t_hat) * s_hat / sh, h=t_next - t_hat)
        for k in keys:
            rows[k].append(vals[k])
    out = {k: V(np.array([float(r.v) for r in rows[k]]), np.array([float(r.e) for r in rows[k]])) for k in keys}
    out['t_steps'] = t_steps
    return out


def table_rounding(table):
    """round_sigma of an iDDPM network over V: the nearest entry of its float32 table -- exact, bound 0.  The argument is itself an entry of
    the SAME recursion evaluated a second time (the sampler's float64 one against the network's float32 one), so the two differ by float32
    roundings, parts in 1e6, against a table spacing of parts in 1e2: the choice is taken as decided, and asserted to be, when the nearest
    entry is at most 5 % as far as the second nearest (the margin tests/golden/make_golden_preconds.py asks of its noise levels)."""
    tab = np.asarray(table, dtype=np.float64)

    def rs(x):
        d = np.abs(np.float32(x.v).astype(np.float64).reshape(-1, 1) - tab.reshape(1, -1))
        two = np.sort(d, 1)[:, :2]
        assert np.all(two[:, 0] <= 0.05 * two[:, 1]), 'a noise level too close to the midpoint of two table entries'
        return V(tab[d.argmin(1)].reshape(x.v.shape), 0.0)
    return rs


def identity(x):
    return x


def excess(got, ref):
    """max over the elements of |got - ref.v| / (2 ref.e): above 1 = outside what two float64 evaluations may differ by.  A zero bound asks
    for equality (0 / 0 counts as 0); an infinite or NaN value on either side counts as infinitely far unless both are the same."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        err = np.abs(got - ref.v)
        err = np.where(got == ref.v, 0.0, np.where(np.isfinite(err), err, np.inf))
        r = np.where(err == 0, 0.0, err / np.maximum(2 * ref.e, 1e-320))
    return float(np.max(r))
