"""Plain (search-free) batched sampling on MI355X: the two samplers of the reference's bulk generator (edm/generate.py) as device loops.

`edm_sampler` (edm/generate.py:25-60) is the EDM Heun step on the K9 kernels (ops.heun_*), `ablation_sampler` (edm/generate.py:66-176) the
general ODE  dx/dt = (sigma'/sigma + s'/s) x - (sigma' s / sigma) D(x / s; sigma)  with its choice of solver, time discretisation, noise
schedule sigma(t) and scaling s(t), on the K9b kernels (ops.ode_*).  Both are row for row: every row of a batch is its own trajectory.

What stays on the host, as in sampler.py: the schedule and every per-step scalar (float64 torch operations in the reference's order of
operations, `ode_schedule`), and the random numbers.  `StackedRandomGenerator` keeps one CPU generator per row, so a seed's image does not
depend on the batch it is generated in; the reference draws on the CUDA device, a stream no other device reproduces.  The noise of a step is
drawn every step (the stream stays the reference's) and uploaded once (ablation_sampler: only when its coefficient is not zero).
sampler.py builds on this file: the EDM schedule (`edm_sigmas`), the churn rule (`churn_of`) and the Heun step (`heun_step`, `heun_loop`) exist here, once.
"""
import math

import numpy as np
import torch

from . import ops

SOLVERS = ('euler', 'heun')
DISCRETIZATIONS = ('vp', 've', 'iddpm', 'edm')
SCHEDULES = ('vp', 've', 'linear')
SCALINGS = ('vp', 'none')


class StackedRandomGenerator:
    """One CPU torch.Generator per row (seed mod 2^32, edm/generate.py:182-196): row i of every draw is what a lone generator seeded with
    seeds[i] draws, whatever else is in the batch.  `device=` arguments are accepted and ignored: the numbers are drawn on the host."""

    def __init__(self, seeds):
        self.generators = [torch.Generator().manual_seed(int(seed) % (1 << 32)) for seed in seeds]

    def _rows(self, size):
        size = tuple(size)
        if not size or size[0] != len(self.generators):
            raise ValueError(f'StackedRandomGenerator: {len(self.generators)} generators, asked for a first dimension of {size[:1]}')
        return size[1:]

    def randn(self, size, **kwargs):
        kwargs.pop('device', None)
        rest = self._rows(size)
        return torch.stack([torch.randn(rest, generator=g, **kwargs) for g in self.generators])

    def randn_like(self, input):
        return self.randn(input.shape, dtype=input.dtype, layout=input.layout)

    def randint(self, *args, size, **kwargs):
        kwargs.pop('device', None)
        rest = self._rows(size)
        return torch.stack([torch.randint(*args, size=rest, generator=g, **kwargs) for g in self.generators])


def host_randn_like(x):
    """the default noise source: the torch CPU global generator (the rule of sampler.py)"""
    return torch.randn(x.shape, dtype=x.dtype)


def _choice(name, value, allowed):
    if value not in allowed:
        raise ValueError(f'{name}={value!r}: one of {list(allowed)}')


class _VP:
    """sigma(t) = sqrt(exp(beta_d t^2 / 2 + beta_min t) - 1) and its inverse (python numbers or float64 tensors)"""

    def __init__(self, beta_d, beta_min):
        self.beta_d, self.beta_min = beta_d, beta_min

    def sigma(self, t):
        return (math.e ** (0.5 * self.beta_d * (t ** 2) + self.beta_min * t) - 1) ** 0.5

    def inverse(self, sigma):
        return ((self.beta_min ** 2 + 2 * self.beta_d * (sigma ** 2 + 1).log()).sqrt() - self.beta_min) / self.beta_d


def ode_schedule(net, num_steps=18, sigma_min=None, sigma_max=None, rho=7, discretization='edm', schedule='linear', scaling='none',
                 epsilon_s=1e-3, C_1=0.001, C_2=0.008, M=1000):
    """(t_steps, sigma, sigma_deriv, sigma_inv, s, s_deriv) of edm/generate.py:78-147, on the host in float64.
    t_steps: num_steps + 1 times, the last one 0; the callables map a float64 tensor t (sigma_inv: a noise level) to a float64 tensor, or to
    the python constant the reference uses (the linear schedule's derivative 1, no scaling: s = 1, s' = 0)."""
    _choice('discretization', discretization, DISCRETIZATIONS)
    _choice('schedule', schedule, SCHEDULES)
    _choice('scaling', scaling, SCALINGS)
    # default range by discretisation (:86-92), then the network's own (:95-96)
    paper_vp = _VP(19.9, 0.1)
    if sigma_min is None:
        sigma_min = {'vp': paper_vp.sigma(epsilon_s), 've': 0.02, 'iddpm': 0.002, 'edm': 0.002}[discretization]
    if sigma_max is None:
        sigma_max = {'vp': paper_vp.sigma(1), 've': 100, 'iddpm': 81, 'edm': 80}[discretization]
    sigma_min = max(sigma_min, net.sigma_min)
    sigma_max = min(sigma_max, net.sigma_max)
    # the VP betas that put sigma(epsilon_s) = sigma_min and sigma(1) = sigma_max (:99-100)
    beta_d = float(2 * (np.log(sigma_min ** 2 + 1) / epsilon_s - np.log(sigma_max ** 2 + 1)) / (epsilon_s - 1))
    beta_min = float(np.log(sigma_max ** 2 + 1) - 0.5 * beta_d)
    vp = _VP(beta_d, beta_min)

    idx = torch.arange(num_steps, dtype=torch.float64)
    if discretization == 'vp':
        sigma_steps = vp.sigma(1 + idx / (num_steps - 1) * (epsilon_s - 1))
    elif discretization == 've':
        sigma_steps = ((sigma_max ** 2) * ((sigma_min ** 2 / sigma_max ** 2) ** (idx / (num_steps - 1)))).sqrt()
    elif discretization == 'iddpm':
        # the recursion of :110-114, entry by entry like the reference: alpha_bar of an INTEGER tensor index is a float32 value there (a
        # python float times an int64 tensor), one scalar sine per entry, and the rest of the step is float64
        u = torch.zeros(M + 1, dtype=torch.float64)

        def alpha_bar(k):
            return (0.5 * np.pi * k / M / (C_2 + 1)).sin() ** 2
        for k in torch.arange(M, 0, -1):
            kept_share = (alpha_bar(k - 1) / alpha_bar(k)).clip(min=C_1)              # alpha_j = alpha_bar_j / alpha_bar_{j+1}, floored
            u[k - 1] = ((u[k] ** 2 + 1) / kept_share - 1).sqrt()
        kept = u[torch.logical_and(u >= sigma_min, u <= sigma_max)]
        sigma_steps = kept[((len(kept) - 1) / (num_steps - 1) * idx).round().to(torch.int64)]
    else:
        sigma_steps = edm_sigmas(num_steps, sigma_min, sigma_max, rho)

    if schedule == 'vp':
        sigma, sigma_inv = vp.sigma, vp.inverse

        def sigma_deriv(t):
            return 0.5 * (beta_min + beta_d * t) * (sigma(t) + 1 / sigma(t))
    elif schedule == 've':
        def sigma(t):
            return t.sqrt()

        def sigma_deriv(t):
            return 0.5 / t.sqrt()

        def sigma_inv(sig):
            return sig ** 2
    else:
        def sigma(t):
            return t

        def sigma_deriv(t):
            return 1

        def sigma_inv(sig):
            return sig

    if scaling == 'vp':
        def s(t):
            return 1 / (1 + sigma(t) ** 2).sqrt()

        def s_deriv(t):
            return -sigma(t) * sigma_deriv(t) * (s(t) ** 3)
    else:
        def s(t):
            return 1

        def s_deriv(t):
            return 0

    t_steps = sigma_inv(net.round_sigma(sigma_steps))
    t_steps = torch.cat([t_steps, torch.zeros_like(t_steps[:1])])
    return t_steps, sigma, sigma_deriv, sigma_inv, s, s_deriv


def ode_step_scalars(t_cur, t_next, sched, round_sigma, num_steps, alpha=1, S_churn=0, S_min=0, S_max=float('inf'), S_noise=1):
    """The host scalars of one step (edm/generate.py:156-165) as python floats: t_hat, h, the kernel arguments of x_hat (ratio, noise_coef,
    s_hat), of the slope at t_hat (a, b, sigma_hat) and the predictor's time t_prime = t_hat + alpha h."""
    _, sigma, sigma_deriv, sigma_inv, s, s_deriv = sched
    sig_cur = sigma(t_cur)
    gamma = min(S_churn / num_steps, np.sqrt(2) - 1) if S_min <= sig_cur <= S_max else 0
    t_hat = sigma_inv(round_sigma(sig_cur + gamma * sig_cur))
    sig_hat, s_hat = sigma(t_hat), s(t_hat)
    h = t_next - t_hat
    return dict(t_hat=t_hat, h=float(h), ratio=float(s_hat / s(t_cur)),
                noise_coef=float((sig_hat ** 2 - sig_cur ** 2).clip(min=0).sqrt() * s_hat * S_noise), s_hat=float(s_hat),
                sigma_hat=sig_hat, t_prime=t_hat + alpha * h, **slope_scalars(t_hat, sched))


def slope_scalars(t, sched):
    """a = sigma'/sigma + s'/s and b = sigma' s / sigma at time t (edm/generate.py:163)"""
    _, sigma, sigma_deriv, _, s, s_deriv = sched
    return dict(a=float(sigma_deriv(t) / sigma(t) + s_deriv(t) / s(t)), b=float(sigma_deriv(t) * s(t) / sigma(t)))


def _start(net, latents, class_labels, scale):
    dev = net.device
    x = (latents.to(torch.float64).cpu() * scale).to(dev).contiguous()
    labels = None if class_labels is None else class_labels.to(dev, torch.float32).contiguous()
    return dev, x, labels


def _noise(randn_like, x_cur, coef, dev):
    """the ablation step's draw (made whether or not it is used), on the device when it is"""
    eps = randn_like(x_cur)
    return None if coef == 0.0 else eps.to(dev).contiguous()


def edm_sigmas(num_steps, sigma_min, sigma_max, rho):
    """The EDM time discretisation (edm/main.py:78-79, edm/generate.py:38-39): num_steps noise levels from sigma_max down to sigma_min, float64
    on the host.  Clamping to the network's range, rounding with net.round_sigma and the final 0 are each caller's own."""
    idx = torch.arange(num_steps, dtype=torch.float64)
    return (sigma_max ** (1 / rho) + idx / (num_steps - 1) * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho


def edm_schedule(net, num_steps, sigma_min, sigma_max, rho):
    """t_steps of edm_sampler (edm/generate.py:33-40): the range clamped to the network's own, `edm_sigmas`, rounded, then 0"""
    t_steps = edm_sigmas(num_steps, max(sigma_min, net.sigma_min), min(sigma_max, net.sigma_max), rho)
    return torch.cat([net.round_sigma(t_steps), torch.zeros_like(t_steps[:1])])


def churn_of(t_cur, num_steps, S_churn, S_min, S_max, S_noise, round_sigma):
    """(t_hat, noise coefficient) of the sigma step that starts at `t_cur` (edm/main.py:84-86, edm/generate.py:47-49); host arithmetic only"""
    gamma = min(S_churn / num_steps, np.sqrt(2) - 1) if S_min <= t_cur <= S_max else 0
    t_hat = round_sigma(t_cur + gamma * t_cur)
    coef = (t_hat ** 2 - t_cur ** 2).sqrt() * S_noise
    return float(t_hat), float(coef)


def heun_step(net, x_cur, eps, churn, t_next, last, labels, nb=None, interleave=False):
    """One EDM step (edm/main.py:82-96, edm/generate.py:44-58) on the K9 kernels.  x_cur [xb, ...] f64 is broadcast to nb rows (default: the
    rows of eps); eps [nb, ...] f64 | f32 on the device; churn = (t_hat, coef) of `churn_of`; last: the Euler step alone, no second-order
    correction.  Returns x_next, the first denoiser output D(x_hat, t_hat) and the last one (the same tensor at the last step)."""
    t_hat, coef = churn
    x_hat = ops.heun_xhat(x_cur, eps, coef, eps.shape[0] if nb is None else nb, interleave)
    D = D1 = net(x_hat, torch.tensor([t_hat], dtype=torch.float64), labels)
    d_cur, x_next = ops.heun_euler(x_hat, D, t_hat, float(t_next))
    if not last:
        D = net(x_next, torch.as_tensor(t_next, dtype=torch.float64).reshape(1), labels)
        ops.heun_correct(x_hat, D, d_cur, t_hat, float(t_next), x_next)
    return x_next, D1, D


def heun_step_rows(net, x_cur, eps, t_hat, coef, t_next, labels, interleave=True):
    """`heun_step` with the step's scalars PER ROW (the per-row K9 kernels): rows of one launch stand at different sigma steps, none at the last
    one.  t_hat, coef, t_next: host sequences of eps.shape[0] numbers -- checked here (no t_hat or t_next of 0: the device arrays cannot be
    checked without a read), uploaded once and shared by the three kernels and, as the per-row sigma, by the two denoiser calls.  x_cur
    [xb, ...] f64 is broadcast to the rows of eps.  Row r is the row `heun_step` computes with churn = (t_hat[r], coef[r]) and t_next[r].
    Returns x_next."""
    nb, dev = eps.shape[0], x_cur.device
    th = ops.row_scalars(t_hat, nb, 'heun_step_rows: t_hat', dev, nonzero=True)
    tn = ops.row_scalars(t_next, nb, 'heun_step_rows: t_next', dev, nonzero=True)
    x_hat = ops.heun_xhat_rows(x_cur, eps, ops.row_scalars(coef, nb, 'heun_step_rows: coef', dev), nb, interleave)
    D = net(x_hat, th, labels)
    d_cur, x_next = ops.heun_euler_rows(x_hat, D, th, tn)
    D = net(x_next, tn, labels)
    return ops.heun_correct_rows(x_hat, D, d_cur, th, tn, x_next)


def heun_loop(net, x_next, labels, t_steps, churn, draw):
    """The search-free trajectory over t_steps (the last one 0): per step one host draw `draw(x)` for the whole batch (made at zero-noise
    steps too: the stream is the reference's), uploaded, and one `heun_step`.  churn(t_cur) -> (t_hat, coef)."""
    last = len(t_steps) - 2
    for i in range(last + 1):
        eps = draw(x_next).to(x_next.device).contiguous()
        x_next = heun_step(net, x_next, eps, churn(t_steps[i]), t_steps[i + 1], i == last, labels)[0]
    return x_next


@torch.no_grad()
def edm_sampler(net, latents, class_labels=None, randn_like=host_randn_like, num_steps=18, sigma_min=0.002, sigma_max=80, rho=7,
                S_churn=0, S_min=0, S_max=float('inf'), S_noise=1):
    """edm/generate.py:25-60 on the K9 kernels: returns x_next, float64 on the device.  latents [n, c, r, r]; class_labels [n, label_dim] or None;
    `randn_like(x)` supplies a step's noise (x float64 [n, c, r, r]; a host tensor is uploaded).  The denoiser counts the rows in net.evals."""
    t_steps = edm_schedule(net, num_steps, sigma_min, sigma_max, rho)
    _, x_next, labels = _start(net, latents, class_labels, t_steps[0])
    return heun_loop(net, x_next, labels, t_steps, lambda t_cur: churn_of(t_cur, num_steps, S_churn, S_min, S_max, S_noise, net.round_sigma), randn_like)


@torch.no_grad()
def ablation_sampler(net, latents, class_labels=None, randn_like=host_randn_like, num_steps=18, sigma_min=None, sigma_max=None, rho=7,
                     solver='heun', discretization='edm', schedule='linear', scaling='none', epsilon_s=1e-3, C_1=0.001, C_2=0.008, M=1000,
                     alpha=1, S_churn=0, S_min=0, S_max=float('inf'), S_noise=1):
    """edm/generate.py:66-176 on the K9b kernels: returns x_next, float64 on the device.  Arguments as edm_sampler's, plus the four ablation
    choices; a value the reference asserts on is a ValueError."""
    _choice('solver', solver, SOLVERS)
    sched = ode_schedule(net, num_steps, sigma_min, sigma_max, rho, discretization, schedule, scaling, epsilon_s, C_1, C_2, M)
    t_steps, sigma, _, _, s, _ = sched
    dev, x_next, labels = _start(net, latents, class_labels, sigma(t_steps[0]) * s(t_steps[0]))
    for i in range(num_steps):
        k = ode_step_scalars(t_steps[i], t_steps[i + 1], sched, net.round_sigma, num_steps, alpha, S_churn, S_min, S_max, S_noise)
        x_hat, x_in = ops.ode_xhat(x_next, _noise(randn_like, x_next, k['noise_coef'], dev), k['ratio'], k['noise_coef'], k['s_hat'])
        D = net(x_in, torch.as_tensor(k['sigma_hat'], dtype=torch.float64).reshape(1), labels)
        if solver == 'euler' or i == num_steps - 1:
            _, x_next, _ = ops.ode_slope(x_hat, D, k['a'], k['b'], k['h'], want_d=False)
        else:
            t_prime = k['t_prime']
            d_cur, x_prime, x_in = ops.ode_slope(x_hat, D, k['a'], k['b'], alpha * k['h'], float(s(t_prime)))
            D = net(x_in, torch.as_tensor(sigma(t_prime), dtype=torch.float64).reshape(1), labels)
            kp = slope_scalars(t_prime, sched)
            x_next = ops.ode_correct(x_hat, x_prime, D, d_cur, kp['a'], kp['b'], k['h'], 1 - 1 / (2 * alpha), 1 / (2 * alpha))
    return x_next
