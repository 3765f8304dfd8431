"""GroupNorm in float64, written from the definition, and the seeded inputs ("regimes") the GroupNorm tests run on.
Torch on the CPU only: nothing here calls F.group_norm in float32 or anything of diffusion_tts_amd, so the kernels are
measured against something that shares no arithmetic with them (tests/test_groupnorm_reference.py pins this file)."""
import torch

K = 4                      # err(kernel) < K * max(e_ref32, 1e-7) * max(1, r^2): see tests/test_gpu_groupnorm.py
FLOOR = 1e-7

# name -> (r = |mean| / std the input is built with, sigma, limit on the reference's own f32 error e_ref32: a condition on the INPUT)
REGIMES = {
    'centred': (0.0, 1.0, 4e-7),
    'network_lo': (1.2, 0.15, 4e-7),       # the measured regime (|mean| / std <= 1.14), both ends of the measured std range
    'network_hi': (1.2, 3.0, 4e-7),
    'offset4': (4.0, 1.0, 1e-6),           # first regime where a one-pass variance shows
    'offset16': (16.0, 1.0, 4e-6),         # far outside
    'tiny': (1.0, 2.0 ** -9, 4e-7),        # var near eps: eps dominates rstd
    'large': (1.0, 300.0, 4e-7),           # sums of squares near 1e8 per thread
}


def regime_input(regime, n, c, h, w, seed):
    """float32 NCHW input of a regime: randn * sigma + r * sigma (the same offset in every group); returns (x, r)."""
    r, sigma, _ = REGIMES[regime]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=gen, dtype=torch.float64) * sigma + r * sigma
    return x.float(), r


def groups_of(c):
    return min(32, c // 4)


def gn_ref64(x1, x2, groups, eps, gamma, beta, scale_shift=None, silu=False, pool=False):
    """GroupNorm of concat(x1, x2) (NCHW float32 tensors) in float64: biased group variance, (x - mean) / sqrt(var + eps) * gamma + beta,
    then * (1 + scale) + shift (scale_shift [n, 2C] = scale | shift), then x * sigmoid(x), then the 2x2 average.
    Returns (y, a64, b64): a64, b64 [n, C] are the coefficients of the affine part, y_before_silu == x * a64 + b64."""
    x = (x1 if x2 is None else torch.cat([x1, x2], 1)).double()
    n, c, h, w = x.shape
    cg = c // groups
    assert cg * groups == c
    xg = x.reshape(n, groups, cg * h * w)
    mean = xg.sum(2) / (cg * h * w)
    var = ((xg - mean[:, :, None]) ** 2).sum(2) / (cg * h * w)
    mean_c = mean.repeat_interleave(cg, 1)[:, :, None, None]
    std_c = torch.sqrt(var + eps).repeat_interleave(cg, 1)[:, :, None, None]
    ga = torch.ones(c, dtype=torch.float64) if gamma is None else gamma.double()
    be = torch.zeros(c, dtype=torch.float64) if beta is None else beta.double()
    y = (x - mean_c) / std_c * ga[None, :, None, None] + be[None, :, None, None]
    a = ga[None, :] / std_c[:, :, 0, 0]
    b = be[None, :] - mean_c[:, :, 0, 0] * a
    if scale_shift is not None:
        sc, sh = 1.0 + scale_shift.double()[:, :c], scale_shift.double()[:, c:2 * c]
        y = y * sc[:, :, None, None] + sh[:, :, None, None]
        a, b = a * sc, b * sc + sh
    if silu:
        y = y * torch.sigmoid(y)
    if pool:
        y = y.reshape(n, c, h // 2, 2, w // 2, 2).sum((3, 5)) / 4.0
    return y, a, b


def err(got, ref64):
    """the one error measure: max |got - ref64| / max |ref64|, both in float64"""
    return float((got.double() - ref64).abs().max() / ref64.abs().max())


def ref32(x1, x2, eps, gamma, beta, scale_shift=None, silu=False, pool=False):
    """the reference's own float32 arithmetic of the same operation (oracle.edm_nets: torch's float32 group_norm, addcmul, silu, 2x2 mean)"""
    from oracle import edm_nets as onet
    x = x1 if x2 is None else torch.cat([x1, x2], 1)
    c = x.shape[1]
    y = onet.group_norm(x, gamma, beta, eps)
    if scale_shift is not None:
        y = torch.addcmul(scale_shift[:, c:, None, None], y, scale_shift[:, :c, None, None] + 1)
    if silu:
        y = onet.silu(y)
    if pool:
        y = onet.resample_down(y)
    return y


def bound(e_ref32, r, extra=0.0):
    return K * max(e_ref32, FLOOR) * max(1.0, r * r) + extra
