"""Test plumbing of the VP, VE and iDDPM preconditioners: the golden files of tests/golden/make_golden_preconds.py, the tiny networks' weights
pinned by their checksums, and a synthetic EDM network pickle of any of the four preconditioner classes."""
import collections
import json
import os
import pickle
import sys
import types

import numpy as np
import torch

from diffusion_tts_amd import init as dinit
from diffusion_tts_amd.config import EDMConfig

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KINDS = ('vp', 've', 'iddpm')
CLASS_NAMES = {'edm': 'EDMPrecond', 'vp': 'VPPrecond', 've': 'VEPrecond', 'iddpm': 'iDDPMPrecond'}
# what each class's constructor stores in its __dict__ besides img_resolution / img_channels / label_dim / use_fp16 (networks.py:482-492,
# 539-545, 584-599, 644-651)
RECORDED = {'edm': ('sigma_min', 'sigma_max', 'sigma_data'), 'vp': ('beta_d', 'beta_min', 'M', 'epsilon_t', 'sigma_min', 'sigma_max'),
            've': ('sigma_min', 'sigma_max'), 'iddpm': ('C_1', 'C_2', 'M', 'sigma_min', 'sigma_max')}


def golden():
    return np.load(os.path.join(GOLDEN, 'preconds_golden.npz'))


def manifest():
    with open(os.path.join(GOLDEN, 'preconds_manifest.json')) as f:
        return json.load(f)


def close(a, b, rel=1e-9):
    return abs(a - b) <= rel * max(1.0, abs(b))


def tiny_cfg(man, kind):
    return EDMConfig(**man[kind]['cfg'])


def with_golden_table(sd):
    """iDDPM: the state dict with the `u` table of the golden file in place of this machine's.  The constructor's recursion takes a float32
    sine per entry, which the host's vector library rounds differently from one CPU to the next, so the table the initialiser builds here need
    not be bit for bit the one the reference module carried when the goldens were recorded (test_preconds.py bounds the difference)."""
    if 'u' in sd:
        sd = collections.OrderedDict(sd)
        sd['u'] = torch.from_numpy(golden()['iddpm_u'].copy())
    return sd


def iddpm_table_f64(M=1000, C_1=0.001, C_2=0.008):
    """(u, bound): the recursion of networks.py:594-597 in float64, and how far a float32 evaluation may lie from it.  Per step, relative to
    w = 1 + u^2 = w_next / ratio:  the sine's argument is three float32 operations (3 e32, at most that relative to the sine) and the sine
    itself 2 ulp (4 e32), squared (x 2, + e32): alpha_bar to 15 e32, the ratio of two to 31 e32; u^2 + 1, the division and the subtraction add
    one e32 each: 34 e32 per step, k = M - j steps before entry j.  u = sqrt(w - 1) turns w's relative error into w / (2 u^2) of it relative
    to u, plus the root's and the subtraction's own 2 e32.  Widened by 1 % for the second-order terms."""
    e32 = 2.0 ** -24
    j = np.arange(M + 1, dtype=np.float64)
    ab = np.sin(0.5 * np.pi * j / M / (C_2 + 1)) ** 2
    u = np.zeros(M + 1)
    for i in range(M, 0, -1):
        u[i - 1] = np.sqrt((u[i] ** 2 + 1) / max(ab[i - 1] / ab[i], C_1) - 1)
    k = M - j
    with np.errstate(divide='ignore', invalid='ignore'):
        bound = np.where(u > 0, 1.01 * u * ((1 + u * u) * 34 * k * e32 / (2 * u * u) + 2 * e32), 0.0)
    return u, bound


def vp_range_f64(beta_d=19.9, beta_min=0.1, epsilon_t=1e-5):
    """((sigma_min, sigma_max), (bound, bound)): sigma(t) = sqrt(exp(z) - 1), z = beta_d t^2 / 2 + beta_min t (networks.py:511-513) in float64,
    and how far a float32 evaluation may lie from it: z is three float32 operations (3 |z| e32, which the exponential turns into that much
    relative error) and expf 3 ulp (6 e32), so exp(z) (3 |z| + 6) e32 absolute on sigma^2, plus e32 sigma^2 for the subtraction; the root
    divides by 2 sigma and adds its own 3 ulp.  At t = epsilon_t, exp(z) - 1 is eight ulps of 1: sigma_min is only known to ~20 % in float32,
    and an exponential that rounds the other way on another CPU moves it by 6 %."""
    e32 = 2.0 ** -24
    out, bounds = [], []
    for t in (epsilon_t, 1.0):
        z = 0.5 * beta_d * t * t + beta_min * t
        s2 = np.expm1(z)
        s = np.sqrt(s2)
        b2 = np.exp(z) * (3 * abs(z) + 6) * e32 + e32 * s2
        out.append(float(s))
        bounds.append(float(1.01 * (b2 / (2 * s) + 6 * e32 * s)))
    return tuple(out), tuple(bounds)


def tiny_weights(man, kind):
    """(cfg, state dict under the weight rule) of a tiny network; the checksum is the one recorded for the weights the reference module carried"""
    cfg = tiny_cfg(man, kind)
    sd, _ = dinit.refill_degenerate(with_golden_table(dinit.edm_state_dict(cfg, man['net_seed'])), man['net_seed'])
    ck, ref = dinit.checksum(sd), man[kind]['checksum']
    assert ck['numel'] == ref['numel'] and close(ck['sum'], ref['sum']) and close(ck['abs_sum'], ref['abs_sum']), (kind, ck, ref)
    return cfg, sd


def precond_pickle(cfg, sd, drop=(), top_override=None, **kwargs_override):
    """Bytes with the layout of an NVIDIA EDM network pickle (nested `torch_utils.persistence._reconstruct_persistent_obj(meta)` calls whose
    `state` is a torch.nn.Module `__dict__`) for the preconditioner class of cfg.precond over the denoiser cfg describes.  The wrapper's
    `__dict__` holds what that class's constructor records, minus the names in `drop`, updated by `top_override`; the denoiser's recorded
    constructor arguments are `cfg`'s, overridden by `kwargs_override`.  `u`, `*.resample_filter` and `*.freqs` entries of `sd` become buffers
    (`u` on the wrapper itself), everything else parameters.  `module_src` holds a placeholder: no reference text."""

    def _reconstruct_persistent_obj(meta):          # never called: only its qualified name is pickled
        raise RuntimeError

    mod = types.ModuleType('torch_utils.persistence')
    _reconstruct_persistent_obj.__module__ = 'torch_utils.persistence'
    _reconstruct_persistent_obj.__qualname__ = '_reconstruct_persistent_obj'
    mod._reconstruct_persistent_obj = _reconstruct_persistent_obj
    pkg = types.ModuleType('torch_utils')
    pkg.persistence = mod

    class Obj:
        def __init__(self, class_name, **attrs):
            self.class_name = class_name
            self.state = dict(training=False, _parameters=collections.OrderedDict(), _buffers=collections.OrderedDict(),
                              _non_persistent_buffers_set=set(), _modules=collections.OrderedDict(), **attrs)

        def __reduce__(self):
            meta = dict(type='class', version=6, module_src='# (source text omitted in the synthetic fixture)',
                        class_name=self.class_name, state=self.state)
            return (_reconstruct_persistent_obj, (meta,))

    adm = cfg.arch == 'adm'
    init_kwargs = dict(img_resolution=cfg.img_resolution, in_channels=cfg.img_channels, out_channels=cfg.out_channels,
                       label_dim=cfg.label_dim, model_channels=cfg.model_channels, channel_mult=list(cfg.channel_mult),
                       num_blocks=cfg.num_blocks, attn_resolutions=list(cfg.attn_resolutions), augment_dim=cfg.augment_dim)
    if not adm:
        init_kwargs.update(embedding_type=cfg.embedding_type, encoder_type=cfg.encoder_type, decoder_type='standard',
                           channel_mult_noise=cfg.channel_mult_noise, resample_filter=list(cfg.resample_filter), dropout=0.13)
    init_kwargs.update(kwargs_override)
    attrs = dict(img_resolution=cfg.img_resolution, img_channels=cfg.img_channels, label_dim=cfg.label_dim, use_fp16=cfg.use_fp16)
    attrs.update({k: getattr(cfg, k) for k in RECORDED[cfg.precond]})
    attrs.update(top_override or {})
    for k in drop:
        del attrs[k]
    top = Obj(CLASS_NAMES[cfg.precond], _init_args=(), _init_kwargs=None, **attrs)
    model = Obj('DhariwalUNet' if adm else 'SongUNet', _init_args=(), _init_kwargs=init_kwargs)
    top.state['_modules']['model'] = model
    for key, value in sd.items():
        parts = key.split('.')
        if parts == ['u']:
            top.state['_buffers']['u'] = value.clone()
            continue
        assert parts[0] == 'model'
        node = model
        for name in parts[1:-1]:
            node = node.state['_modules'].setdefault(name, Obj('Module'))
        if parts[-1] in ('resample_filter', 'freqs'):
            node.state['_buffers'][parts[-1]] = value.clone()
        else:
            node.state['_parameters'][parts[-1]] = torch.nn.Parameter(value.clone(), requires_grad=False)
    saved = {k: sys.modules.get(k) for k in ('torch_utils', 'torch_utils.persistence')}
    sys.modules['torch_utils'], sys.modules['torch_utils.persistence'] = pkg, mod
    try:
        return pickle.dumps(dict(ema=top))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
