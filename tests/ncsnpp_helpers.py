"""Test plumbing of the NCSN++ denoisers: the golden files of tests/golden/make_golden_ncsnpp.py, the preset weights pinned by their
checksums, and a synthetic EDM network pickle that records the SongUNet constructor arguments and buffers of choice."""
import collections
import json
import os
import pickle
import sys
import types

import numpy as np
import torch

from diffusion_tts_amd import init as dinit
from diffusion_tts_amd.config import ncsnpp_cifar10, ncsnpp_ffhq64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PRESETS = {'ncsnpp_cifar10': ncsnpp_cifar10, 'ncsnpp_ffhq64': ncsnpp_ffhq64}


def golden():
    return np.load(os.path.join(GOLDEN, 'ncsnpp_golden.npz'))


def manifest():
    with open(os.path.join(GOLDEN, 'ncsnpp_manifest.json')) as f:
        return json.load(f)


def close(a, b, rel=1e-9):
    return abs(a - b) <= rel * max(1.0, abs(b))


def preset_weights(man, name):
    """(cfg, state dict under the weight rule) of a preset; the checksum is the one recorded for the weights the reference module carried"""
    cfg = PRESETS[name]()
    sd, _ = dinit.refill_degenerate(dinit.edm_state_dict(cfg, man['net_seed']), man['net_seed'])
    ck, ref = dinit.checksum(sd), man[name]['checksum']
    assert ck['numel'] == ref['numel'] and close(ck['sum'], ref['sum']) and close(ck['abs_sum'], ref['abs_sum']), (name, ck, ref)
    return cfg, sd


def song_pickle(cfg, sd, **kwargs_override):
    """Bytes with the layout of an NVIDIA EDM network pickle (nested `torch_utils.persistence._reconstruct_persistent_obj(meta)` calls whose
    `state` is a torch.nn.Module `__dict__`) for a SongUNet under EDMPrecond: the recorded constructor arguments are `cfg`'s, overridden by
    `kwargs_override`; `*.resample_filter` and `*.freqs` entries of `sd` become buffers, everything else parameters.  `module_src` holds a
    placeholder: no reference text."""

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

    init_kwargs = dict(img_resolution=cfg.img_resolution, in_channels=cfg.img_channels, out_channels=cfg.img_channels,
                       label_dim=cfg.label_dim, model_channels=cfg.model_channels, channel_mult=list(cfg.channel_mult),
                       num_blocks=cfg.num_blocks, attn_resolutions=list(cfg.attn_resolutions), augment_dim=cfg.augment_dim,
                       embedding_type=cfg.embedding_type, encoder_type=cfg.encoder_type, decoder_type='standard',
                       channel_mult_noise=cfg.channel_mult_noise, resample_filter=list(cfg.resample_filter), dropout=0.13)
    init_kwargs.update(kwargs_override)
    top = Obj('EDMPrecond', img_resolution=cfg.img_resolution, img_channels=cfg.img_channels, label_dim=cfg.label_dim, use_fp16=False,
              sigma_min=cfg.sigma_min, sigma_max=cfg.sigma_max, sigma_data=cfg.sigma_data, _init_args=(), _init_kwargs=None)
    model = Obj('SongUNet', _init_args=(), _init_kwargs=init_kwargs)
    top.state['_modules']['model'] = model
    for key, value in sd.items():
        parts = key.split('.')
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
