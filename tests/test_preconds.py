"""VP, VE and iDDPM preconditioners, host side: configuration, the initialiser against the reference constructors' record
(tests/golden/make_golden_preconds.py), checkpoint ingestion of the three classes and its refusals, bundles and presets.  No GPU."""
import dataclasses
import inspect

import numpy as np
import pytest
import torch

import precond_helpers as ph
from diffusion_tts_amd import init as dinit
from diffusion_tts_amd.checkpoint import load_edm_pickle
from diffusion_tts_amd.config import (EDMConfig, adm_imagenet64, ddpmpp_cifar10, iddpm_imagenet64, ncsnpp_cifar10, ve_cifar10,
                                      vp_cifar10)

KINDS = ph.KINDS


@pytest.fixture(scope='module')
def man():
    return ph.manifest()


def test_new_fields_default_to_the_edm_wrapper():
    """every config written before these fields existed equals itself"""
    assert adm_imagenet64() == EDMConfig('adm', 64, 3, 1000, 192, [1, 2, 3, 4], 4, 3, [32, 16, 8], 0)
    assert ddpmpp_cifar10() == EDMConfig('ddpmpp', 32, 3, 10, 128, [2, 2, 2], 4, 4, [16], 9)
    c = EDMConfig()
    assert (c.precond, c.beta_d, c.beta_min, c.M, c.epsilon_t, c.C_1, c.C_2, c.use_fp16) == ('edm', 19.9, 0.1, 1000, 1e-5, 0.001, 0.008, False)
    assert c.out_channels == 3 and dataclasses.replace(c, precond='iddpm').out_channels == 6 and dataclasses.replace(c, precond='vp').out_channels == 3


def test_presets(man):
    vp, ve, idd = vp_cifar10(), ve_cifar10(), iddpm_imagenet64()
    assert (vp.precond, vp.arch, vp.fir) == ('vp', 'ddpmpp', False) and dataclasses.replace(vp, precond='edm', sigma_min=0.0, sigma_max=float('inf')) == ddpmpp_cifar10()
    assert (ve.precond, ve.arch, ve.fir) == ('ve', 'ddpmpp', True) and dataclasses.replace(ve, precond='edm', sigma_min=0.0, sigma_max=float('inf')) == ncsnpp_cifar10()
    assert (idd.precond, idd.arch, idd.out_channels) == ('iddpm', 'adm', 6)
    assert (ve.sigma_min, ve.sigma_max) == (0.02, 100) == (man['ve_cifar10']['sigma_min'], man['ve_cifar10']['sigma_max'])
    # VP and iDDPM compute their range through float32 exp / sin, which CPUs do not all round alike: this machine's value and the one the
    # golden script checked against the reference constructor are each held to the float64 value by the derived bound
    (lo, hi), (blo, bhi) = ph.vp_range_f64()
    for got, rec, want, b in ((vp.sigma_min, man['vp_cifar10']['sigma_min'], lo, blo), (vp.sigma_max, man['vp_cifar10']['sigma_max'], hi, bhi)):
        assert abs(got - want) <= b and abs(rec - want) <= b, (got, rec, want, b)
    assert bhi < 1e-5 * hi and blo < 0.25 * lo
    u64, bound = ph.iddpm_table_f64()                      # iDDPM: the table's ends, to the bound of a float32 evaluation of it
    for got, rec, j in ((idd.sigma_min, man['iddpm_imagenet64']['sigma_min'], 999), (idd.sigma_max, man['iddpm_imagenet64']['sigma_max'], 0)):
        assert abs(got - u64[j]) <= bound[j] and abs(rec - u64[j]) <= bound[j], (j, got, rec, u64[j], bound[j])
    from diffusion_tts_amd import sampler
    src = inspect.getsource(sampler.load_network)
    assert all(n in src for n in ('vp_cifar10', 've_cifar10', 'iddpm_imagenet64'))


def test_iddpm_table_is_the_constructors():
    """the golden script asserts bit equality with the reference constructor where both run; a float32 sine is not the same on every CPU, so
    here the initialiser's table and the recorded one are each held to the float64 recursion by the derived bound"""
    u = dinit.iddpm_u()
    g = ph.golden()['iddpm_u']
    u64, bound = ph.iddpm_table_f64()
    assert u.dtype == torch.float32 and g.dtype == np.float32
    for name, t in (('initialiser', u.numpy()), ('golden', g)):
        ex = np.abs(t.astype(np.float64) - u64) - bound
        print(f'{name}: largest excess over the bound {ex.max():.3e}; largest |u - u64| / u64 {np.max(np.abs(t[:-1] - u64[:-1]) / u64[:-1]):.3e}')
        assert ex.max() <= 0
    assert bound[999] < 0.05 * u64[999] and bound[0] < 0.01 * u64[0]      # and the bound still tells one entry from the next
    assert u.numel() == 1001 and float(u[1000]) == 0.0 and bool((u[1:] < u[:-1]).all())
    assert (float(u[999]), float(u[0])) == (iddpm_imagenet64().sigma_min, iddpm_imagenet64().sigma_max)
    assert dinit.iddpm_u(M=50).numel() == 51


@pytest.mark.parametrize('kind', KINDS)
def test_initialiser_reproduces_the_reference_constructor_record(kind, man):
    """keys (state_dict() order: iDDPM's `u` first, then the denoiser) and checksums the golden generator read off the reference module"""
    cfg = ph.tiny_cfg(man, kind)
    assert cfg.precond == kind
    sd = ph.with_golden_table(dinit.edm_state_dict(cfg, man['net_seed']))
    rec = man[kind]
    assert list(sd.keys()) == rec['keys']
    for want in (rec['checksum_reference_raw'], rec['checksum_raw']):
        got = dinit.checksum(sd)
        assert got['numel'] == want['numel'] and ph.close(got['sum'], want['sum']) and ph.close(got['abs_sum'], want['abs_sum'])
    ph.tiny_weights(man, kind)                             # and under the weight rule
    if kind == 'iddpm':
        assert list(sd)[0] == 'u' and sd['model.out_conv.weight'].shape[0] == 6 and sd['model.out_conv.bias'].shape[0] == 6
    else:
        assert 'u' not in sd


# (iddpm_imagenet64 is 296 M values: its 6-channel draw and table are covered by the tiny network above, its range by test_presets)
@pytest.mark.parametrize('name', ['vp_cifar10', 've_cifar10'])
def test_fullsize_preset_initialiser_checksums(name, man):
    import diffusion_tts_amd.config as C
    sd = dinit.edm_state_dict(getattr(C, name)(), man['net_seed'])
    got, want = dinit.checksum(sd), man[name]['checksum_raw']
    assert got['numel'] == want['numel'] and ph.close(got['sum'], want['sum']) and ph.close(got['abs_sum'], want['abs_sum'])


@pytest.mark.parametrize('kind', KINDS)
def test_reader_round_trip(kind, man):
    cfg, sd = ph.tiny_weights(man, kind)
    got_cfg, got = load_edm_pickle(ph.precond_pickle(cfg, sd))
    assert got_cfg == cfg and got_cfg.precond == kind
    assert (got_cfg.sigma_min, got_cfg.sigma_max) == (cfg.sigma_min, cfg.sigma_max)
    assert list(got.keys()) == list(sd.keys()) and all(torch.equal(got[k], sd[k]) for k in sd)
    if kind == 'iddpm':
        assert 'u' in got and 'model.u' not in got and got['model.out_conv.weight'].shape[0] == 6


def test_reader_takes_scalars_and_range_from_the_file(man):
    cfg, sd = ph.tiny_weights(man, 'vp')
    c2 = dataclasses.replace(cfg, beta_d=15.0, beta_min=0.2, M=500, epsilon_t=1e-3, sigma_min=0.01, sigma_max=33.0, use_fp16=True)
    got, _ = load_edm_pickle(ph.precond_pickle(c2, sd))
    assert got == c2 and got.use_fp16 is True and got.M == 500
    cfg, sd = ph.tiny_weights(man, 'iddpm')
    u = dinit.iddpm_u(M=20, C_1=0.002, C_2=0.01)
    sd2 = dict(sd, u=u)
    c2 = dataclasses.replace(cfg, M=20, C_1=0.002, C_2=0.01, sigma_min=float(u[19]), sigma_max=float(u[0]))
    got, gsd = load_edm_pickle(ph.precond_pickle(c2, sd2))
    assert got == c2 and torch.equal(gsd['u'], u)
    # EDMPrecond files read as before
    cfg = EDMConfig('adm', 16, 3, 10, 64, [1, 2], 4, 1, [8], 0)
    sd = dinit.edm_state_dict(cfg, 0)
    got, gsd = load_edm_pickle(ph.precond_pickle(cfg, sd))
    assert got == cfg and got.precond == 'edm' and list(gsd) == list(sd)


@pytest.mark.parametrize('kind,attr', [('vp', 'beta_d'), ('vp', 'beta_min'), ('vp', 'M'), ('vp', 'sigma_min'), ('ve', 'sigma_max'),
                                       ('iddpm', 'M'), ('iddpm', 'sigma_min')])
def test_reader_refuses_a_state_without_an_attribute_the_forward_reads(kind, attr, man):
    cfg, sd = ph.tiny_weights(man, kind)
    with pytest.raises(NotImplementedError, match=attr):
        load_edm_pickle(ph.precond_pickle(cfg, sd, drop=(attr,)))


def test_reader_refuses_bad_iddpm_files(man):
    cfg, sd = ph.tiny_weights(man, 'iddpm')
    no_u = {k: v for k, v in sd.items() if k != 'u'}
    with pytest.raises(NotImplementedError, match="'u'"):
        load_edm_pickle(ph.precond_pickle(cfg, no_u))
    u = sd['u']
    for bad in (u[:-1], torch.cat([u[:500], u[499:]]).contiguous()[:1001], torch.cat([u[:1000], u[999:1000] * 0.5])):
        with pytest.raises(ValueError):
            load_edm_pickle(ph.precond_pickle(cfg, dict(sd, u=bad.clone())))
    with pytest.raises(NotImplementedError, match='out_channels'):
        load_edm_pickle(ph.precond_pickle(cfg, sd, out_channels=3))
    with pytest.raises(NotImplementedError):
        load_edm_pickle(ph.precond_pickle(dataclasses.replace(cfg, precond='edm'), sd).replace(b'EDMPrecond', b'FooPrecond'))


def test_bundle_carries_the_preconditioner(man, tmp_path):
    """a .pt bundle is {'cfg': EDMConfig kwargs, 'state_dict': ...}: precond and its scalars ride in the kwargs, `u` in the state dict"""
    cfg, sd = ph.tiny_weights(man, 'iddpm')
    p = tmp_path / 'net.pt'
    torch.save(dict(cfg=dataclasses.asdict(cfg), state_dict=sd), p)
    blob = torch.load(p, map_location='cpu')
    back = EDMConfig(**blob['cfg'])
    assert back == cfg and back.precond == 'iddpm' and torch.equal(blob['state_dict']['u'], sd['u'])


def test_cli_takes_dtype_auto_and_keeps_its_default():
    import main
    p = main.build_parser()
    base = ['--backend', 'edm', '--scorer', 'brightness']
    assert p.parse_args(base).dtype == 'f16x3'
    assert p.parse_args(base + ['--dtype', 'auto', '--network', 'random:iddpm_imagenet64']).dtype == 'auto'
