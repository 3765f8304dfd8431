"""NCSN++ denoisers (SongUNet with the Fourier embedding, the residual encoder and the [1,3,3,1] resampling filter: the network of the published
`*-ve.pkl` EDM checkpoints), host side: configuration, the initialiser against the reference constructor's record, checkpoint ingestion, and
the weight composition behind the one-launch `aux_residual` convolution.  No GPU."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

import ncsnpp_helpers as nh
from diffusion_tts_amd import init as dinit
from diffusion_tts_amd.checkpoint import load_edm_pickle
from diffusion_tts_amd.config import EDMConfig, ddpmpp_cifar10, edm_blocks, ncsnpp_cifar10, ncsnpp_ffhq64

TINY = EDMConfig('ddpmpp', 16, 3, 10, 64, [1, 2], 4, 1, [8], 9, embedding_type='fourier', channel_mult_noise=2, encoder_type='residual',
                 resample_filter=[1, 3, 3, 1])


def test_new_options_default_to_the_ddpmpp_values():
    assert ddpmpp_cifar10() == EDMConfig('ddpmpp', 32, 3, 10, 128, [2, 2, 2], 4, 4, [16], 9)
    c = ddpmpp_cifar10()
    assert (c.embedding_type, c.channel_mult_noise, c.encoder_type, c.resample_filter) == ('positional', 1, 'standard', [1, 1])
    assert not c.fir and c.noise_channels == 128 and ncsnpp_cifar10().fir and ncsnpp_cifar10().noise_channels == 256
    assert all(b.kind != 'aux_residual' for b in edm_blocks(c)[0])


def test_aux_residual_blocks_follow_the_constructor_order():
    enc, dec, cfin = edm_blocks(ncsnpp_cifar10())
    aux = [(b.name, b.cin, b.cout, b.res_in, b.res_out) for b in enc if b.kind == 'aux_residual']
    assert aux == [('enc.16x16_aux_residual', 3, 256, 32, 16), ('enc.8x8_aux_residual', 256, 256, 16, 8)]
    names = [b.name for b in enc]
    assert names.index('enc.16x16_aux_residual') == names.index('enc.16x16_down') + 1
    enc, _, _ = edm_blocks(ncsnpp_ffhq64())
    assert [(b.cin, b.cout) for b in enc if b.kind == 'aux_residual'] == [(3, 128), (128, 256), (256, 256)]


@pytest.mark.parametrize('name', ['ncsnpp_cifar10', 'ncsnpp_ffhq64'])
def test_initialiser_reproduces_the_reference_constructor_record(name):
    """keys (parameters and buffers, state_dict() order) and checksums the golden generator read off the reference module"""
    man = nh.manifest()
    sd = dinit.edm_state_dict(nh.PRESETS[name](), man['net_seed'])
    rec = man[name]
    assert list(sd.keys()) == rec['keys']
    assert 'model.map_noise.freqs' in sd and sd['model.map_noise.freqs'].numel() == 128
    assert any(k.endswith('_aux_residual.weight') for k in sd) and any(k.endswith('conv0.resample_filter') for k in sd)
    for got, want in ((dinit.checksum(sd), rec['checksum_reference_raw']), (dinit.checksum(sd), rec['checksum_raw'])):
        assert got['numel'] == want['numel'] and nh.close(got['sum'], want['sum']) and nh.close(got['abs_sum'], want['abs_sum'])
    nh.preset_weights(man, name)                           # and under the weight rule


def test_reader_returns_the_ncsnpp_config_and_every_key():
    sd, _ = dinit.refill_degenerate(dinit.edm_state_dict(TINY, 0), 0)
    cfg, got = load_edm_pickle(nh.song_pickle(TINY, sd))
    assert cfg == TINY and cfg.fir and cfg.embedding_type == 'fourier' and cfg.encoder_type == 'residual' and cfg.channel_mult_noise == 2
    assert list(got.keys()) == list(sd.keys())
    for k in ('model.map_noise.freqs', 'model.enc.8x8_aux_residual.weight', 'model.enc.8x8_aux_residual.bias',
              'model.enc.8x8_aux_residual.resample_filter', 'model.enc.8x8_down.conv0.resample_filter', 'model.dec.16x16_up.skip.resample_filter'):
        assert k in got, k
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    assert got['model.map_layer0.weight'].shape[1] == 128 and got['model.map_label.weight'].shape[0] == 128


def test_reader_still_refuses_what_is_not_implemented():
    sd = dinit.edm_state_dict(TINY, 0)
    for bad in (dict(encoder_type='skip'), dict(decoder_type='skip'), dict(resample_filter=[1, 2, 1]), dict(embedding_type='other')):
        with pytest.raises(NotImplementedError):
            load_edm_pickle(nh.song_pickle(TINY, sd, **bad))
    # constructor arguments and filter buffers that disagree, both ways round
    with pytest.raises(NotImplementedError):
        load_edm_pickle(nh.song_pickle(TINY, sd, resample_filter=[1, 1]))
    wrong = dict(sd)
    wrong['model.enc.8x8_down.skip.resample_filter'] = dinit.resample_filter_2d([1, 1])
    with pytest.raises(NotImplementedError):
        load_edm_pickle(nh.song_pickle(TINY, wrong))
    no_freqs = {k: v for k, v in sd.items() if k != 'model.map_noise.freqs'}
    with pytest.raises(ValueError):
        load_edm_pickle(nh.song_pickle(TINY, no_freqs))


def _s2d(x):
    n, c, h, w = x.shape
    return x.view(n, c, h // 2, 2, w // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(n, 4 * c, h // 2, w // 2)


@pytest.mark.parametrize('cin,cout,h,w', [(3, 8, 8, 8), (3, 256, 32, 32), (5, 7, 6, 10), (17, 9, 4, 4), (16, 4, 10, 6)])
def test_fused_down_weight_is_the_two_step_convolution(cin, cout, h, w):
    """conv2d(x, w, padding 2) followed by the depthwise [1,3,3,1] filter at stride 2 == ONE 3x3 padding-1 convolution of space_to_depth(x) with
    the composed weight, in float64 to 1e-12 (odd channel counts and the 3-channel image included; zero-padded channels change nothing)"""
    from diffusion_tts_amd import ops
    g = torch.Generator().manual_seed(cin * 100 + cout)
    x = torch.randn(2, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    f2 = dinit.resample_filter_2d([1, 3, 3, 1]).double()
    want = F.conv2d(F.conv2d(x, wt, padding=2), f2.tile([cout, 1, 1, 1]), stride=2, groups=cout)
    w3 = ops.fused_down_weight(wt, out_dtype=torch.float64)
    assert w3.shape == (cout, 4 * cin, 3, 3)
    got = F.conv2d(_s2d(x), w3, padding=1)
    assert got.shape == want.shape and float((got - want).abs().max()) < 1e-12
    cpad = 4 * cin + 20
    wp = ops.fused_down_weight(wt, cpad=cpad, out_dtype=torch.float64)
    xp = torch.cat([_s2d(x), torch.randn(2, 20, h // 2, w // 2, generator=g, dtype=torch.float64)], 1)
    assert wp.shape[1] == cpad and float((F.conv2d(xp, wp, padding=1) - want).abs().max()) < 1e-12
    assert ops.fused_down_weight(wt.float()).dtype == torch.float32


def test_fir_formulas_of_the_kernel_documentation():
    """the per-axis weights the device pass uses, against conv2d / conv_transpose2d with the reference's filter buffer (float64)"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 1, 6, 6, generator=g, dtype=torch.float64)
    f2 = dinit.resample_filter_2d([1, 3, 3, 1]).double()
    up = F.conv_transpose2d(x, f2 * 4, stride=2, padding=1)
    xp = F.pad(x, (1, 1, 1, 1))
    ax = lambda t, d: torch.stack([0.75 * t.narrow(d, 1, 6) + 0.25 * t.narrow(d, 0, 6), 0.75 * t.narrow(d, 1, 6) + 0.25 * t.narrow(d, 2, 6)], d + 1)
    rows = ax(xp, 2).reshape(1, 1, 12, 8)
    mine = ax(rows, 3).reshape(1, 1, 12, 12)
    assert float((mine - up).abs().max()) < 1e-14
    k = torch.tensor([0.125, 0.375, 0.375, 0.125], dtype=torch.float64)
    assert float((torch.outer(k, k) - f2[0, 0]).abs().max()) == 0.0


def test_random_presets_are_named_by_the_loader():
    import inspect
    from diffusion_tts_amd import sampler
    src = inspect.getsource(sampler.load_network)
    assert 'ncsnpp_cifar10' in src and 'ncsnpp_ffhq64' in src
    assert dataclasses.asdict(ncsnpp_ffhq64())['channel_mult'] == [1, 2, 2, 2] and ncsnpp_ffhq64().label_dim == 0
