"""CPU: the host-side pieces of the SD U-Net on the HIP kernels (diffusion_tts_amd/sd_unet.py) that need no GPU -- the seeded initialiser's
keys and shapes against the reference module's own state dict (recorded by tests/golden/make_golden_sd_unet.py), the two exact weight
transforms (zero-padded heads; the stride-2 convolution over space-to-depth) in float64, and the refusal of non-stock configurations."""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT


@pytest.fixture(scope='module')
def manifest():
    with open(os.path.join(ROOT, 'tests', 'golden', 'sd_unet_manifest.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('name', ['narrow', 'sd15'])
def test_initialiser_has_the_reference_state_dict_keys_and_shapes(manifest, name):
    from diffusion_tts_amd import init as dinit
    c = manifest['cases'][name]
    if name == 'sd15':      # shapes only: 860 M parameters need not be drawn to know them
        sd = _shapes_only(dinit, c)
    else:
        sd = {k: tuple(v.shape) for k, v in dinit.sd_unet_state_dict(tuple(c['block_out_channels']), c['heads'], c['cross_attention_dim'], 2,
                                                                     seed=c['seed']).items()}
    want = {k: tuple(s) for k, s in c['state_dict']}
    assert len(want) == 686 and sd == want, (sorted(set(sd) ^ set(want))[:6], [k for k in sd if k in want and sd[k] != want[k]][:6])


def _shapes_only(dinit, c):
    """sd_unet_state_dict with the random draws replaced by empty meta tensors"""
    real_randn = torch.randn
    try:
        torch.randn = lambda *shape, generator=None, **kw: torch.empty(*shape, device='meta')
        sd = dinit.sd_unet_state_dict(tuple(c['block_out_channels']), c['heads'], c['cross_attention_dim'], 2, seed=c['seed'])
    finally:
        torch.randn = real_randn
    return {k: tuple(v.shape) for k, v in sd.items()}


def test_initialiser_is_seeded(manifest):
    from diffusion_tts_amd import init as dinit
    c = manifest['cases']['narrow']
    args = (tuple(c['block_out_channels']), c['heads'], c['cross_attention_dim'], 2)
    a, b, other = dinit.sd_unet_state_dict(*args, seed=c['seed']), dinit.sd_unet_state_dict(*args, seed=c['seed']), dinit.sd_unet_state_dict(*args, seed=c['seed'] + 1)
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a['conv_in.weight'], other['conv_in.weight'])
    got, want = dinit.checksum(a), c['checksum']                       # the parameters the golden outputs were computed with
    assert got['numel'] == want['numel'] and abs(got['abs_sum'] - want['abs_sum']) <= 1e-9 * want['abs_sum']


def test_zero_padded_heads_leave_the_attention_unchanged():
    """SD-1.5's head dim 40 on a kernel that takes 64: rows of to_q / to_k / to_v and columns of to_out.0 zero-padded per head, softmax
    scale 1/sqrt(40) of the TRUE dim.  Exact: float64, 1e-12."""
    from diffusion_tts_amd.sd_unet import pad_head_rows, pad_head_cols, padded_head_dim
    g = torch.Generator().manual_seed(0)
    heads, d, cin, n, tq, tk = 8, 40, 320, 2, 9, 7
    dp = padded_head_dim(d)
    assert dp == 64 and padded_head_dim(64) == 64 and padded_head_dim(80) == 128 and padded_head_dim(160) == 256
    with pytest.raises(ValueError):
        padded_head_dim(257)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    wq, wk, wv, wo = rnd(heads * d, cin) / 18, rnd(heads * d, cin) / 18, rnd(heads * d, cin) / 18, rnd(cin, heads * d) / 18
    x, ctx = rnd(n, tq, cin), rnd(n, tk, cin)

    def attend(wq, wk, wv, wo, dh):
        q = (x @ wq.T).view(n, tq, heads, dh).transpose(1, 2)
        k = (ctx @ wk.T).view(n, tk, heads, dh).transpose(1, 2)
        v = (ctx @ wv.T).view(n, tk, heads, dh).transpose(1, 2)
        w = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), -1)
        return (w @ v).transpose(1, 2).reshape(n, tq, heads * dh) @ wo.T

    want = attend(wq, wk, wv, wo, d)
    got = attend(pad_head_rows(wq, heads, dp), pad_head_rows(wk, heads, dp), pad_head_rows(wv, heads, dp), pad_head_cols(wo, heads, dp), dp)
    assert tuple(pad_head_rows(wq, heads, dp).shape) == (heads * dp, cin) and tuple(pad_head_cols(wo, heads, dp).shape) == (cin, heads * dp)
    assert float((got - want).abs().max()) < 1e-12


def space_to_depth2_torch(x):
    """dts_space_to_depth2 restated: NCHW [n, c, h, w] -> [n, 4c, h/2, w/2], channel (ry*2 + rx)*c + ci of pixel (i, j) = x[ci, 2i+ry, 2j+rx]"""
    n, c, h, w = x.shape
    return x.view(n, c, h // 2, 2, w // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(n, 4 * c, h // 2, w // 2)


@pytest.mark.parametrize('cpad', [None, 64])
def test_stride2_convolution_as_a_stride1_convolution_over_space_to_depth(cpad):
    """Downsample2D's Conv2d(3, stride 2, padding 1) == conv2d(space_to_depth2(x), stride2_conv_weight(w), padding 1), in float64; only the
    block taps at offsets {-1, 0} are live."""
    from diffusion_tts_amd import ops
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 12, 10, 6, generator=g, dtype=torch.float64)
    w, b = torch.randn(5, 12, 3, 3, generator=g, dtype=torch.float64), torch.randn(5, generator=g, dtype=torch.float64)
    w3 = ops.stride2_conv_weight(w, cpad=cpad)
    assert tuple(w3.shape) == (5, cpad or 48, 3, 3) and not w3[:, :, 2, :].any() and not w3[:, :, :, 2].any() and not w3[:, 48:].any()
    assert int((w3 != 0).sum()) == w.numel()                              # a rearrangement: every source tap lands exactly once
    xs = space_to_depth2_torch(x)
    if cpad:
        xs = torch.cat([xs, torch.zeros(2, cpad - 48, 5, 3, dtype=torch.float64)], 1)
    want = F.conv2d(x, w, b, stride=2, padding=1)
    got = F.conv2d(xs, w3, b, stride=1, padding=1)
    assert got.shape == want.shape and float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize('key,value', [('use_linear_projection', True), ('act_fn', 'gelu'), ('norm_num_groups', 16), ('resnet_time_scale_shift', 'scale_shift'),
                                       ('addition_embed_type', 'text_time'), ('class_embed_type', 'timestep'), ('transformer_layers_per_block', 2),
                                       ('down_block_types', ['DownBlock2D'] * 4), ('mid_block_type', 'UNetMidBlock2D'), ('flip_sin_to_cos', False),
                                       ('freq_shift', 1), ('up_block_types', ['UpBlock2D'] * 4), ('attention_head_dim', [5, 10, 20, 20]),
                                       ('block_out_channels', [320, 640, 1280]), ('_class_name', 'UNet2DModel'), ('norm_eps', 1e-6)])
def test_unsupported_configurations_are_refused_by_name(tmp_path, key, value):
    from diffusion_tts_amd.sd_unet import SDUNet, check_config
    stock = {'_class_name': 'UNet2DConditionModel', 'act_fn': 'silu', 'attention_head_dim': 8, 'block_out_channels': [320, 640, 1280, 1280],
             'cross_attention_dim': 768, 'layers_per_block': 2, 'norm_num_groups': 32, 'norm_eps': 1e-5, 'sample_size': 64, 'in_channels': 4,
             'down_block_types': ['CrossAttnDownBlock2D'] * 3 + ['DownBlock2D'], 'up_block_types': ['UpBlock2D'] + ['CrossAttnUpBlock2D'] * 3,
             'flip_sin_to_cos': True, 'freq_shift': 0, 'center_input_sample': False, 'downsample_padding': 1, 'mid_block_scale_factor': 1,
             'out_channels': 4}
    check_config(stock)                                                    # SD-1.5's own unet/config.json passes
    bad = dict(stock, **{key: value})
    with pytest.raises(ValueError, match=key):
        check_config(bad)
    d = tmp_path / 'unet'
    d.mkdir()
    (d / 'config.json').write_text(json.dumps(bad))
    with pytest.raises(ValueError, match=key):                             # before any tensor is read
        SDUNet.from_pretrained(str(d))


def test_a_pickle_only_directory_is_not_read_and_a_missing_config_is_not_guessed(tmp_path):
    from diffusion_tts_amd.sd_unet import SDUNet
    d = tmp_path / 'unet'
    d.mkdir()
    (d / 'diffusion_pytorch_model.bin').write_bytes(b'x')
    with pytest.raises(FileNotFoundError, match='config.json'):            # no configuration: SD-1.5's is not assumed
        SDUNet.from_pretrained(str(d))
    (d / 'config.json').write_text(json.dumps({'_class_name': 'UNet2DConditionModel', 'block_out_channels': [320, 640, 1280, 1280]}))
    with pytest.raises(FileNotFoundError, match='safetensors'):
        SDUNet.from_pretrained(str(d))


def test_parameters_that_do_not_fit_the_configuration_are_refused_by_name():
    """host logic only: the shape check that runs before anything is packed for the device"""
    from diffusion_tts_amd import init as dinit
    from diffusion_tts_amd.sd_unet import SDUNet
    sd = dinit.sd_unet_state_dict((64, 128, 192, 192), 2, 64, 2, seed=1)

    def probe(boc=(64, 128, 192, 192), heads=2, ctx=64, lpb=2):
        u = SDUNet.__new__(SDUNet)
        u.boc, u.heads, u.ctx_dim, u.lpb = boc, heads, ctx, lpb
        u._check_shapes(sd)

    probe()
    with pytest.raises(ValueError, match='conv_in.weight'):
        probe(boc=(320, 640, 1280, 1280))
    with pytest.raises(ValueError, match='attn2.to_k.weight.*cross_attention_dim=768'):
        probe(ctx=768)
    with pytest.raises(ValueError, match='layers_per_block=1'):
        probe(lpb=1)
    with pytest.raises(ValueError, match='has no'):
        probe(lpb=3)
    with pytest.raises(ValueError, match='attention_head_dim=5'):
        probe(heads=5)


def test_cli_takes_the_hip_unet_without_diffusers_and_does_not_fall_back(tmp_path, monkeypatch):
    """`--unet hip` reads $DTS_SD_UNET_DIR through load_sd_unet; a directory that is missing is an error, not a quiet switch to diffusers."""
    import main as cli
    monkeypatch.setenv('DTS_SD_UNET_DIR', str(tmp_path / 'nowhere'))
    with pytest.raises(FileNotFoundError, match='DTS_SD_UNET_DIR'):
        cli.load_sd_unet('runwayml/stable-diffusion-v1-5', torch.device('cpu'), 'hip')
    with pytest.raises(ValueError, match='--unet'):
        cli.load_sd_unet('runwayml/stable-diffusion-v1-5', torch.device('cpu'), 'eager')
