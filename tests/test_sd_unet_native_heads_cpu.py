"""CPU: the host side of head_dims='native' of the SD U-Net (diffusion_tts_amd/sd_unet.py): which head dim a level gets, that nothing is
padded when it is the model's own, that the zero-padding stays exact where one is still needed (36 -> 40), and that a bad mode is refused by
the constructor, the loader and the command line before anything else happens."""
import math

import pytest
import torch


def test_native_head_dim():
    from diffusion_tts_amd.sd_unet import native_head_dim
    for (d, heads), want in {(40, 8): 40, (80, 8): 80, (160, 8): 160, (36, 8): 40, (41, 8): 64, (64, 2): 64, (96, 2): 128}.items():
        assert native_head_dim(d, heads) == want, (d, heads)
    assert native_head_dim(32, 2) == 64                    # 2 x 40 = 80 channels are no multiple of 64: the 1x1 convolutions need cin % 64 == 0
    assert native_head_dim(256, 1) == 256
    with pytest.raises(ValueError, match='257'):
        native_head_dim(257, 1)


def test_padded_head_dim_is_unchanged():
    from diffusion_tts_amd.sd_unet import padded_head_dim
    assert [padded_head_dim(d) for d in (1, 40, 64, 65, 80, 128, 160, 256)] == [64, 64, 64, 128, 128, 128, 256, 256]
    with pytest.raises(ValueError):
        padded_head_dim(257)


def test_nothing_is_padded_at_the_models_own_head_dim():
    from diffusion_tts_amd.sd_unet import native_head_dim, pad_head_cols, pad_head_rows
    g = torch.Generator().manual_seed(3)
    for heads, d, cin in ((8, 40, 320), (8, 80, 640), (8, 160, 1280)):
        dn = native_head_dim(d, heads)
        w, wo = torch.randn(heads * d, cin, generator=g), torch.randn(cin, heads * d, generator=g)
        assert dn == d and torch.equal(pad_head_rows(w, heads, dn), w) and torch.equal(pad_head_cols(wo, heads, dn), wo)


def test_zero_padded_heads_leave_the_attention_unchanged_at_36_in_40():
    """the identity of tests/test_sd_unet_cpu.py at a head dim the native mode still pads: 36 -> 40, scale 1/sqrt(36).  Exact: float64, 1e-12."""
    from diffusion_tts_amd.sd_unet import native_head_dim, pad_head_cols, pad_head_rows
    g = torch.Generator().manual_seed(0)
    heads, d, cin, n, tq, tk = 8, 36, 288, 2, 9, 7
    dp = native_head_dim(d, heads)
    assert dp == 40
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    wq, wk, wv, wo = rnd(heads * d, cin) / 17, rnd(heads * d, cin) / 17, rnd(heads * d, cin) / 17, rnd(cin, heads * d) / 17
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


def test_a_bad_mode_is_refused_before_anything_else(tmp_path):
    from diffusion_tts_amd.sd_unet import SDUNet
    u = SDUNet.__new__(SDUNet)
    with pytest.raises(ValueError, match="head_dims='bogus'"):             # before the GPU is asked for and before the state dict is looked at
        u.__init__({}, head_dims='bogus')
    with pytest.raises(ValueError, match="head_dims='bogus'"):             # before the directory is looked at
        SDUNet.from_pretrained(str(tmp_path / 'nowhere'), head_dims='bogus')


def test_command_line_flag():
    import main as cli
    parser = cli.build_parser()
    base = ['--backend', 'sd', '--scorer', 'brightness']
    assert parser.parse_args(base).unet_head_dims == 'padded'
    assert parser.parse_args(base + ['--unet-head-dims', 'padded']).unet_head_dims == 'padded'
    assert parser.parse_args(base + ['--unet', 'hip', '--unet-head-dims', 'native']).unet_head_dims == 'native'
    with pytest.raises(SystemExit):
        parser.parse_args(base + ['--unet-head-dims', 'bogus'])


def test_loader_refuses_a_bad_mode_before_any_file_is_touched(tmp_path, monkeypatch):
    import main as cli
    monkeypatch.setenv('DTS_SD_UNET_DIR', str(tmp_path / 'nowhere'))
    with pytest.raises(ValueError, match='--unet-head-dims'):
        cli.load_sd_unet('runwayml/stable-diffusion-v1-5', torch.device('cpu'), 'hip', head_dims='bogus')
    with pytest.raises(FileNotFoundError, match='DTS_SD_UNET_DIR'):        # a good mode reaches the directory, as the three-argument call does
        cli.load_sd_unet('runwayml/stable-diffusion-v1-5', torch.device('cpu'), 'hip', head_dims='native')
    with pytest.raises(FileNotFoundError, match='DTS_SD_UNET_DIR'):
        cli.load_sd_unet('runwayml/stable-diffusion-v1-5', torch.device('cpu'), 'hip')
