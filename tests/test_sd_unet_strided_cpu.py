"""CPU: the downsample mode of the SD U-Net (SDUNet(downsample=), main.load_sd_unet, main.py --unet-downsample) is refused by name where it
cannot hold -- before the GPU is asked for, before a file is touched, and on the command line where it is parsed."""
import pytest
import torch


def test_a_bad_mode_is_refused_before_anything_else(tmp_path):
    from diffusion_tts_amd.sd_unet import DOWNSAMPLE, SDUNet
    assert DOWNSAMPLE == ('s2d', 'strided')
    u = SDUNet.__new__(SDUNet)
    with pytest.raises(ValueError, match="downsample='bogus'"):            # before the GPU is asked for and before the state dict is looked at
        u.__init__({}, downsample='bogus')
    with pytest.raises(ValueError, match="downsample='bogus'"):            # before the directory is looked at
        SDUNet.from_pretrained(str(tmp_path / 'nowhere'), downsample='bogus')
    with pytest.raises(FileNotFoundError):                                 # a good mode reaches the directory
        SDUNet.from_pretrained(str(tmp_path / 'nowhere'), downsample='strided')


def test_command_line_flag(capsys):
    import main as cli
    parser = cli.build_parser()
    base = ['--backend', 'sd', '--scorer', 'brightness']
    assert parser.parse_args(base).unet_downsample == 's2d'
    assert parser.parse_args(base + ['--unet-downsample', 's2d']).unet_downsample == 's2d'
    assert parser.parse_args(base + ['--unet', 'hip']).unet_downsample == 's2d'
    ns = parser.parse_args(base + ['--unet', 'hip', '--unet-downsample', 'strided', '--unet-head-dims', 'native'])
    assert (ns.unet_downsample, ns.unet_head_dims) == ('strided', 'native')
    for bad in (['--unet-downsample', 'strided'], ['--unet', 'diffusers', '--unet-downsample', 'strided']):       # not without --unet hip
        with pytest.raises(SystemExit):
            parser.parse_args(base + bad)
        assert '--unet-downsample strided goes with --unet hip' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parser.parse_args(base + ['--unet', 'hip', '--unet-downsample', 'bogus'])


def test_loader_refuses_before_any_file_is_touched(tmp_path, monkeypatch):
    import main as cli
    monkeypatch.setenv('DTS_SD_UNET_DIR', str(tmp_path / 'nowhere'))
    model = 'runwayml/stable-diffusion-v1-5'
    with pytest.raises(ValueError, match='--unet-downsample'):
        cli.load_sd_unet(model, torch.device('cpu'), 'hip', downsample='bogus')
    with pytest.raises(ValueError, match='--unet-downsample strided goes with --unet hip'):
        cli.load_sd_unet(model, torch.device('cpu'), 'diffusers', downsample='strided')
    with pytest.raises(FileNotFoundError, match='DTS_SD_UNET_DIR'):        # a good mode reaches the directory, as the call without it does
        cli.load_sd_unet(model, torch.device('cpu'), 'hip', downsample='strided')
    with pytest.raises(FileNotFoundError, match='DTS_SD_UNET_DIR'):
        cli.load_sd_unet(model, torch.device('cpu'), 'hip', head_dims='native', downsample='s2d')
