"""CPU: the host-side pieces of the JPEG byte-length path (ops.jpeg_quant_tables, ops.jpeg_header_bytes, the codec= switch of
CompressibilityScorer and of the CLI) against files Pillow writes.  No kernel runs."""
import numpy as np
import pytest
import torch

from jpeg_helpers import make_images, parse_segments, pil_jpeg


@pytest.mark.parametrize('quality', [1, 30, 50, 80, 95, 100])
def test_quant_tables_and_header_equal_pillows(quality):
    from diffusion_tts_amd import ops
    seg = parse_segments(pil_jpeg(make_images('noise', 1, 32, 32)[0], quality))
    luma, chroma = ops.jpeg_quant_tables(quality)
    assert sorted(seg['dqt']) == [0, 1]
    assert list(luma) == seg['dqt'][0] and list(chroma) == seg['dqt'][1]
    assert ops.jpeg_header_bytes() == seg['entropy']


@pytest.mark.parametrize('quality', [0, 101, -3, 80.0, None, True])
def test_quality_outside_1_100_is_refused_by_name(quality):
    from diffusion_tts_amd import ops, scorers
    with pytest.raises(ValueError, match='quality'):
        ops.jpeg_quant_tables(quality)
    with pytest.raises(ValueError, match='quality'):
        scorers.CompressibilityScorer(quality=quality, codec='hip')


def test_codec_switch_and_cpu_refusals():
    from diffusion_tts_amd import ops, scorers
    pil = scorers.CompressibilityScorer()
    assert pil.codec == 'pil' and not getattr(pil, 'batched', False)           # the default is the host codec, per-image in the SD loop
    hip = scorers.CompressibilityScorer(codec='hip', max_size=150000)
    assert hip.codec == 'hip' and hip.batched is True
    with pytest.raises(ValueError, match='codec'):
        scorers.CompressibilityScorer(codec='turbo')
    img = torch.from_numpy(make_images('noise', 2, 32, 32))
    with pytest.raises(ValueError, match='cpu'):                               # a CPU tensor: no fallback to the host codec
        hip(img, None, None)
    with pytest.raises(ValueError, match='cpu'):
        ops.jpeg_size(img)
    with pytest.raises(ValueError, match='uint8'):
        ops.jpeg_size(img.float())
    # the default path did not change: a CPU uint8 batch still goes through Pillow
    want = [1.0 - min(1.0, max(0.0, len(pil_jpeg(im.numpy())) / 3000)) for im in img]
    assert torch.equal(pil(img, None, None), torch.tensor(want))


def test_cli_passes_the_codec_through():
    import main
    assert main.get_scorer('edm', 'compressibility', 'cuda').codec == 'pil'
    s = main.get_scorer('sd', 'compressibility', 'cuda', jpeg_codec='hip')
    assert s.codec == 'hip' and s.max_size == 150000 and s.batched
    assert main.get_scorer('edm', 'compressibility', 'cuda', jpeg_codec='hip').max_size == 3000
