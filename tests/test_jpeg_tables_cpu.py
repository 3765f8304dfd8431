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


def test_shapes_whose_bit_count_could_pass_int_are_refused():
    """Bit counts, block offsets and positions are int in every kernel.  A block costs at most 64 * (16 + 11) = 1728 bits, so an image of
    up to (2^31 - 1) // 1728 // 6 = 207 126 MCUs cannot wrap them and one more could: dts_jpeg_workspace_bytes (host arithmetic, no
    allocation, no GPU) answers 0 from there on, which ops.jpeg_size turns into a ValueError.  A 16-pixel-high image has at most 1024 MCUs
    (w <= 16384), far below the bound: it is the width cap that ends those."""
    import launch_rules as R
    from diffusion_tts_amd import _lib
    lib = _lib.load()
    last = ((1 << 31) - 1) // R.JPEG_BLOCK_MAX_BITS // 6
    assert last == 207126 and last * 6 * R.JPEG_BLOCK_MAX_BITS < 1 << 31 <= (last + 1) * 6 * R.JPEG_BLOCK_MAX_BITS

    def accepted(n, h, w):
        got = lib.dts_jpeg_workspace_bytes(n, h, w)
        assert (got > 0) == R.jpeg_shape_ok(n, h, w) and (got == 0 or got == R.jpeg_layout(n, h, w).bytes), (n, h, w, got)
        return got > 0
    # square: 455^2 = 207 025 MCUs is the last accepted side, 456^2 = 207 936 the first refused
    assert 455 * 455 <= last < 456 * 456
    assert accepted(1, 455 * 16, 455 * 16) and not accepted(1, 456 * 16, 456 * 16)
    # the MCU count itself: 666 x 311 = 207 126 (the last accepted count), 611 x 339 = 207 129 (207 127 and 207 128 have no factor pair
    # within 1024 x 1024), either way round
    assert 666 * 311 == last and last < 611 * 339 <= last + 3
    for a, b in ((666, 311), (311, 666)):
        assert accepted(1, a * 16, b * 16)
    for a, b in ((611, 339), (339, 611), (1024, 203), (1024, 1024)):
        assert not accepted(1, a * 16, b * 16)
    assert accepted(1, 1024 * 16, 202 * 16)
    # the bound is per image: n does not enter it (n * blocks <= 2^24 is the older cap, and it binds first for n >= 14)
    assert accepted(13, 666 * 16, 311 * 16) and not accepted(14, 666 * 16, 311 * 16) and not accepted(2, 611 * 16, 339 * 16)
    # 16 pixels high (and wide): every width up to the cap, at every n the block cap leaves
    assert accepted(1, 16, 16384) and accepted(1, 16384, 16) and accepted(2730, 16, 16384) and not accepted(1, 16, 16400) and not accepted(1, 16400, 16)
    # what the search loops produce
    assert accepted(64, 512, 512) and accepted(64, 1024, 1024) and accepted(1, 16, 16)


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
