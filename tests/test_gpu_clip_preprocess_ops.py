"""GPU: dts_resample_u8 and dts_lut_u8_f32 on their own, exact (no tolerance anywhere in this file).

resample_u8_kernel is one pass of Pillow's 8-bit separable resampling; the image processor only ever runs it on square planes, both
passes, to 224.  Here each pass runs alone, on non-square planes, against Pillow itself -- PIL.Image.resize(..., BICUBIC) of a plane,
which skips the pass whose length does not change -- and both passes in Pillow's order with uint8 in between, with tables from
clip_preprocess.resample_tables: long filters (200 -> 16: 51 taps), short ones (40 -> 100: 5 taps), and pixels of 0 / 255 whose cubic
overshoot clips at both ends.  lut_u8_f32_kernel is a gather: any number of channels, any h * w, a table of distinct values.

Every output sits in the middle of a guard-filled buffer.  One case has 524 288 + 257 outputs, one more block than the 2048 x 256 threads
a launch is capped at: the second trip of the grid-stride loop."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from diffusion_tts_amd import ops                                      # noqa: E402
from diffusion_tts_amd.clip_preprocess import resample_tables          # noqa: E402

DEV = 'cuda'
GUARD = 1024
FILL = 0xA5
PLANES = 5
# (input h, w) -> (output h, w)
CASES = [((37, 53), (16, 24)), ((200, 40), (16, 100)), ((16, 200), (100, 16)), ((64, 48), (64, 20))]
_TABLES = {}


def make_planes(planes, h, w):
    """uint8 [planes, h, w]: uniform noise, and random 0 / 255 pixels in the half where y + x is large (both axes see both halves); the
    last two planes are random 0 / 255 in tiles of a third of the plane instead, so that the long averaging filters also meet edges whose
    overshoot leaves [0, 255]"""
    g = np.random.default_rng([planes, h, w])
    yy, xx = np.mgrid[0:h, 0:w]
    sat = (yy * w + xx * h) >= h * w
    out = np.where(sat[None], g.integers(0, 2, (planes, h, w)) * 255, g.integers(0, 256, (planes, h, w)))
    th, tw = -(-h // 3), -(-w // 3)
    for p in (planes - 2, planes - 1):
        tiles = np.array([[0, 1, 0], [1, 0, 1], [1, 1, 0]]) if p == planes - 2 else g.integers(0, 2, (3, 3))
        out[p] = np.kron(tiles, np.ones((th, tw), dtype=np.int64))[:h, :w] * 255
    return out.astype(np.uint8)


def pil_resize(planes, oh, ow):
    return np.stack([np.asarray(Image.fromarray(p, 'L').resize((ow, oh), Image.BICUBIC)) for p in planes])


def tables(in_len, out_len):
    if (in_len, out_len) not in _TABLES:
        b, k = resample_tables(in_len, out_len)
        _TABLES[(in_len, out_len)] = (torch.from_numpy(b).to(DEV), torch.from_numpy(k).to(DEV))
    return _TABLES[(in_len, out_len)]


def one_pass(x, out_len, axis):
    """dts_resample_u8 on the GPU tensor x [planes, h, w] into the middle of a FILL-filled buffer; the guard bands must stay FILL"""
    planes, h, w = x.shape
    shape = (planes, h, out_len) if axis else (planes, out_len, w)
    numel = int(np.prod(shape))
    bounds, coefs = tables(w if axis else h, out_len)
    buf = torch.full((numel + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
    ops._call('dts_resample_u8', x.data_ptr(), buf.data_ptr() + GUARD, planes, h, w, out_len, axis, bounds.data_ptr(), coefs.data_ptr(),
              coefs.shape[1])
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all()), f'resample_u8 {tuple(x.shape)} -> {shape}: wrote outside'
    return buf[GUARD:GUARD + numel].view(shape)


def assert_same(got, want, what):
    assert want.min() == 0 and want.max() == 255, what                   # the reference clips at both ends
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = tuple(np.argwhere(got != want)[0])
        raise AssertionError(f'{what}: {np.count_nonzero(got != want)} samples differ, the first at {at}: {got[at]}, Pillow {want[at]}')


@pytest.mark.parametrize('src,dst', CASES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_each_pass_and_both_equal_pillow(src, dst):
    (h, w), (oh, ow) = src, dst
    planes = make_planes(PLANES, h, w)
    x = torch.from_numpy(planes).to(DEV)
    both = pil_resize(planes, oh, ow)
    assert_same(ops.resample_u8(x, ow, 1, *tables(w, ow)), pil_resize(planes, h, ow), f'{h}x{w} -> {h}x{ow} (ops.resample_u8)')
    hor = one_pass(x, ow, 1)
    assert_same(hor, pil_resize(planes, h, ow), f'{h}x{w} -> {h}x{ow}, horizontal pass alone')
    if oh == h:                                                           # Pillow runs no vertical pass: the horizontal one is the resize
        assert_same(hor, both, f'{h}x{w} -> {oh}x{ow}')
        return
    assert_same(one_pass(x, oh, 0), pil_resize(planes, oh, w), f'{h}x{w} -> {oh}x{w}, vertical pass alone')
    assert_same(one_pass(hor.contiguous(), oh, 0), both, f'{h}x{w} -> {oh}x{ow}, horizontal then vertical')


def test_filter_lengths_of_the_cases():
    """the long and the short filter are both there, in either direction"""
    assert resample_tables(200, 16)[1].shape[1] == 51 and resample_tables(40, 100)[1].shape[1] == 5
    assert resample_tables(16, 100)[1].shape[1] == 5 and resample_tables(53, 24)[1].shape[1] == 11 and resample_tables(37, 16)[1].shape[1] == 11


def test_resample_takes_the_second_trip_of_the_grid_stride_loop():
    planes, h, w, ow = 5, 49, 700, 2141
    assert planes * h * ow == 524288 + 257
    img = make_planes(planes, h, w)
    want = pil_resize(img, h, ow)
    assert_same(one_pass(torch.from_numpy(img).to(DEV), ow, 1), want, f'{h}x{w} -> {h}x{ow}')


@pytest.mark.parametrize('hw', [(1, 1), (15, 17), (25, 40)], ids=lambda s: f'hw{s[0] * s[1]}')
@pytest.mark.parametrize('c', [1, 3, 4])
def test_lut_is_a_gather_per_channel(c, hw):
    n, (h, w) = 3, hw
    assert h * w in (1, 255, 1000)
    g = torch.Generator().manual_seed(1000 * c + h * w)
    total = n * c * h * w
    img = (torch.arange(total) % 256)[torch.randperm(total, generator=g)].to(torch.uint8).view(n, c, h, w)
    assert total < 256 or len(torch.unique(img)) == 256                   # every byte value, wherever there is room for them
    # a distinct, NaN-free value per entry and channel
    lut = ((torch.randperm(c * 256, generator=g).to(torch.float32) - 300.5) * 0.37).view(c, 256)
    assert len(torch.unique(lut)) == c * 256 and bool(torch.isfinite(lut).all())
    want = torch.stack([lut[ch][img[:, ch].long()] for ch in range(c)], dim=1)
    assert torch.equal(ops.lut_u8_f32(img.to(DEV), lut.to(DEV)).cpu(), want)
    buf = torch.full((total + 2 * GUARD,), float('nan'), dtype=torch.float32, device=DEV)
    dimg, dlut = img.to(DEV), lut.to(DEV)
    ops._call('dts_lut_u8_f32', dimg.data_ptr(), dlut.data_ptr(), buf.data_ptr() + 4 * GUARD, n, c, h * w)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), 'lut_u8_f32 wrote outside the output'
    assert torch.equal(buf[GUARD:-GUARD].view(n, c, h, w).cpu(), want)
