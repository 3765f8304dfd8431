"""CPU: the reference of the JPEG stage tests, pinned without a GPU.  jpeg_helpers.decode_scan entropy-decodes the files Pillow writes
with the Huffman tables of their own DHT segments; here its coefficients equal the integer model of the transform stage
(jpeg_helpers.model_coefficients), the header it skips has the length ops.jpeg_header_bytes() states, and its bit count accounts for
every byte of the file.  The inputs the GPU tests feed the kernels do reach what they are there for: the largest DC category of either
table, the largest AC category of either table, runs of 62 zeros (three ZRL codes) in either table, stuffed bytes and blocks without
EOB.  No kernel runs; no tolerance anywhere."""
import numpy as np
import pytest

from jpeg_helpers import SPECIAL_KINDS, all_kinds, decode_scan, make_images, model_coefficients, pil_jpeg, special_image, zrl_image

QUALITIES = [1, 30, 49, 50, 80, 95, 100]


def check_file(img, quality):
    data = pil_jpeg(img, quality)
    from diffusion_tts_amd import ops
    s = decode_scan(data)
    assert (s.height, s.width) == img.shape[1:]
    want = model_coefficients(img, quality)
    assert s.coef.shape == want.shape and np.array_equal(s.coef, want), np.argwhere(s.coef != want)[:8]
    assert s.header == ops.jpeg_header_bytes()
    assert (s.total + 7) // 8 + s.stuffed + s.header + 2 == len(data)
    assert len(s.stream) == (s.total + 7) // 8
    assert s.start[0] == 0 and np.all(np.diff(s.start) > 0) and s.start[-1] < s.total
    return s


@pytest.mark.parametrize('quality', QUALITIES)
def test_decoder_equals_the_integer_model_and_the_file_length(quality):
    """every kind of image at 32x32, two images of each random kind, and the one-MCU constructed image"""
    names, imgs = all_kinds(32, 32, seed=quality)
    for name, img in list(zip(names, imgs)) + [(k, make_images(k, 2, 32, 32, seed=quality)[1]) for k in names[:4]] + [('zrl16', zrl_image())]:
        s = check_file(img, quality)
        print(f'quality {quality} {name}: {s.total} bits, {s.stuffed} stuffed, DC categories {s.dc_cat}, AC {s.ac_cat}, lanes {s.lane}, runs {s.run}')


@pytest.mark.parametrize('h,w', [(16, 16), (48, 80), (80, 48), (112, 112)])
def test_decoder_walks_non_square_images_in_mcu_order(h, w):
    names, imgs = all_kinds(h, w)
    for img in imgs:
        check_file(img, 80)


def test_inputs_reach_the_largest_categories_runs_and_lanes():
    """What the GPU stream tests rely on, shown on the reference alone (table 0: luma, table 1: chroma).  A clean run of 62 in front of a
    category-10 value (the 59-bit lane of LaneBits) cannot be had from a rounded 8-bit image; the longest lanes reached are printed, and
    45 bits (three ZRLs, a 16-bit code, one value bit in the chroma table) is the least either table must see."""
    at100 = {k: decode_scan(pil_jpeg(special_image(k, 32, 32), 100)) for k in SPECIAL_KINDS}
    assert at100['checker'].dc_cat[0] == 11
    assert {-1024, 1016} <= set(at100['checker'].coef[:, 0].tolist())
    assert at100['redblue'].dc_cat[1] == 11
    cb = at100['redblue'].coef[4::6, 0]
    assert cb.min() == -344 and cb.max() == 1016
    assert at100['ac10'].ac_cat[0] == 10 and int(at100['ac10'].coef[0, 63]) == 838
    assert at100['ac10c'].ac_cat[1] == 10
    runs, lanes = [0, 0], [0, 0]
    for q in QUALITIES:
        s = decode_scan(pil_jpeg(zrl_image(), q))
        runs = [max(a, b) for a, b in zip(runs, s.run)]
        lanes = [max(a, b) for a, b in zip(lanes, s.lane)]
    low = decode_scan(pil_jpeg(special_image('zrl', 32, 32), 1))                # quality 1 is one of the qualities the kernels run at
    assert low.run == [62, 62] and low.no_eob >= 1
    noise = decode_scan(pil_jpeg(make_images('noise', 1, 64, 64)[0], 80))
    assert noise.stuffed >= 1 and noise.no_eob >= 1
    print(f'largest DC category: luma {at100["checker"].dc_cat[0]}, chroma {at100["redblue"].dc_cat[1]}; largest AC category: luma '
          f'{at100["ac10"].ac_cat[0]}, chroma {at100["ac10c"].ac_cat[1]}; longest run: luma {runs[0]}, chroma {runs[1]}; longest lane: luma '
          f'{lanes[0]} bits, chroma {lanes[1]} bits; stuffed pairs in 64x64 noise: {noise.stuffed}; blocks without EOB: {noise.no_eob}')
    assert runs == [62, 62]
    assert min(lanes) >= 45, lanes


def test_decoder_refuses_a_broken_padding():
    """the padding assertion is live: clearing one of the 1-bits that complete the last byte is noticed"""
    img = make_images('smooth', 1, 32, 32)[0]
    for quality in QUALITIES:
        data = bytearray(pil_jpeg(img, quality))
        tail = 8 * len(decode_scan(bytes(data)).stream) - decode_scan(bytes(data)).total
        if tail and data[-3] != 0:                                                # (data[-3]: the last entropy byte, not a stuffed zero)
            data[-3] &= 0xFE
            with pytest.raises(AssertionError, match='padding'):
                decode_scan(bytes(data))
            return
    raise AssertionError('no quality left padding bits to break')
