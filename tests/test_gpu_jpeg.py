"""GPU: ops.jpeg_size / CompressibilityScorer(codec='hip') against Pillow itself -- the byte length of the file
`PIL.Image.save(format='JPEG', quality=q)` writes, exact (no tolerance anywhere in this file), the quantised coefficients against an
integer numpy model of the transform stage, the scorer against the default codec and the reference-made fixture, one search with
either codec, and the refusals."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import tiny_edm, T                                                          # noqa: E402
from jpeg_helpers import ZIGZAG, make_images, parse_segments, pil_jpeg, zrl_image       # noqa: E402
from diffusion_tts_amd import ops, scorers                                               # noqa: E402
from diffusion_tts_amd.hashing import seed0_scale                                        # noqa: E402

DEV = 'cuda'
KINDS = ['noise', 'smooth', 'flat', 'sat']


def pil_sizes(imgs, quality=80):
    return np.array([len(pil_jpeg(im, quality)) for im in imgs], dtype=np.int32)


def gpu_sizes(imgs, quality=80):
    got = ops.jpeg_size(torch.from_numpy(imgs).to(DEV), quality)
    assert got.dtype == torch.int32 and got.is_cuda and got.shape == (imgs.shape[0],)
    return got.cpu().numpy()


# ---- exact sizes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('h,w', [(16, 16), (32, 32), (64, 64), (48, 80)])
def test_size_equals_pillow(h, w, kind):
    """16x16: one MCU, every DC predictor at its start value; 48x80: rows != columns, so an MCU-order or row/column mix-up shows.
    Batches of 1, 5 and 64 distinct images: every image has its own bit offsets and its own stretch of the bit buffer."""
    for n in (1, 5, 64):
        imgs = make_images(kind, n, h, w)
        assert len({im.tobytes() for im in imgs}) == n
        want = pil_sizes(imgs)
        got = gpu_sizes(imgs)
        print(f'{h}x{w} {kind} n={n}: Pillow {want[:5]}, HIP {got[:5]}')
        assert np.array_equal(got, want), (h, w, kind, n, np.nonzero(got != want)[0][:8], got[:8], want[:8])


def test_size_equals_pillow_512():
    """6 144 blocks per image: several workgroups per image in every stage, 24 blocks per thread in the offset scan"""
    imgs = np.concatenate([make_images('noise', 1, 512, 512), make_images('smooth', 1, 512, 512)])
    want = pil_sizes(imgs)
    got = gpu_sizes(imgs)
    print(f'512x512 noise, smooth: Pillow {want}, HIP {got}')
    assert np.array_equal(got, want)


@pytest.mark.parametrize('quality', [80, 30, 95, 100])
def test_size_equals_pillow_over_qualities(quality):
    imgs = np.concatenate([make_images(k, 2, 32, 32, seed=quality) for k in KINDS])
    want = pil_sizes(imgs, quality)
    got = gpu_sizes(imgs, quality)
    print(f'quality {quality}: Pillow {want}, HIP {got}')
    assert np.array_equal(got, want)


def test_inputs_reach_byte_stuffing_zrl_and_blocks_without_eob():
    """The cases above cannot pass vacuously: (1) a Pillow stream of the 64x64 noise images holds stuffed FF 00 pairs, (2) some block has a
    zero run longer than 15 in front of a non-zero coefficient (ZRL), (3) some block ends on coefficient 63 (no EOB) -- (2) and (3) read
    off the kernel's own coefficients, and the image that has them is held to Pillow's size like every other."""
    noise = make_images('noise', 5, 64, 64)
    stuffed = 0
    for im in noise:
        data = pil_jpeg(im)
        stuffed += data[parse_segments(data)['entropy']:-2].count(b'\xff\x00')
    assert stuffed >= 1, stuffed
    imgs = np.concatenate([noise[:1, :, :16, :16], zrl_image()[None]])
    sizes, coef = ops.jpeg_size(torch.from_numpy(imgs).to(DEV), return_coefficients=True)
    coef = coef.cpu().numpy()
    assert coef.shape == (2, 6, 64) and coef.dtype == np.int16
    zrl = ends63 = 0
    for blk in coef.reshape(-1, 64):
        nz = np.nonzero(blk[1:])[0] + 1
        if len(nz):
            runs = np.diff(np.concatenate([[0], nz])) - 1
            zrl += int((runs > 15).any())
            ends63 += int(nz[-1] == 63)
    print(f'stuffed FF00 pairs {stuffed}; blocks with a run > 15: {zrl}; blocks ending on coefficient 63: {ends63}')
    assert zrl >= 1 and ends63 >= 1
    chroma = coef[1, 4:]                                                 # the constructed image: one AC coefficient, at 63 (three ZRLs)
    assert all(np.count_nonzero(b[1:]) == 1 and b[63] != 0 for b in chroma)
    assert np.array_equal(sizes.cpu().numpy(), pil_sizes(imgs))


# ---- stage A alone ----------------------------------------------------------------------------------------------------------------------
BASE_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def model_fdct(b):
    """the "slow integer" 8x8 forward DCT over the last two axes of an int64 array: 13-bit constants, 2 extra bits through the row pass,
    rounding right shifts, output scaled by 8"""
    def one_pass(d, first):
        d = [d[..., i] for i in range(8)]
        t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        n = 11 if first else 15

        def ds(x, n=n):
            return (x + (1 << (n - 1))) >> n
        o = [None] * 8
        o[0], o[4] = ((t10 + t11) << 2, (t10 - t11) << 2) if first else (ds(t10 + t11, 2), ds(t10 - t11, 2))
        z1 = (t12 + t13) * 4433
        o[2], o[6] = ds(z1 + t13 * 6270), ds(z1 - t12 * 15137)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * 9633
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        o[7], o[5], o[3], o[1] = ds(t4 * 2446 + z1 + z3), ds(t5 * 16819 + z2 + z4), ds(t6 * 25172 + z2 + z3), ds(t7 * 12299 + z1 + z4)
        return np.stack(o, axis=-1)
    rows = one_pass(b, True)
    return np.swapaxes(one_pass(np.swapaxes(rows, -1, -2), False), -1, -2)


def model_coefficients(img, quality):
    """img uint8 [3, h, w] -> int16 [h/16 * w/16 * 6, 64]: colour, 2x2 chroma mean, level shift, DCT, quantisation; zigzag, scan order"""
    R, G, B = (img[i].astype(np.int64) for i in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    h, w = Y.shape
    bias = np.tile(np.array([1, 2]), w // 4)[None, :]
    Cb, Cr = ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2 for c in (Cb, Cr))
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    ql, qc = (np.clip((np.array(base) * scale + 50) // 100, 1, 255).reshape(8, 8) * 8 for base in (BASE_LUMA, BASE_CHROMA))
    px, q8 = [], []
    for my in range(h // 16):
        for mx in range(w // 16):
            for by in range(2):
                for bx in range(2):
                    px.append(Y[my * 16 + by * 8:my * 16 + by * 8 + 8, mx * 16 + bx * 8:mx * 16 + bx * 8 + 8])
                    q8.append(ql)
            for c in (Cb, Cr):
                px.append(c[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8])
                q8.append(qc)
    c, q8 = model_fdct(np.stack(px) - 128), np.stack(q8)
    v = np.sign(c) * ((np.abs(c) + (q8 >> 1)) // q8)
    return v.reshape(-1, 64)[:, ZIGZAG].astype(np.int16)


@pytest.mark.parametrize('kind', ['noise', 'smooth'])
def test_coefficients_equal_the_integer_model(kind):
    imgs = make_images(kind, 2, 32, 32, seed=3)
    _, coef = ops.jpeg_size(torch.from_numpy(imgs).to(DEV), return_coefficients=True)
    assert coef.dtype == torch.int16 and coef.shape == (2, 24, 64)
    for i in range(2):
        want = model_coefficients(imgs[i], 80)
        got = coef[i].cpu().numpy()
        assert np.array_equal(got, want), (kind, i, np.argwhere(got != want)[:8])
    assert np.count_nonzero(coef.cpu().numpy()[:, :, 1:]) > 100


# ---- scorer -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_size', [3000, 150000])
def test_scorer_rewards_are_bit_identical_to_the_default_codec(golden, max_size):
    img = T(golden['score_images']).to(DEV)
    want = scorers.CompressibilityScorer(max_size=max_size)(img, None, None)
    hip = scorers.CompressibilityScorer(max_size=max_size, codec='hip')
    got = hip(img, None, None)
    assert got.dtype == want.dtype and got.device == want.device and torch.equal(got, want)
    if max_size == 3000:
        assert np.array_equal(got.numpy(), golden['score_jpeg'])          # the reference's own rewards for these images
    assert len(set(got.tolist())) > 1
    # the SD loop's calling convention: a list of [1, 3, H, W] tensors, one call
    assert hip.batched
    as_list = hip(images=[img[j:j + 1] for j in range(img.shape[0])], prompts=['a prompt'], timesteps=None)
    assert as_list.dtype == want.dtype and as_list.device == want.device and torch.equal(as_list, want)
    one = hip(images=[img[2:3]], prompts=['a prompt'], timesteps=None)
    assert torch.equal(one, want[2:3])


# ---- search -----------------------------------------------------------------------------------------------------------------------------
def test_search_is_the_same_with_either_codec(golden, manifest):
    """one tiny eps-greedy search (tests/test_gpu_search.py's call pattern) scored by JPEG size: same rewards, picks and final image"""
    from diffusion_tts_amd import networks, sampler as sm
    meta = manifest['cases']['epsgreedy_adm_bright']
    cfg, sd = tiny_edm(manifest, meta['net'])
    net = networks.EDMPrecond(cfg, sd, device=DEV, dtype=torch.float32)
    b = meta['batch']
    lat, lab = T(golden[f'search_latents{b}']), T(golden[f'search_lab{b}'])
    res = {}
    for codec in ('pil', 'hip'):
        np.random.seed(0)
        res[codec] = sm.generate_image_grid(net, None, lat, lab, seed=meta['seed'], gridw=b, gridh=1, device=torch.device(DEV),
                                            num_steps=meta['num_steps'], S_churn=40, S_min=0.05, S_max=50, S_noise=1.003,
                                            sampling_method=sm.SamplingMethod.EPS_GREEDY,
                                            sampling_params=dict(scorer=scorers.CompressibilityScorer(codec=codec), **meta['params']),
                                            scale_fn=seed0_scale, compute_dtype=torch.float32, verbose=False)
    p, h = res['pil'], res['hip']
    assert len(p['selected']) == len(h['selected']) > 0
    for a, c in zip(p['selected'], h['selected']):
        assert torch.equal(a, c)
    for a, c in zip(p['rewards'] + [p['final_scores']], h['rewards'] + [h['final_scores']]):
        assert a.dtype == c.dtype and torch.equal(a, c)
    assert any(len(set(r.reshape(-1).tolist())) > 1 for r in p['rewards'])     # the rewards did decide something
    assert torch.equal(p['image'], h['image']) and torch.equal(p['x'], h['x'])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_launch_nothing(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError('a refused call reached the library')
    monkeypatch.setattr(ops, '_call', no_launch)
    hip = scorers.CompressibilityScorer(codec='hip')
    for shape in [(1, 3, 17, 23), (2, 3, 8, 8), (1, 1, 32, 32), (1, 3, 40, 56)]:
        img = torch.zeros(shape, dtype=torch.uint8, device=DEV)
        with pytest.raises(ValueError, match=re.escape(str(shape))):
            ops.jpeg_size(img)
        with pytest.raises(ValueError, match=re.escape(str(shape))):
            hip(img, None, None)
    ok = torch.zeros((1, 3, 32, 32), dtype=torch.uint8)
    with pytest.raises(ValueError, match='cpu'):
        ops.jpeg_size(ok)
    with pytest.raises(ValueError, match='cpu'):
        hip(ok, None, None)
    with pytest.raises(ValueError, match='quality=0'):
        ops.jpeg_size(ok.to(DEV), quality=0)
    with pytest.raises(ValueError, match='quality=0'):
        scorers.CompressibilityScorer(quality=0, codec='hip')
    with pytest.raises(ValueError, match='different shapes'):
        hip([ok.to(DEV), torch.zeros((1, 3, 16, 16), dtype=torch.uint8, device=DEV)], None, None)
