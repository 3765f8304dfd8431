"""GPU: ops.jpeg_size / CompressibilityScorer(codec='hip') against Pillow itself -- the byte length of the file
`PIL.Image.save(format='JPEG', quality=q)` writes, exact (no tolerance anywhere in this file), the quantised coefficients against an
integer numpy model of the transform stage, the scorer against the default codec and the reference-made fixture, one search with
either codec, and the refusals.

Every stage of dts_jpeg_size is also held to the stream of Pillow's own file, entropy-decoded on the CPU (jpeg_helpers.decode_scan): the
coefficients, every block's bit offset, the bit total, every bit of the emitted stream and the zeros behind it, then the size -- in a
workspace the test owns, pre-filled with 0xFF between guard bands, read by the layout tests/launch_rules.py restates."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import tiny_edm, T                                                          # noqa: E402
import launch_rules as R                                                                # noqa: E402
from jpeg_helpers import (all_kinds, decode_scan, make_images, model_coefficients, parse_segments, pil_jpeg, stream_bits,     # noqa: E402
                          zrl_image)
from diffusion_tts_amd import _lib, ops, scorers                                              # noqa: E402
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


# ---- every stage against the decoded stream of Pillow's file -----------------------------------------------------------------------------
GUARD = 4096


def run_stages(imgs, quality):
    """dts_jpeg_size on imgs uint8 [n, 3, h, w] with a workspace, a coefficient output and a size output that each sit between guard bands
    in a buffer pre-filled with 0xFF -> (sizes, coefficients, the workspace's bytes), numpy; asserts that nothing outside them was written"""
    n, _, h, w = imgs.shape
    lay = R.jpeg_layout(n, h, w)
    need = _lib.load().dts_jpeg_workspace_bytes(n, h, w)
    assert need == lay.bytes, (need, lay)
    dev_img = torch.from_numpy(imgs).to(DEV)
    qtab = torch.tensor(ops.jpeg_quant_tables(quality), dtype=torch.int16, device=DEV)
    bufs = {name: torch.full((GUARD + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
            for name, nbytes in (('workspace', lay.bytes), ('coef', n * lay.nb * 128), ('sizes', n * 4))}
    ptr = {name: b.data_ptr() + GUARD for name, b in bufs.items()}
    assert all(p % 16 == 0 for p in ptr.values())
    ops._call('dts_jpeg_size', dev_img.data_ptr(), ptr['sizes'], n, h, w, qtab.data_ptr(), ptr['workspace'], lay.bytes, ptr['coef'])
    torch.cuda.synchronize()
    host = {name: b.cpu().numpy() for name, b in bufs.items()}
    for name, b in host.items():
        assert (b[:GUARD] == 0xFF).all() and (b[-GUARD:] == 0xFF).all(), f'{name}: wrote outside the buffer'
    ws = host['workspace'][GUARD:-GUARD]
    # with coef_out given the workspace's own coefficient array is not used, and the padding between the arrays never is
    blocks = n * lay.nb
    for lo, hi in ((lay.coef, lay.bitoff), (lay.bitoff + blocks * 4, lay.totals), (lay.totals + n * 4, lay.bitbuf),
                   (lay.bitbuf + blocks * R.JPEG_BLOCK_BUF_BYTES, lay.bytes)):
        assert (ws[lo:hi] == 0xFF).all(), f'workspace bytes [{lo}, {hi}) were written'
    return (host['sizes'][GUARD:-GUARD].view(np.int32), host['coef'][GUARD:-GUARD].view(np.int16).reshape(n, lay.nb, 64), ws)


def check_stages(imgs, quality, names=None):
    """every image of the call: coefficients, block bit offsets, bit total, the stream bit for bit, zeros behind it, and the size"""
    n, _, h, w = imgs.shape
    lay = R.jpeg_layout(n, h, w)
    sizes, coef, ws = run_stages(imgs, quality)
    bitoff = ws[lay.bitoff:lay.bitoff + n * lay.nb * 4].view(np.int32).reshape(n, lay.nb)
    totals = ws[lay.totals:lay.totals + n * 4].view(np.int32)
    # bit i of the stream is bit 31 - (i & 31) of word i >> 5: the words' big-endian bytes are the stream's bytes
    words = ws[lay.bitbuf:lay.bitbuf + n * lay.nb * R.JPEG_BLOCK_BUF_BYTES].view('<u4').reshape(n, lay.nb * R.JPEG_BLOCK_BUF_BYTES // 4)
    for im in range(n):
        what = f'{h}x{w} quality {quality} image {im}' + (f' ({names[im]})' if names else '')
        data = pil_jpeg(imgs[im], quality)
        ref = decode_scan(data)
        assert ref.coef.shape == (lay.nb, 64)
        if not np.array_equal(coef[im], ref.coef):
            b, k = np.argwhere(coef[im] != ref.coef)[0]
            raise AssertionError(f'{what}: coefficients differ first in block {b} at zigzag position {k}: {coef[im][b, k]}, Pillow {ref.coef[b, k]}')
        if not np.array_equal(bitoff[im], ref.start):
            b = int(np.nonzero(bitoff[im] != ref.start)[0][0])
            raise AssertionError(f'{what}: bit offsets differ first at block {b}: {bitoff[im][b]}, Pillow {ref.start[b]}')
        assert totals[im] == ref.total, f'{what}: {totals[im]} bits, Pillow {ref.total}'
        got = stream_bits(words[im].astype('>u4').tobytes())
        want = stream_bits(ref.stream, ref.total)
        if not np.array_equal(got[:ref.total], want):
            i = int(np.nonzero(got[:ref.total] != want)[0][0])
            b = int(np.searchsorted(ref.start, i, side='right')) - 1
            raise AssertionError(f'{what}: the stream differs first at bit {i} (bit {i - ref.start[b]} of block {b}): {got[i]}, Pillow {want[i]}')
        stray = np.nonzero(got[ref.total:])[0]
        assert len(stray) == 0, f'{what}: {len(stray)} bits set behind the end of the stream ({ref.total}), the first at bit {ref.total + int(stray[0])}'
        assert sizes[im] == len(data), f'{what}: size {sizes[im]}, Pillow {len(data)} ({ref.stuffed} stuffed bytes)'
    return sizes


def scan_plan_holds(h, w):
    nb, per, busy, last = R.JPEG_SCAN_SHAPES[(h, w)]
    assert R.jpeg_layout(1, h, w).nb == nb and R.jpeg_scan_plan(nb) == (per, busy, last)
    return per, busy


@pytest.mark.parametrize('quality', [80, 100])
@pytest.mark.parametrize('h,w', [(16, 16), (48, 80), (80, 48), (112, 112), (176, 160), (48, 688)])
def test_every_stage_equals_pillows_stream(h, w, quality):
    """One image of every kind in one call.  16x16: one MCU; 48x80 and 80x48: rows != columns either way; 112x112, 176x160, 48x688: 2, 3, 4
    blocks per thread in the offset scan with the upper threads clamped to nothing (48x688: the last busy thread stops short).  Quality 100
    brings the DC categories 11 and the AC categories 10 of the constructed images (tests/test_jpeg_decoder_cpu.py)."""
    per, busy = scan_plan_holds(h, w)
    assert (per, busy < 256) == {(16, 16): (1, True), (48, 80): (1, True), (80, 48): (1, True), (112, 112): (2, True), (176, 160): (3, True),
                                 (48, 688): (4, True)}[(h, w)]
    names, imgs = all_kinds(h, w)
    assert (len(imgs), h, w) in R.JPEG_STREAM_CALLS
    check_stages(imgs, quality, names)


def test_every_stage_equals_pillows_stream_512():
    """6 144 blocks: 24 per thread in the offset scan, every thread busy; `smooth` is the kind whose stream holds no 0xFF byte, so that the
    size alone cannot see it"""
    assert scan_plan_holds(512, 512) == (24, 256) and (1, 512, 512) in R.JPEG_STREAM_CALLS
    check_stages(make_images('smooth', 1, 512, 512), 80, ['smooth'])


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('n', [1, 5, 64])
def test_every_stage_equals_pillows_stream_over_batches(n, kind):
    """every image has its own offsets, its own total and its own stretch of the bit buffer"""
    assert (n, 64, 64) in R.JPEG_STREAM_CALLS and scan_plan_holds(64, 64) == (1, 96)
    check_stages(make_images(kind, n, 64, 64), 80, [kind] * n)


@pytest.mark.parametrize('quality', [1, 49, 50, 80, 100])
def test_every_stage_equals_pillows_stream_over_qualities(quality):
    """quality 1: every table entry 255 and runs of 62 in both tables (the tiled zrl_image); 49 / 50: either side of the scale rule"""
    names, imgs = all_kinds(32, 32, seed=quality)
    assert (len(imgs), 32, 32) in R.JPEG_STREAM_CALLS and scan_plan_holds(32, 32) == (1, 24)
    check_stages(imgs, quality, names)


def test_cached_workspace_serves_smaller_and_differently_shaped_calls():
    """ops.jpeg_size keeps one workspace per device and reuses it for any call it is large enough for: a small call after a large one
    finds the large one's bits and offsets in it.  Each call equals Pillow and its own result from an empty cache."""
    calls = [('noise', 64, 64, 64, 100), ('flat', 1, 16, 16, 80), ('smooth', 5, 32, 32, 80)]
    ops._JPEG_WS.clear()
    reused = [gpu_sizes(make_images(kind, n, h, w), q) for kind, n, h, w, q in calls]
    assert len(ops._JPEG_WS) == 1
    (ws,) = ops._JPEG_WS.values()
    assert ws.numel() == R.jpeg_layout(64, 64, 64).bytes                    # the first call's: the later ones did not replace it
    for (kind, n, h, w, q), got in zip(calls, reused):
        imgs = make_images(kind, n, h, w)
        ops._JPEG_WS.clear()
        fresh = gpu_sizes(imgs, q)
        want = pil_sizes(imgs, q)
        print(f'{kind} n={n} {h}x{w} quality {q}: Pillow {want[:5]}, reused workspace {got[:5]}, fresh {fresh[:5]}')
        assert np.array_equal(got, want) and np.array_equal(fresh, want), (kind, n, h, w)


# ---- stage A alone ----------------------------------------------------------------------------------------------------------------------
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
