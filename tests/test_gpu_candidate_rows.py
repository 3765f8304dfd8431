"""GPU: `dts_candidate_noise_rows`, the per-row form of the candidate builder (mode / scale per OUTPUT row: searches of several seeds in
lock-step, whose coins differ from image to image), in float64.

Reference: tests/elementwise_reference.candidate_noise_ref called row by row (row r = n * b + sample against pivot[sample], mode[r], scale[r]),
with that file's bound, 2 e64 |pivot| + (ceil(chw / 256) + 16) e64 |scale g / norm|.  Shapes: chw = 192 (fewer elements than the block's 256
threads, one wave idle), 300 (a partial second trip of the strided loops), 768 (three whole trips); (N, B) = (1, 1), (4, 3), (3, 4); modes mixed
within a candidate across its images, all 0, all 1.  Exact properties: a mode-0 row is its Gaussian, scale 0 returns the pivot, and with mode /
scale constant over the images of every candidate the output is `ops.candidate_noise`'s bit for bit (one body, same reduction order)."""
import pytest
import torch

import elementwise_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CHW = (192, 300, 768)
NB = ((1, 1), (4, 3), (3, 4))


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


def inputs(n, b, chw, seed):
    g = torch.Generator().manual_seed(seed)
    pivot = torch.randn(b, chw, generator=g, dtype=torch.float64)
    gauss = torch.randn(n * b, chw, generator=g, dtype=torch.float64)
    scale = (torch.rand(n * b, generator=g) * 30).to(torch.float32)
    return pivot, gauss, scale


def mixed_modes(n, b):
    """rows n-major: candidate n's images alternate, starting with n's parity -- every candidate with b > 1 holds both branches"""
    return torch.tensor([(n_ + s) % 2 for n_ in range(n) for s in range(b)], dtype=torch.int32)


def rows_ref(pivot, gauss, mode, scale):
    b = pivot.shape[0]
    parts = [R.candidate_noise_ref(pivot[r % b:r % b + 1], gauss[r:r + 1], mode[r:r + 1], scale[r:r + 1]) for r in range(gauss.shape[0])]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


@pytest.mark.parametrize('chw', CHW)
@pytest.mark.parametrize('n,b', NB)
def test_rows_form_against_the_reference_row_by_row(ops, n, b, chw):
    pivot, gauss, scale = inputs(n, b, chw, 100 * n + 10 * b + chw)
    scale[::3] = 0.0                                                                # some rows step nowhere
    worst = 0.0
    for what, mode in (('mixed', mixed_modes(n, b)), ('all 0', torch.zeros(n * b, dtype=torch.int32)), ('all 1', torch.ones(n * b, dtype=torch.int32))):
        ref, bound = rows_ref(pivot, gauss, mode, scale)
        got = ops.candidate_noise_rows(pivot.to(DEV), gauss.to(DEV), mode.to(DEV), scale.to(DEV)).cpu()
        ratio, err = R.worst(got, ref, bound)
        worst = max(worst, ratio)
        assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (what, ratio, err)
        keep = mode == 0
        assert torch.equal(got[keep], gauss[keep]), what                            # mode 0: the Gaussian, bit for bit
        zero = (mode == 1) & (scale == 0)
        assert torch.equal(got[zero], pivot[torch.arange(n * b) % b][zero]), what   # scale 0: the pivot itself
        if what == 'mixed' and b > 1:
            assert all(len(set(mode.view(n, b)[n_].tolist())) == 2 for n_ in range(n))
    print(f'candidate_noise_rows N={n} B={b} chw={chw}: worst err/bound {worst:.3f}')


@pytest.mark.parametrize('chw', CHW)
@pytest.mark.parametrize('n,b', NB)
def test_constant_over_images_is_the_per_candidate_form_bit_for_bit(ops, n, b, chw):
    pivot, gauss, _ = inputs(n, b, chw, 7 * n + b + chw)
    g = torch.Generator().manual_seed(n + b)
    mode = (torch.arange(n) % 2).to(torch.int32) if n > 1 else torch.ones(1, dtype=torch.int32)
    scale = (torch.rand(n, generator=g) * 30).to(torch.float32)
    want = ops.candidate_noise(pivot.to(DEV), gauss.to(DEV), mode.to(DEV), scale.to(DEV))
    got = ops.candidate_noise_rows(pivot.to(DEV), gauss.to(DEV), mode.repeat_interleave(b).to(DEV), scale.repeat_interleave(b).to(DEV))
    assert torch.equal(got, want)
    got2 = ops.candidate_noise_rows(pivot.to(DEV), gauss.to(DEV), mode.repeat_interleave(b).view(n, b).to(DEV), scale.repeat_interleave(b).view(n, b).to(DEV))
    assert torch.equal(got2, want)                                                  # [N, B] as the sampler holds them


def test_rebuilding_b_pivots_is_one_launch_with_nb_equal_b(ops):
    """nb = b = B: image b's next pivot from its own winner, mode and scale -- what took B one-row launches of the per-candidate form"""
    B, chw = 4, 300
    pivot, gauss, scale = inputs(1, B, chw, 5)
    mode = torch.tensor([1, 0, 1, 1], dtype=torch.int32)
    got = ops.candidate_noise_rows(pivot.to(DEV), gauss.to(DEV), mode.to(DEV), scale.to(DEV))
    rows = [ops.candidate_noise(pivot[b:b + 1].to(DEV), gauss[b:b + 1].to(DEV), mode[b:b + 1].to(DEV), scale[b:b + 1].to(DEV)) for b in range(B)]
    assert torch.equal(got, torch.cat(rows))


def test_argument_errors_are_reported_through_dts_last_error(ops):
    from diffusion_tts_amd import _lib
    pivot, gauss, scale = inputs(2, 2, 192, 1)
    mode = torch.ones(4, dtype=torch.int32)
    p, g, m, s = (t.to(DEV) for t in (pivot, gauss, mode, scale))
    out = torch.empty_like(g)
    with pytest.raises(RuntimeError, match='dts_candidate_noise_rows: null pointer'):
        ops._call('dts_candidate_noise_rows', p.data_ptr(), g.data_ptr(), None, s.data_ptr(), out.data_ptr(), 4, 2, 192)
    assert b'dts_candidate_noise_rows: null pointer' in _lib.load().dts_last_error()
    for nb, b, chw in ((3, 2, 192), (0, 2, 192), (4, 0, 192), (4, 2, 0)):            # nb no multiple of b; empty sizes
        with pytest.raises(RuntimeError, match=f'dts_candidate_noise_rows: nb={nb} b={b}'):
            ops._call('dts_candidate_noise_rows', p.data_ptr(), g.data_ptr(), m.data_ptr(), s.data_ptr(), out.data_ptr(), nb, b, chw)
        assert f'dts_candidate_noise_rows: nb={nb} b={b}'.encode() in _lib.load().dts_last_error()
    with pytest.raises(ValueError, match='one entry per output row'):               # the binding: mode / scale per candidate are the other form's
        ops.candidate_noise_rows(p, g, m[:2].contiguous(), s[:2].contiguous())
