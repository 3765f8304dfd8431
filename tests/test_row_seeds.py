"""CPU: per-image random streams (`generate_image_grid(row_seeds=...)`) and the lock-step split of bulk mode.

The draw source alone: image b of a batch with row_seeds = [0, 5, 7] gets, number for number, what a one-image search gets from torch's global
generator after torch.manual_seed(row_seeds[b]) -- for the naive sampler, rejection sampling, the beam search and eps-greedy (pivots,
Gaussians, the discarded first draw, the coin-derived mode[n][b] and scale[n][b]) -- and a seed's numbers do not depend on its position or
its companions ([7, 0, 5]).  The one-image side of the first three is written out here as the expression the searches have always used.
Then the refusals by name, and rank_batches with a search batch."""
from types import SimpleNamespace

import pytest
import torch

from diffusion_tts_amd import bulk, sampler as sm
from diffusion_tts_amd.hashing import seed0_scale

SEEDS, SHUFFLED = [0, 5, 7], [7, 0, 5]
SHAPE1 = (3, 16, 16)
STEPS = 4
F64 = torch.float64


def test_a_fresh_generator_replays_the_global_stream():
    """what the whole construction rests on: normals (float64 and float32), rand(1) interleaved, seeds past 2^31 up to the generator's 32 bits"""
    for s in (0, 7, 2 ** 31 + 5, 2 ** 32 - 1):
        torch.manual_seed(s)
        want = [torch.randn((1,) + SHAPE1, dtype=F64), torch.rand(1), torch.randn((4,) + SHAPE1, dtype=F64), torch.rand(1), torch.randn(2, 5)]
        src = sm._Source([s])
        got = [src.randn(0, (1,) + SHAPE1), src.rand1(0), src.randn(0, (4,) + SHAPE1), src.rand1(0), src.randn(0, (2, 5), dtype=torch.float32)]
        assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(want, got)), s
    for s in (2 ** 32 + 7, -1):                                                    # torch would replay seed 7 for 2^32 + 7: refused, not reduced
        with pytest.raises(ValueError, match=r'row_seeds: seed -?\d+ is outside \[0, 2\^32\)'):
            sm._Source([0, s])


def test_without_row_seeds_the_source_is_the_global_stream():
    torch.manual_seed(3)
    want = [torch.randn((2,) + SHAPE1, dtype=F64), torch.randn((2 * 3,) + SHAPE1, dtype=F64),
            torch.stack([torch.randn((3,) + SHAPE1, dtype=F64) for _ in range(2 * 2)]), torch.rand(1)]
    torch.manual_seed(3)
    src = sm._Source()
    got = [src.images(2, 1, SHAPE1), src.images(2, 3, SHAPE1), src.beams(2, 2, 3, SHAPE1), src.rand1(None)]
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    assert src.lanes((2,) + SHAPE1) == [(None, (2,) + SHAPE1)]


@pytest.mark.parametrize('order', [SEEDS, SHUFFLED])
def test_naive_rejection_and_beam_draws_per_image(order):
    N, B = 4, 2
    src = sm._Source(order)
    naive = [src.images(len(order), 1, SHAPE1) for _ in range(STEPS)]
    src = sm._Source(order)
    rej = [src.images(len(order), N, SHAPE1).view(len(order), N, *SHAPE1) for _ in range(STEPS)]            # b-major rows
    src = sm._Source(order)
    beam = [src.beams(len(order), B, 3, SHAPE1).view(len(order), B, 3, *SHAPE1) for _ in range(STEPS)]      # image-major beam rows
    for b, s in enumerate(order):
        torch.manual_seed(s)
        for i in range(STEPS):
            assert torch.equal(naive[i][b:b + 1], torch.randn((1,) + SHAPE1, dtype=F64)), (s, i)
        torch.manual_seed(s)
        for i in range(STEPS):
            assert torch.equal(rej[i][b], torch.randn((1 * N,) + SHAPE1, dtype=F64)), (s, i)
        torch.manual_seed(s)
        for i in range(STEPS):
            assert torch.equal(beam[i][b], torch.stack([torch.randn((3,) + SHAPE1, dtype=F64) for _ in range(1 * B)])), (s, i)


def eps_greedy_stream(src, images):
    """every item `_eps_greedy_draws` yields for N = 3, K = 2 over `images` images: pivots, then (Gaussians [N][B, ...], mode, scale) per iteration"""
    L = SimpleNamespace(num_steps=STEPS, scale_fn=seed0_scale, src=src)
    p = SimpleNamespace(N=3, K=2, eps=0.4)
    return list(sm._eps_greedy_draws(L, p, None, (images,) + SHAPE1, 0.15 * (3 * 64 * 64) ** 0.5))


def test_eps_greedy_draws_per_image():
    solo = {}
    for s in SEEDS:
        torch.manual_seed(s)
        solo[s] = eps_greedy_stream(sm._Source(), 1)
    coins = set()
    for order in (SEEDS, SHUFFLED):
        batch = eps_greedy_stream(sm._Source(order), len(order))
        assert len(batch) == STEPS * (1 + 2)
        for b, s in enumerate(order):
            for item, one in zip(batch, solo[s]):
                if not isinstance(item, tuple):                                    # a pivot [B, ...]
                    assert item.shape == (len(order),) + SHAPE1 and torch.equal(item[b:b + 1], one)
                    continue
                (g, mode, scale), (g1, mode1, scale1) = item, one
                assert mode.shape == scale.shape == (3, len(order)) and mode.dtype == torch.int32 and scale.dtype == torch.float32
                assert mode1.shape == scale1.shape == (3, 1)                       # without row_seeds: one lane, one coin per candidate, as ever
                assert torch.equal(mode[:, b], mode1[:, 0]) and torch.equal(scale[:, b], scale1[:, 0])
                for n in range(3):
                    assert g[n].shape == (len(order),) + SHAPE1 and torch.equal(g[n][b:b + 1], g1[n]), (s, n)
                    assert float(scale[n, b]) == 0.0 or int(mode[n, b]) == 1
                coins.add(tuple(mode[:, b].tolist()))
    assert len(coins) > 1                                                           # the images' coins do differ: the case the per-row kernel form is for
    # a one-image source with its seed is the global stream after manual_seed, item for item
    for item, one in zip(eps_greedy_stream(sm._Source([5]), 1), solo[5]):
        if isinstance(item, tuple):
            assert torch.equal(item[1].reshape(-1), one[1][:, 0]) and torch.equal(item[2].reshape(-1), one[2][:, 0])
            assert all(torch.equal(a, b) for a, b in zip(item[0], one[0]))
        else:
            assert torch.equal(item, one)


class StubNet:
    img_resolution, img_channels, label_dim = 16, 3, 0

    def round_sigma(self, sigma):
        return torch.as_tensor(sigma)

    def __call__(self, *a):
        raise AssertionError('a refused call must not reach the denoiser')


def test_refusals_by_name():
    lat = torch.zeros((3,) + SHAPE1)
    M = sm.SamplingMethod
    params = dict(scorer=None, N=3, K=2)

    def call(method=M.EPS_GREEDY, **kw):
        kw.setdefault('row_seeds', [0, 5, 7])
        return sm.generate_image_grid(StubNet(), None, lat, None, num_steps=STEPS, sampling_method=method, sampling_params=params,
                                      verbose=False, **kw)
    with pytest.raises(ValueError, match='row_seeds: need one seed per image, got 2 seeds for 3 images'):
        call(row_seeds=[0, 5])
    with pytest.raises(ValueError, match='row_seeds: SamplingMethod.MCTS'):
        call(M.MCTS)
    with pytest.raises(ValueError, match='row_seeds: forced_selections'):
        call(forced_selections=[0] * (STEPS * 2))
    with pytest.raises(ValueError, match='row_seeds: precomputed_noise'):
        call(M.REJECTION_SAMPLING, precomputed_noise={0: torch.zeros(3, 3, *SHAPE1)})
    with pytest.raises(ValueError, match='search_batch'):
        bulk.generate_seeds(StubNet(), '0-3', '.', search_batch=0)


def test_candidate_sharding_is_refused_with_row_seeds(monkeypatch):
    """more than one rank sharing the candidates of a lock-step batch (what CandidateShards reports as not solo)"""
    import diffusion_tts_amd.sampler as mod

    class TwoRanks:
        solo, rank, collectives = False, 0, 0

        def __init__(self, enabled=True):
            pass
    monkeypatch.setattr(mod, 'CandidateShards', TwoRanks)
    with pytest.raises(ValueError, match='row_seeds: candidate sharding'):
        sm.generate_image_grid(StubNet(), None, torch.zeros((2,) + SHAPE1), None, num_steps=STEPS, sampling_method=sm.SamplingMethod.NAIVE,
                               verbose=False, row_seeds=[1, 2])


@pytest.mark.parametrize('count', [8, 7, 1])
@pytest.mark.parametrize('search_batch', [1, 2, 4])
def test_rank_batches_with_a_search_batch_covers_every_seed_once(count, search_batch):
    seeds = list(range(10, 10 + count))
    for world in (1, 2):
        per_rank = [[b.tolist() for b in bulk.rank_batches(seeds, search_batch, r, world)] for r in range(world)]
        flat = sorted(s for batches in per_rank for b in batches for s in b)
        assert flat == seeds, (world, per_rank)
        assert all(len(b) <= search_batch for batches in per_rank for b in batches)
    one = [b.tolist() for b in bulk.rank_batches(seeds, search_batch, 0, 1) if len(b)]
    two = sorted(b.tolist() for r in range(2) for b in bulk.rank_batches(seeds, search_batch, r, 2) if len(b))
    if count % (2 * search_batch) == 0:                                            # whole batches for both worlds: the same batches, dealt out in turn
        assert one == two
