"""CPU: the host side of the SD backend's lock-step searches (no GPU needed).

The per-seed draw source (diffusion_tts_amd/sd_streams.SeedStream) yields exactly the tensors and scalars the global generator yields after
`torch.manual_seed(s)` in the reference loop's call orders (eps-greedy, beam, naive / rejection), for float16 and float32 latents;
`bulk.generate_sd_seeds` splits seeds over ranks like `bulk.generate_seeds` and names its files alike; the CLI parses the new flags and
refuses the combinations that mean nothing; `ops` binds both new entry points and the header's ABI number is the library's."""
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from diffusion_tts_amd import bulk
from diffusion_tts_amd.sd_streams import SeedStream

SHAPE = (1, 4, 8, 8)
DTYPES = [torch.float16, torch.float32]
IDS = ['float16', 'float32']


def global_local_round(n, thr, lam, dtype):
    """the draws of one eps-greedy iteration as the reference makes them on the global generator (pipeline_stable_diffusion.py:1371-1379,
    then the n dropped variance noises of :1410)"""
    draws, mode, scale = [], [], []
    for _ in range(n):
        r = torch.rand(1).item()
        if r < thr:
            draws.append(torch.randn(SHAPE, dtype=dtype))
            mode.append(0)
            scale.append((0.0, 0.0, 0.0))
        else:
            draws.append(torch.randn(SHAPE, dtype=dtype))
            mode.append(1)
            scale.append((torch.rand(1).item(), lam, float(np.sqrt(SHAPE[-1] * SHAPE[-2] * SHAPE[-3]))))
    dropped = [torch.randn(SHAPE, dtype=dtype) for _ in range(n)]
    return torch.stack(draws), mode, scale, dropped


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('seed', [0, 33])
def test_eps_greedy_call_order(seed, dtype):
    """main.py's float32 latents, then per timestep the pivot and K iterations of (coin, Gaussian, step length) x N + N dropped noises"""
    st = SeedStream(seed, SHAPE, dtype)
    torch.manual_seed(seed)
    assert torch.equal(st.latents(), torch.randn(SHAPE))
    modes = []
    for step in range(3):
        pivot = torch.randn(SHAPE, dtype=dtype)
        got = st.randn()
        assert got.dtype == dtype and torch.equal(got, pivot)
        for k in range(2):
            want_u, want_mode, want_scale, _ = global_local_round(4, 0.4, 0.15, dtype)
            u, mode, scale = st.local_round(4, 0.4, 0.15)
            assert u.dtype == dtype and tuple(u.shape) == (4,) + SHAPE and torch.equal(u, want_u)
            assert mode == want_mode and scale == want_scale
            modes += mode
    assert 0 in modes and 1 in modes                                # both branches of the coin were taken
    assert torch.equal(st.randn(), torch.randn(SHAPE, dtype=dtype))  # and the streams are still in step


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_zero_order_draws_no_fresh_gaussian(dtype):
    st = SeedStream(5, SHAPE, dtype)
    torch.manual_seed(5)
    want_u, want_mode, want_scale, _ = global_local_round(3, 0.0, 0.15, dtype)
    u, mode, scale = st.local_round(3, 0.0, 0.15)
    assert mode == want_mode == [1, 1, 1] and scale == want_scale and torch.equal(u, want_u)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_beam_call_order(dtype):
    """per timestep, per beam: N candidate noises (:1080), then the N dropped variance noises of the second step (:1109)"""
    seed, B, N = 4, 2, 3
    st = SeedStream(seed, SHAPE, dtype)
    torch.manual_seed(seed)
    assert torch.equal(st.latents(), torch.randn(SHAPE))
    for step in range(3):
        for beam in range(B):
            want = torch.stack([torch.randn(SHAPE, dtype=dtype) for _ in range(N)])
            for _ in range(N):
                torch.randn(SHAPE, dtype=dtype)
            got = st.beam_round(N)
            assert got.dtype == dtype and torch.equal(got, want), (step, beam)
    assert torch.equal(st.randn(), torch.randn(SHAPE, dtype=dtype))


def test_float16_draws_are_their_own_stream():
    """a float16 normal draw is not the float32 draw rounded: the source must draw in the latents' dtype"""
    a = SeedStream(1, SHAPE, torch.float16).randn()
    b = SeedStream(1, SHAPE, torch.float32).randn()
    assert not torch.equal(a, b.half())


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_rejection_predraw_equals_sequential_naive_runs_on_one_stream(dtype):
    """the reference's main.py:134 loop: N times (latents, then one variance noise per step), all on ONE stream"""
    seed, N, steps = 7, 3, 4
    trajs = SeedStream(seed, SHAPE, dtype).rejection_trajectories(N, steps)
    torch.manual_seed(seed)
    assert len(trajs) == N
    for lat, noises in trajs:
        assert lat.dtype == torch.float32 and torch.equal(lat, torch.randn(SHAPE))
        assert len(noises) == steps
        for z in noises:
            assert z.dtype == dtype and torch.equal(z, torch.randn(SHAPE, dtype=dtype))
    lat, noises = SeedStream(seed, SHAPE, dtype).naive_trajectory(steps)
    assert torch.equal(lat, trajs[0][0]) and all(torch.equal(a, b) for a, b in zip(noises, trajs[0][1]))
    assert SeedStream(seed, SHAPE, dtype).naive_trajectory(steps, draw_latents=False)[0] is None


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('seed', [0, 33])
def test_the_global_generator_is_the_stream_of_seed_none(seed, dtype):
    """SeedStream(None, ...) draws from torch's global generator as it stands: after torch.manual_seed(s) it yields what SeedStream(s, ...)
    yields in every round form the loop uses, two rounds each, and leaves the global generator where the seeded one stands"""
    def draws(st):
        got = []
        for thr in (0.4, 0.0):                                      # eps-greedy, zero-order
            for _ in range(2):
                u, mode, scale = st.local_round(4, thr, 0.15)
                got += [u, torch.tensor(mode), torch.tensor(scale, dtype=torch.float64)]
        got += [st.beam_round(3) for _ in range(2)]
        for _ in range(2):
            lat, noises = st.naive_trajectory(3, draw_latents=False)
            assert lat is None
            got += noises
        return got
    seeded = SeedStream(seed, SHAPE, dtype)
    want = draws(seeded)
    torch.manual_seed(seed)
    glob = SeedStream(None, SHAPE, dtype)
    assert glob.seed is None and glob.gen is None
    got = draws(glob)
    assert len(got) == len(want) == 12 + 2 + 6
    assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(got, want))
    assert all(t.dtype == dtype for t in got[0:12:3] + got[12:])
    assert torch.equal(torch.get_rng_state(), seeded.gen.get_state())


# ---- bulk driver --------------------------------------------------------------------------------------------------------------------------------
class StubPipe:
    """records the calls generate_sd_seeds makes; images carry the seed so the files can be told apart"""

    def __init__(self):
        self.calls = []
        self.unet = types.SimpleNamespace(config=types.SimpleNamespace(in_channels=4, sample_size=8))

    def __call__(self, **kw):
        self.calls.append(kw)
        if 'row_seeds' not in kw:
            return types.SimpleNamespace(images=torch.full((1, 3, 4, 4), 0.5)), torch.tensor(0.25)
        seeds = kw['row_seeds']
        images = torch.stack([torch.full((3, 4, 4), (s % 256) / 255.0) for s in seeds])
        return types.SimpleNamespace(images=images), [s / 1000.0 for s in seeds]


@pytest.mark.parametrize('search_batch', [1, 2, 4])
def test_generate_sd_seeds_splits_seeds_over_ranks_like_generate_seeds(tmp_path, search_batch):
    import PIL.Image
    seeds = list(range(995, 1006))
    for world in (1, 2):
        got = {}
        for rank in range(world):
            pipe = StubPipe()
            done = bulk.generate_sd_seeds(pipe, 'a prompt', '995-1005', str(tmp_path / f'w{world}'), method='eps_greedy', params={'N': 2},
                                          search_batch=search_batch, num_inference_steps=3, score_function='scorer', decode_rows=5,
                                          rank=rank, world=world, guidance_scale=3.0)
            want = [b.tolist() for b in bulk.rank_batches(seeds, search_batch, rank, world) if len(b)]
            assert [c['row_seeds'] for c in pipe.calls] == want                        # the split of generate_seeds, one call per batch
            for c in pipe.calls:
                assert c['prompt'] == 'a prompt' and c['method'] == 'eps_greedy' and c['params'] == {'N': 2} and c['decode_rows'] == 5
                assert c['num_inference_steps'] == 3 and c['score_function'] == 'scorer' and c['guidance_scale'] == 3.0
            assert not set(done) & set(got)
            got.update(done)
        assert got == {s: s / 1000.0 for s in seeds}
        for s in seeds:
            path = tmp_path / f'w{world}' / f'{s:06d}.png'
            assert path.exists()
            assert np.array(PIL.Image.open(path))[0, 0, 0] == s % 256


def test_generate_sd_seeds_file_naming_and_mcts(tmp_path):
    pipe = StubPipe()
    done = bulk.generate_sd_seeds(pipe, 'p', [999, 1000], str(tmp_path), method='naive', subdirs=True, search_batch=2, rank=0, world=1)
    assert sorted(done) == [999, 1000]
    assert (tmp_path / '000000' / '000999.png').exists() and (tmp_path / '001000' / '001000.png').exists()       # as generate_seeds / generate_images
    assert bulk.seed_png_path(str(tmp_path), 1234, True) == os.path.join(str(tmp_path), '001000', '001234.png')
    # mcts: ragged trees, one single-search call per seed whatever the search batch; latents drawn after torch.manual_seed(seed), as main.py does
    pipe = StubPipe()
    done = bulk.generate_sd_seeds(pipe, 'p', '3-4', str(tmp_path / 'm'), method='mcts', params={'N': 2, 'S': 2}, search_batch=2, rank=0, world=1)
    assert done == {3: 0.25, 4: 0.25} and len(pipe.calls) == 2 and all('row_seeds' not in c for c in pipe.calls)
    torch.manual_seed(4)
    assert torch.equal(pipe.calls[1]['latents'], torch.randn(1, 4, 8, 8))
    assert (tmp_path / 'm' / '000003.png').exists()
    with pytest.raises(ValueError, match='search_batch'):
        bulk.generate_sd_seeds(StubPipe(), 'p', '0-3', str(tmp_path), search_batch=0)


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------------------
def test_cli_parses_the_sd_bulk_flags_and_refuses_what_means_nothing():
    import main as cli
    base = ['--backend', 'sd', '--scorer', 'brightness']
    args = cli.build_parser().parse_args(base + ['--seeds', '0-7', '--outdir', 'o', '--subdirs', '--search-batch', '4', '--decode-rows', '8'])
    assert (args.seeds, args.outdir, args.subdirs, args.search_batch, args.decode_rows) == ('0-7', 'o', True, 4, 8)
    cli.check_bulk_args(args)
    plain = cli.build_parser().parse_args(base)
    assert plain.decode_rows is None and plain.seeds is None and plain.search_batch == 1
    cli.check_bulk_args(plain)

    def refused(extra, match, backend='sd'):
        a = cli.build_parser().parse_args(['--backend', backend, '--scorer', 'brightness'] + extra)
        with pytest.raises(ValueError, match=match):
            cli.check_bulk_args(a)
    refused(['--decode-rows', '4'], '--decode-rows goes with --seeds')
    refused(['--seeds', '0-3', '--decode-rows', '0'], '--decode-rows: a positive number')
    refused(['--seeds', '0-3', '--search-batch', '0'], '--search-batch: a positive number')
    refused(['--seeds', '0-3', '--output', 'x.png'], '--output names the one image')
    refused(['--seeds', '0-3', '--decode-rows', '4'], '--decode-rows is an SD option', backend='edm')
    with pytest.raises(ValueError, match='--decode-rows goes with --seeds'):
        cli.main(base + ['--decode-rows', '4'])                     # refused before anything is loaded


# ---- bindings ------------------------------------------------------------------------------------------------------------------------------------
def test_ops_binds_both_entry_points_and_the_abi_numbers_agree():
    from diffusion_tts_amd import _lib, ops
    assert callable(ops.candidate_noise_sd_rows) and callable(ops.ddim_candidates_groups)
    assert len(_lib.SIGNATURES['dts_candidate_noise_sd_rows']) == 10 and len(_lib.SIGNATURES['dts_ddim_candidates_groups']) == 13
    header = open(os.path.join(ROOT, 'include', 'dts.h')).read()
    number = int(re.search(r'#define DTS_ABI_VERSION (\d+)', header).group(1))
    assert number == _lib.ABI_VERSION == 125
    for name in ('dts_candidate_noise_sd_rows', 'dts_ddim_candidates_groups'):
        assert re.search(rf'\bint {name}\(', header), name
    lib = _lib.load()
    assert lib.dts_version() == number
    assert hasattr(lib, 'dts_candidate_noise_sd_rows') and hasattr(lib, 'dts_ddim_candidates_groups')
    # host-side argument checks of the new entry points need no GPU: both refuse null pointers / G = 0 before any launch
    assert lib.dts_candidate_noise_sd_rows(None, None, None, None, None, 1, 1, 1, 1, None) != 0
    assert b'dts_candidate_noise_sd_rows: null pointer' in lib.dts_last_error()


def test_pipeline_refuses_by_name_without_touching_a_gpu():
    """the lock-step refusals come before any tensor moves: checked here on a pipeline object built without a device"""
    from diffusion_tts_amd.sd_pipeline import SDSearchPipeline
    pipe = SDSearchPipeline.__new__(SDSearchPipeline)
    pipe.shards = types.SimpleNamespace(solo=True, collectives=0)
    pipe.mcts_backprop = False
    kw = dict(prompt_embeds=torch.zeros(1, 77, 8), negative_prompt_embeds=torch.zeros(1, 77, 8), score_function=None, params={})
    with pytest.raises(ValueError, match="row_seeds: method 'mcts' is not supported"):
        pipe(method='mcts', row_seeds=[1, 2], **kw)
    with pytest.raises(ValueError, match='row_seeds: prompt: need 1 or 3 prompts'):
        pipe(prompt=['a', 'b'], method='naive', row_seeds=[1, 2, 3], score_function=None, params={})
    # the single call: an unknown method is named (it used to run as 'naive'), and 'rejection' is main.py's loop over N calls or row_seeds' rows
    with pytest.raises(ValueError, match="unknown method 'greedy'"):
        pipe(method='greedy', latents=torch.zeros(1, 4, 8, 8), **kw)
    with pytest.raises(ValueError, match="method 'rejection': the single call runs one trajectory .*row_seeds"):
        pipe(method='rejection', latents=torch.zeros(1, 4, 8, 8), **dict(kw, params={'N': 2}))
    pipe.shards = types.SimpleNamespace(solo=False, collectives=0)
    with pytest.raises(ValueError, match='row_seeds: candidate sharding over more than one rank is not supported'):
        pipe(method='naive', row_seeds=[1, 2], **kw)
