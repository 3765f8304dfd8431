"""GPU: the SD backend's lock-step searches -- SDSearchPipeline(row_seeds=[s0, s1, ...]) -- against `oracle.sd_loop.sd_search` run ONE SEED AT A
TIME on the CPU (never against this build's own batched run).

Settings: TinyUNet / TinyVAE (tests/sd_standins.py), embeddings [1,77,8] from torch.Generator().manual_seed(11) (positive first, then
negative), 8x8 float32 latents, 4 steps, guidance 7.5, eta 1, the list-brightness scorer of tests/test_oracle_sd_golden.py.  The oracle's seed
s is `torch.manual_seed(s); lat = torch.randn(1, 4, 8, 8)` and then the global stream; the lock-step call gets `latents=None` and draws the
same from its per-seed generator.

Bounds (tests/test_gpu_sd.py's): scores and final image within 2e-5 of the oracle.  A decision is CHECKABLE only when its deciding gap in the
oracle's scores exceeds 4e-5 = 2 x that bound -- eps-greedy / zero-order: best against second best of every iteration; beam: ranks 1|2 and
B|B+1 of every timestep and the two final beams; rejection: best against second best -- and every test ASSERTS that every decision of every
seed it uses is checkable, so nothing passes by being left out.  Seeds (scanned on the CPU with the oracle at exactly these settings):
  eps-greedy (N=3, K=2, lambda=0.15, eps=0.4): 33, 34, 39 (smallest gap 4.9e-5); most other seeds of 0..39 have sub-margin decisions.
  beam (B=2, N=3): 4, 11, 15, 33 (smallest gap 4.2e-5 with the final pair counted).
  zero-order (N=3, K=2): every candidate is a short step from the pivot, so the gaps scale with lambda; at lambda=0.15 NO seed of 0..599 has
    all 8 decisions above the margin (best: 3.0e-5).  The test therefore runs zero-order at lambda=1.0: seeds 61, 85, 98, 112 (>= 5.7e-5).
  rejection (N=3): 1, 4, 5 (gaps > 2e-2); naive makes no decision: 1, 2, 3.
Against this build's own solo run (`row_seeds=[s]`) the selections are identical and the values within 4e-5 (both are within 2e-5 of the
oracle).  The single call (`pipe(latents=[1,...])` after torch.manual_seed(s)) IS the one-seed lock-step call on the global generator: equal
bit for bit, and it leaves the global generator where the oracle leaves it."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sd_standins import TinyUNet, TinyVAE                  # noqa: E402
from test_oracle_sd_golden import ListBrightness           # noqa: E402
from oracle.sd_loop import DDIMOracle, sd_search           # noqa: E402

DEV = 'cuda'
STEPS, BOUND, MARGIN = 4, 2e-5, 4e-5
PARAMS = {'eps_greedy': {'N': 3, 'K': 2, 'lambda': 0.15, 'eps': 0.4}, 'zero_order': {'N': 3, 'K': 2, 'lambda': 1.0, 'eps': 0.4},
          'beam': {'B': 2, 'N': 3}, 'naive': {}, 'rejection': {'N': 3}}
SEEDS = {'eps_greedy': [33, 34, 39], 'zero_order': [61, 85, 98, 112], 'beam': [4, 11, 15, 33], 'naive': [1, 2, 3], 'rejection': [1, 4, 5]}
METHODS = list(SEEDS)


def embeddings(seed=11):
    g = torch.Generator().manual_seed(seed)
    pe = torch.randn(1, 77, 8, generator=g)
    return pe, torch.randn(1, 77, 8, generator=g)


PE, NE = embeddings()
PE2, NE2 = embeddings(12)                                 # a second prompt
_ORACLE = {}


def oracle(method, seed, pe=PE, ne=NE, tag=0):
    """the reference loop for ONE seed on the CPU, computed once per (method, seed, prompt) and shared"""
    key = (method, seed, tag)
    if key not in _ORACLE:
        unet, vae = TinyUNet(), TinyVAE()                 # constructors touch the global RNG: build before seeding
        torch.manual_seed(seed)
        runs = []
        for _ in range(PARAMS[method]['N'] if method == 'rejection' else 1):          # the reference's main.py:134 loop
            lat = torch.randn(1, 4, 8, 8)
            runs.append(sd_search(unet, vae, DDIMOracle(), pe, ne, lat, num_inference_steps=STEPS, score_function=ListBrightness(),
                                  method='naive' if method == 'rejection' else method, params=PARAMS[method]))
        finals = [float(r['max_score']) for r in runs]
        best = runs[finals.index(max(finals))]
        _ORACLE[key] = dict(scores=[v for r in runs for v in r['scores']], unet_rows=sum(r['unet_rows'] for r in runs), max_score=max(finals),
                            image=(best['image'] / 2 + 0.5).clamp(0, 1), rng_state=torch.get_rng_state())
    return _ORACLE[key]


def decisions(method, scores):
    """(selections, deciding gaps) that a list of rewards implies under the loop's rules: first maximum, stable sort"""
    p = PARAMS[method]
    sel, gaps = [], []
    if method in ('eps_greedy', 'zero_order'):
        for i in range(0, len(scores), p['N']):
            v = scores[i:i + p['N']]
            top = sorted(v, reverse=True)
            sel.append(v.index(top[0]))
            gaps.append(top[0] - top[1])
    elif method == 'beam':
        B, per = p['B'], p['B'] * p['N']
        body, fin = scores[:-B], scores[-B:]
        for i in range(0, len(body), per):
            v = body[i:i + per]
            order = sorted(range(per), key=lambda k: v[k], reverse=True)
            sel.append(tuple(order[:B]))
            gaps += [v[order[0]] - v[order[1]], v[order[B - 1]] - v[order[B]]]
        top = sorted(fin, reverse=True)
        sel.append(fin.index(top[0]))
        gaps.append(top[0] - top[1])
    elif method == 'rejection':
        top = sorted(scores, reverse=True)
        sel.append(scores.index(top[0]))
        gaps.append(top[0] - top[1])
    return sel, gaps


@pytest.fixture(scope='module')
def pipe():
    from diffusion_tts_amd.sd_pipeline import SDSearchPipeline
    return SDSearchPipeline(TinyUNet().to(DEV), TinyVAE().to(DEV), device=DEV)


def run(pipe, method, seeds, pe=PE, ne=NE, **kw):
    return pipe(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=STEPS, score_function=ListBrightness(), method=method,
                params=PARAMS[method], row_seeds=seeds, output_type='pt', **kw)


_BATCH = {}


def batch(pipe, method):
    """the undivided lock-step run of the method's seeds, computed once and shared"""
    if method not in _BATCH:
        _BATCH[method] = run(pipe, method, SEEDS[method])
    return _BATCH[method]


def assert_close_to_oracle(method, seed, search, want):
    got, ref = np.array(search.scores), np.array(want['scores'])
    assert got.shape == ref.shape, (method, seed, got.shape, ref.shape)
    err_s = float(np.abs(got - ref).max())
    err_i = float((search.images.float().cpu() - want['image']).abs().max())
    print(f'{method} seed {seed}: {len(got)} scores, max |score - oracle| {err_s:.2e}, max |image - oracle| {err_i:.2e}')
    assert err_s < BOUND and err_i < BOUND, (method, seed, err_s, err_i)
    assert abs(float(search.max_score) - want['max_score']) < BOUND
    assert decisions(method, search.scores)[0] == decisions(method, want['scores'])[0], (method, seed)


@pytest.mark.parametrize('method', METHODS)
def test_every_decision_of_every_seed_is_checkable(method):
    for seed in SEEDS[method]:
        sel, gaps = decisions(method, oracle(method, seed)['scores'])
        print(f'{method} seed {seed}: {len(gaps)} deciding gaps, smallest {min(gaps, default=float("inf")):.2e}')
        assert all(gp > MARGIN for gp in gaps), (method, seed, min(gaps))
        assert method == 'naive' or len(sel) > 0


@pytest.mark.parametrize('method', METHODS)
def test_lockstep_batch_matches_the_oracle_seed_by_seed(pipe, method):
    seeds = SEEDS[method]
    out, max_scores = batch(pipe, method)
    assert len(out.searches) == len(seeds) and out.row_seeds == seeds and tuple(out.images.shape) == (len(seeds), 3, 16, 16)
    wants = [oracle(method, s) for s in seeds]
    for k, (seed, want) in enumerate(zip(seeds, wants)):
        assert_close_to_oracle(method, seed, out.searches[k], want)
        assert float(max_scores[k]) == float(out.searches[k].max_score)
        assert torch.equal(out.searches[k].latents, out.latents[k:k + 1]) and out.scores[k] is out.searches[k].scores
    # the counts: lock-step searches do equal work, so the totals are the oracle's per-seed counts times the batch
    assert out.unet_rows == sum(w['unet_rows'] for w in wants) and out.unet_rows % len(seeds) == 0
    scored = sum(len(w['scores']) for w in wants)
    assert out.scorer_calls == scored                                         # ListBrightness is not `batched`: one call per image, as the oracle
    assert out.decoded == scored - (len(seeds) * PARAMS[method].get('N', 1) if method in ('naive', 'rejection') else 0)
    assert out.collectives == 0


@pytest.mark.parametrize('method', METHODS)
def test_a_seed_in_a_batch_equals_its_solo_runs(pipe, method):
    """row_seeds=[s] alone: identical selections, values within 4e-5; the single call after torch.manual_seed(s): equal to row_seeds=[s]"""
    out, _ = batch(pipe, method)
    for k, seed in enumerate(SEEDS[method][:2]):
        solo, solo_max = run(pipe, method, [seed])
        assert decisions(method, solo.scores[0])[0] == decisions(method, out.scores[k])[0]
        assert float(np.abs(np.array(solo.scores[0]) - np.array(out.scores[k])).max()) < MARGIN
        assert float((solo.images - out.images[k:k + 1]).abs().max()) < MARGIN
        assert solo.unet_rows * len(SEEDS[method]) == out.unet_rows and solo.decoded * len(SEEDS[method]) == out.decoded
        if method == 'rejection':
            continue                                                          # (the single-search call has no rejection loop: main.py's)
        torch.manual_seed(seed)
        lat = torch.randn(1, 4, 8, 8)
        one, one_max = pipe(prompt_embeds=PE, negative_prompt_embeds=NE, latents=lat, num_inference_steps=STEPS, score_function=ListBrightness(),
                            method=method, params=PARAMS[method], output_type='pt')
        assert one.scores == solo.scores[0]
        assert torch.equal(one.images, solo.images)
        assert float(one_max) == float(solo_max[0])
        assert one.unet_rows == solo.unet_rows and one.decoded == solo.decoded


def assert_same_search(one, one_max, solo, solo_max):
    """the single call's result against the one-seed lock-step call's: the same search, bit for bit, counted alike"""
    assert one.scores == solo.scores[0]
    assert torch.equal(one.latents, solo.latents) and torch.equal(one.images, solo.images)
    assert isinstance(one_max, float) and float(one_max) == float(solo_max[0])
    assert (one.unet_rows, one.decoded, one.scorer_calls) == (solo.unet_rows, solo.decoded, solo.scorer_calls)
    assert sorted(vars(one)) == ['collectives', 'decoded', 'images', 'latents', 'nsfw_content_detected', 'scorer_calls', 'scores', 'unet_rows']


@pytest.mark.parametrize('method', ['naive', 'eps_greedy', 'zero_order', 'beam'])
def test_the_single_call_is_the_one_seed_lockstep_call(pipe, method):
    """`torch.manual_seed(s); pipe(...)` without row_seeds is `pipe(row_seeds=[s], ...)` on the global generator, bit for bit, in each form
    of passing the latents.  A seed's stream starts with main.py's latent draw unless the lock-step call is GIVEN latents (then it starts
    at the loop's first draw, test_latents_given_per_seed), so each single call is paired with the lock-step call whose stream it is:
      main.py's call -- seed, draw `lat`, pipe(latents=lat) -- with row_seeds=[s] drawing the same latents itself;
      seed, pipe(latents=lat) with row_seeds=[s], latents=lat (no latent draw on either stream);
      seed, pipe(latents=None) with row_seeds=[s] (the stand-in U-Net is float32, so prepare_latents' draw is main.py's float32 draw).
    The single call leaves the global generator where the oracle's run from the same seed and latents leaves it: the count of draws, the
    dropped variance noises after the last decision included, which no score can see."""
    kw = dict(prompt_embeds=PE, negative_prompt_embeds=NE, num_inference_steps=STEPS, score_function=ListBrightness(), method=method,
              params=PARAMS[method], output_type='pt')
    for seed in SEEDS[method][:2]:
        want = oracle(method, seed)
        drawing = run(pipe, method, [seed])
        torch.manual_seed(seed)
        lat = torch.randn(1, 4, 8, 8)
        one, one_max = pipe(latents=lat.clone(), **kw)
        assert torch.equal(torch.get_rng_state(), want['rng_state']), (method, seed)
        assert_same_search(one, one_max, *drawing)
        torch.manual_seed(seed)
        given, given_max = pipe(latents=lat.clone(), **kw)
        assert_same_search(given, given_max, *run(pipe, method, [seed], latents=lat.clone()))
        torch.manual_seed(seed)
        drawn, drawn_max = pipe(latents=None, **kw)
        assert torch.equal(torch.get_rng_state(), want['rng_state']), (method, seed)
        assert_same_search(drawn, drawn_max, *drawing)


@pytest.mark.parametrize('method', METHODS)
def test_decode_rows_changes_no_selection(pipe, method):
    out, _ = batch(pipe, method)
    cut, _ = run(pipe, method, SEEDS[method], decode_rows=2)
    for k, seed in enumerate(SEEDS[method]):
        assert decisions(method, cut.scores[k])[0] == decisions(method, out.scores[k])[0], (method, seed)
        assert_close_to_oracle(method, seed, cut.searches[k], oracle(method, seed))
    assert (cut.unet_rows, cut.decoded, cut.scorer_calls) == (out.unet_rows, out.decoded, out.scorer_calls)


@pytest.mark.parametrize('method', ['eps_greedy', 'beam'])
def test_latents_given_per_seed(pipe, method):
    """latents [S,C,H,W] given: the streams start at the loop's first draw, i.e. seed s continues as the global generator does after
    torch.manual_seed(s) WITHOUT main.py's latent draw -- the unchanged single-search call with the same latents is the yardstick"""
    seeds = SEEDS[method][:2]
    lat = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(5))
    out, _ = run(pipe, method, seeds, latents=lat)
    for k, seed in enumerate(seeds):
        torch.manual_seed(seed)
        one, _ = pipe(prompt_embeds=PE, negative_prompt_embeds=NE, latents=lat[k:k + 1].clone(), num_inference_steps=STEPS,
                      score_function=ListBrightness(), method=method, params=PARAMS[method], output_type='pt')
        assert len(one.scores) == len(out.scores[k])
        assert float(np.abs(np.array(one.scores[:PARAMS[method]['N']]) - np.array(out.scores[k][:PARAMS[method]['N']])).max()) < MARGIN


def test_two_prompts_in_one_batch(pipe):
    """searches 0 and 2 under one embedding pair, search 1 under another: each equals the oracle's run of its seed under ITS prompt and its
    own solo run.  Seed 77 is checkable under the second pair (scanned like the others: smallest gap 1.4e-4), asserted here."""
    method, seeds = 'eps_greedy', [33, 77, 34]
    wants = [oracle(method, seeds[0]), oracle(method, seeds[1], PE2, NE2, tag=1), oracle(method, seeds[2])]
    assert all(gp > MARGIN for w in wants for gp in decisions(method, w['scores'])[1])
    mixed, _ = run(pipe, method, seeds, pe=torch.cat([PE, PE2, PE]), ne=torch.cat([NE, NE2, NE]))
    for k, seed in enumerate(seeds):
        assert_close_to_oracle(method, seed, mixed.searches[k], wants[k])
    solo, _ = run(pipe, method, [seeds[1]], pe=PE2, ne=NE2)
    assert decisions(method, solo.scores[0])[0] == decisions(method, mixed.scores[1])[0]
    assert float(np.abs(np.array(solo.scores[0]) - np.array(mixed.scores[1])).max()) < MARGIN
    # the prompt matters by more than both runs' bounds together, so a search under the wrong pair could not have passed above
    other = oracle(method, seeds[1])
    assert float(np.abs(np.array(other['scores']) - np.array(wants[1]['scores'])).max()) > 2 * BOUND


class RecordingUNet:
    """a U-Net that announces `takes_context_rows` and records what the loop hands it"""
    takes_context_rows = True

    def __init__(self, inner):
        self.inner, self.config, self.calls = inner, inner.config, []

    dtype = torch.float32

    def __call__(self, sample, t, encoder_hidden_states=None, context_rows=None, return_dict=False):
        self.calls.append((sample.shape[0], tuple(encoder_hidden_states.shape), context_rows))
        return self.inner(sample, t, encoder_hidden_states=encoder_hidden_states[context_rows.long()], return_dict=False)


def test_a_unet_that_takes_context_rows_gets_the_distinct_contexts_and_a_map():
    from diffusion_tts_amd.sd_pipeline import SDSearchPipeline
    rec = RecordingUNet(TinyUNet().to(DEV))
    p = SDSearchPipeline(rec, TinyVAE().to(DEV), device=DEV)
    method, seeds = 'eps_greedy', SEEDS['eps_greedy']
    n = PARAMS[method]['N']
    out, _ = run(p, method, seeds, pe=torch.cat([PE, PE2, PE]), ne=torch.cat([NE, NE2, NE]))
    assert rec.calls and sum(c[0] for c in rec.calls) == out.unet_rows
    maps = {}
    for rows, ehs_shape, cmap in rec.calls:
        assert ehs_shape == (6, 77, 8), ehs_shape                                 # 3 negative + 3 positive contexts, never the 2*S*N expanded tensor
        assert cmap.dtype == torch.int32 and cmap.is_cuda and tuple(cmap.shape) == (rows,)
        per = rows // 2 // len(seeds)
        assert per in (1, n)
        own = [r // per for r in range(rows // 2)]
        assert cmap.tolist() == own + [3 + c for c in own]
        maps.setdefault(rows, cmap)
        assert cmap is maps[rows]                                                 # built once per (rows, prompts)
    mixed, _ = run(SDSearchPipeline(TinyUNet().to(DEV), TinyVAE().to(DEV), device=DEV), method, seeds, pe=torch.cat([PE, PE2, PE]),
                   ne=torch.cat([NE, NE2, NE]))
    assert mixed.scores == out.scores                                             # same rows through the same module either way
    # one shared prompt: the two distinct contexts
    rec.calls.clear()
    run(p, method, seeds)
    assert all(shape == (2, 77, 8) for _, shape, _ in rec.calls)


def test_row_map_equals_expanded_contexts_on_the_hip_unet():
    """The lock-step path through a small SDUNet (the narrow configuration of tests/test_gpu_sd_unet.py, float16): the distinct contexts with
    the row map against the same run with `takes_context_rows` hidden (expanded contexts, grouped on the device by the U-Net itself): bit
    for bit, as tests/test_gpu_sd_unet_ops.py holds the map to the expanded form."""
    import json
    import os
    from conftest import ROOT
    from diffusion_tts_amd import init as dinit
    from diffusion_tts_amd.sd_pipeline import SDSearchPipeline
    from diffusion_tts_amd.sd_unet import SDUNet
    with open(os.path.join(ROOT, 'tests', 'golden', 'sd_unet_manifest.json')) as f:
        c = json.load(f)['cases']['narrow']
    boc = tuple(c['block_out_channels'])
    unet = SDUNet(dinit.sd_unet_state_dict(boc, c['heads'], c['cross_attention_dim'], 2, seed=c['seed']), device=DEV, dtype=torch.float16,
                  block_out_channels=boc, attention_head_dim=c['heads'], cross_attention_dim=c['cross_attention_dim'], layers_per_block=2,
                  sample_size=c['latent'][-1])

    class Hidden:                                                                 # the same model without the announcement
        def __init__(self, inner):
            self.inner, self.config, self.dtype = inner, inner.config, inner.dtype

        def __call__(self, sample, t, encoder_hidden_states=None, return_dict=False):
            return self.inner(sample, t, encoder_hidden_states=encoder_hidden_states, return_dict=False)

    g = torch.Generator().manual_seed(13)
    pe = torch.randn(2, c['context_len'], c['cross_attention_dim'], generator=g)
    ne = torch.randn(2, c['context_len'], c['cross_attention_dim'], generator=g)
    vae = TinyVAE().to(DEV).half()
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=2, score_function=ListBrightness(), method='eps_greedy',
              params={'N': 3, 'K': 1, 'lambda': 0.15, 'eps': 0.4}, row_seeds=[33, 34], output_type='pt')
    a, _ = SDSearchPipeline(unet, vae, device=DEV)(**kw)
    b, _ = SDSearchPipeline(Hidden(unet), vae, device=DEV)(**kw)
    assert a.unet_rows == b.unet_rows == 2 * (2 * 2 + 2 * 2 * 3)
    assert bool(torch.isfinite(a.images).all()) and a.scores == b.scores
    assert torch.equal(a.images, b.images) and torch.equal(a.latents, b.latents)


def test_refusals(pipe):
    kw = dict(prompt_embeds=PE, negative_prompt_embeds=NE, num_inference_steps=STEPS, score_function=ListBrightness())
    from diffusion_tts_amd.sd_pipeline import SDSearchPipeline
    for backprop in (False, True):
        p = SDSearchPipeline(pipe.unet, pipe.vae, device=DEV, mcts_backprop=backprop)
        with pytest.raises(ValueError, match="row_seeds: method 'mcts' is not supported"):
            p(method='mcts', params={'N': 2, 'S': 2}, row_seeds=[1, 2], **kw)
    with pytest.raises(ValueError, match='row_seeds: prompt: need 1 or 3 prompts'):
        pipe(prompt=['a', 'b'], num_inference_steps=STEPS, score_function=ListBrightness(), method='naive', params={}, row_seeds=[1, 2, 3])
    with pytest.raises(ValueError, match='row_seeds: prompt_embeds: need 1 or 3 rows'):
        pipe(method='naive', params={}, row_seeds=[1, 2, 3], **dict(kw, prompt_embeds=torch.cat([PE, PE2]), negative_prompt_embeds=torch.cat([NE, NE2])))
    with pytest.raises(ValueError, match=r'row_seeds: latents: need \[3, C, H, W\]'):
        pipe(method='naive', params={}, row_seeds=[1, 2, 3], latents=torch.zeros(2, 4, 8, 8), **kw)
    with pytest.raises(ValueError, match="row_seeds: method 'rejection' draws the latents"):
        pipe(method='rejection', params={'N': 2}, row_seeds=[1], latents=torch.zeros(1, 4, 8, 8), **kw)
    with pytest.raises(ValueError, match='decode_rows: a positive number'):
        pipe(method='naive', params={}, row_seeds=[1], decode_rows=0, **kw)
    with pytest.raises(ValueError, match='decode_rows goes with row_seeds'):
        pipe(method='naive', params={}, latents=torch.zeros(1, 4, 8, 8), decode_rows=2, **kw)
    sharded = SDSearchPipeline(pipe.unet, pipe.vae, device=DEV)
    sharded.shards = types.SimpleNamespace(solo=False, world=2, rank=0, collectives=0)          # a rank of a two-rank candidate-sharded world
    with pytest.raises(ValueError, match='row_seeds: candidate sharding over more than one rank is not supported'):
        sharded(method='naive', params={}, row_seeds=[1, 2], **kw)
