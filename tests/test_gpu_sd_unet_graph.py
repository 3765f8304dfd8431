"""GPU: the SD U-Net's forward behind graphs.GraphCache (sd_unet.SDUNet._device_forward captured once per shape and replayed), the grouping
of its text contexts on the device, and the `context_rows=` keyword that hands it the distinct contexts and a row map.

Replay launches the very kernels of the eager forward on the same values, so every comparison between the two is bit for bit
(torch.equal); only the golden comparison has a tolerance, the one of tests/test_gpu_sd_unet.py (manifest tolerance_factor x own_error).
All at the `narrow` case of tests/golden/sd_unet_manifest.json, 16x16 latents, six rows where the rows are ours to choose (two contexts
three times each, the cond / uncond halves of a search step)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ROOT                                        # noqa: E402
from diffusion_tts_amd import init as dinit                      # noqa: E402

DEV = 'cuda'
DT = {'float16': torch.float16, 'bfloat16': torch.bfloat16}


@pytest.fixture(scope='module')
def gold():
    with open(os.path.join(ROOT, 'tests', 'golden', 'sd_unet_manifest.json')) as f:
        return np.load(os.path.join(ROOT, 'tests', 'golden', 'sd_unet_golden.npz')), json.load(f)


def narrow_unet(gold, dtype=torch.float16):
    from diffusion_tts_amd.sd_unet import SDUNet
    c = gold[1]['cases']['narrow']
    sd = dinit.sd_unet_state_dict(tuple(c['block_out_channels']), c['heads'], c['cross_attention_dim'], 2, seed=c['seed'])
    return SDUNet(sd, device=DEV, dtype=dtype, block_out_channels=tuple(c['block_out_channels']), attention_head_dim=c['heads'],
                  cross_attention_dim=c['cross_attention_dim'], layers_per_block=2, sample_size=16), c


def inputs(c, seed, distinct=2, rows=6):
    """(sample [rows,4,16,16], the `distinct` contexts [distinct, L, cd], the row map as a list): float16 on the device"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, 4, 16, 16, generator=g).to(DEV, torch.float16)
    ctx = torch.randn(distinct, c['context_len'], c['cross_attention_dim'], generator=g).to(DEV, torch.float16)
    rmap = [i * distinct // rows for i in range(rows)]
    return x, ctx, rmap


def expand(ctx, rmap):
    return ctx[torch.tensor(rmap, device=ctx.device)].contiguous()


def eager(unet, *args, **kw):
    unet._graphs.enabled = False
    try:
        return unet(*args, **kw)[0]
    finally:
        unet._graphs.enabled = True


def test_replay_is_bit_identical_to_eager(gold):
    unet, c = narrow_unet(gold)
    assert unet._graphs.enabled
    calls = []
    for i in range(5):
        x, ctx, rmap = inputs(c, 100 + i)
        t = 900 - 170 * i
        calls.append((x, t, expand(ctx, rmap), unet(x, t, encoder_hidden_states=expand(ctx, rmap), return_dict=False)[0]))
    assert unet._graphs.captures == 1 and unet._graphs.replays >= 2, unet._graphs.path_report()
    for x, t, ehs, got in calls:
        assert got.dtype == torch.float16 and tuple(got.shape) == (6, 4, 16, 16) and torch.isfinite(got).all()
        assert torch.equal(got, eager(unet, x, t, encoder_hidden_states=ehs, return_dict=False))
    assert not torch.equal(calls[3][3], calls[4][3])             # the replays did read their own inputs
    assert unet.rows == 6 * 10
    assert unet._graphs.captures == 1


@pytest.mark.parametrize('dname', ['float16', 'bfloat16'])
def test_golden_comparison_holds_on_replay(gold, dname):
    vg, man = gold
    unet, c = narrow_unet(gold, DT[dname])
    x, ctx, t, want = (torch.from_numpy(vg[f'narrow_{k}']) for k in ('x', 'context', 't', 'y'))
    for _ in range(4):
        got = unet(x.to(DEV, DT[dname]), t.to(DEV), encoder_hidden_states=ctx.to(DEV, DT[dname]), return_dict=False)[0]
    assert unet._graphs.captures == 1 and unet._graphs.replays >= 2, unet._graphs.path_report()
    tol = man['tolerance_factor'] * c['own_error'][dname]
    err = float((got.double().cpu() - want.double()).abs().max() / want.double().abs().max())
    print(f'SDUNet narrow {dname}, replayed: rel. max err {err:.3e} (tolerance {tol:.3e})')
    assert err < tol, (err, tol)


def test_context_rows_gives_the_same_result_without_a_synchronisation(gold):
    unet, c = narrow_unet(gold)
    x, ctx, rmap = inputs(c, 7)
    assert rmap == [0, 0, 0, 1, 1, 1]
    want = unet(x, 500, encoder_hidden_states=expand(ctx, rmap), return_dict=False)[0]
    got = unet(x, 500, encoder_hidden_states=ctx, context_rows=rmap, return_dict=False)[0]
    assert torch.equal(got, want)
    rows_dev = torch.tensor(rmap, dtype=torch.int32).to(DEV)
    t_dev = torch.full((6,), 500.0, device=DEV)
    got = unet(x, t_dev, encoder_hidden_states=ctx, context_rows=rows_dev, return_dict=False)[0]     # third sighting: captured
    assert torch.equal(got, want) and unet._graphs.captures == 1
    x2, ctx2, _ = inputs(c, 8)
    want2 = eager(unet, x2, 500, encoder_hidden_states=expand(ctx2, rmap), return_dict=False)
    replays = unet._graphs.replays
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode('error')
        got2 = unet(x2, t_dev, encoder_hidden_states=ctx2, context_rows=rows_dev, return_dict=False)[0]
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert unet._graphs.replays == replays + 1 and unet._graphs.captures == 1
    assert torch.equal(got2, want2)


def test_changing_the_number_of_distinct_contexts(gold):
    """one, two and six distinct contexts among six rows: each count has its own graph, and no call is answered by another count's"""
    unet, c = narrow_unet(gold)
    seed = 0
    for distinct in (2, 2, 2, 1, 1, 1, 2, 1, 2, 6, 6, 6, 6, 1, 2):
        seed += 1
        x, ctx, rmap = inputs(c, 40 + seed, distinct)
        ehs = expand(ctx, rmap)
        got = unet(x, 321, encoder_hidden_states=ehs, return_dict=False)[0]
        assert torch.equal(got, eager(unet, x, 321, encoder_hidden_states=ehs, return_dict=False)), (seed, distinct)
    G = unet._graphs
    assert G.captures == 3 and sorted(key[2][0][0] for key in G.graphs) == [1, 2, 6], G.path_report()
    assert G.replays == 15 - 3 * 2                               # everything after the two eager sightings of each count


def test_the_pipeline_passes_the_row_map(gold, monkeypatch):
    from diffusion_tts_amd import ops
    from diffusion_tts_amd.sd_pipeline import SDSearchPipeline
    unet, c = narrow_unet(gold)
    x, ctx, _ = inputs(c, 21, rows=3)
    eu, ec = ctx[:1].contiguous(), ctx[1:].contiguous()
    t = torch.tensor(481)                                        # a 0-d host tensor, as the loop's timesteps are
    calls = []
    real = ops.group_rows
    monkeypatch.setattr(ops, 'group_rows', lambda v: (calls.append(tuple(v.shape)), real(v))[1])
    pipe = SDSearchPipeline(unet, None, device=DEV)
    got = pipe._eps_rows(x, t, eu, ec, [0], 3, 7.5)
    assert calls == [] and pipe.unet_rows == 6 and unet.rows == 6
    assert list(pipe._context_rows) == [3] and pipe._context_rows[3].tolist() == [0, 0, 0, 1, 1, 1]
    out = unet(torch.cat([x, x]), t, encoder_hidden_states=torch.cat([eu.expand(3, -1, -1), ec.expand(3, -1, -1)]), return_dict=False)[0]
    assert calls == [(6, c['context_len'], c['cross_attention_dim'])]        # the stock surface does group (and the counter does count)
    assert torch.equal(got, ops.cfg_combine(out[:3].contiguous(), out[3:].contiguous(), 7.5))
    assert pipe._eps_rows(x, t, eu, ec, [0], 3, 7.5) is not None and len(pipe._context_rows) == 1      # the map is built once per n

    class Plain:                                                 # a U-Net without the keyword: the expanded tensor, as before
        dtype, seen = torch.float16, []

        def __call__(self, sample, timestep, encoder_hidden_states=None, return_dict=False, **kw):
            self.seen.append((tuple(sample.shape), tuple(encoder_hidden_states.shape), sorted(kw)))
            self.ehs = encoder_hidden_states
            return (sample,)
    plain = Plain()
    SDSearchPipeline(plain, None, device=DEV)._eps_rows(x, t, eu, ec, [0], 3, 7.5)
    assert plain.seen == [((6, 4, 16, 16), (6, c['context_len'], c['cross_attention_dim']), [])]
    assert torch.equal(plain.ehs[:3], eu.expand(3, -1, -1)) and torch.equal(plain.ehs[3:], ec.expand(3, -1, -1))


def test_context_rows_refusals(gold):
    unet, c = narrow_unet(gold)
    assert unet.takes_context_rows is True
    x, ctx, rmap = inputs(c, 9)
    with pytest.raises(ValueError):
        unet(x, 500, encoder_hidden_states=ctx, context_rows=rmap[:5], return_dict=False)                           # wrong length
    with pytest.raises(ValueError):
        unet(x, 500, encoder_hidden_states=ctx, context_rows=torch.tensor(rmap, device=DEV), return_dict=False)     # int64
    with pytest.raises(ValueError):
        unet(x, 500, encoder_hidden_states=inputs(c, 9, distinct=7, rows=7)[1], context_rows=rmap, return_dict=False)      # G > n
    with pytest.raises(ValueError):
        unet(x, 500, encoder_hidden_states=ctx, context_rows=rmap, class_labels=torch.zeros(6), return_dict=False)
    assert unet.rows == 0
