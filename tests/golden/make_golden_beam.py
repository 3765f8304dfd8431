#!/usr/bin/env python3
"""Golden vectors of the EDM beam search from THE REFERENCE ITSELF: its BEAM_SEARCH branch (edm/main.py:138-404) run on the CPU.

Run:  PYTHONHASHSEED=0 python tests/golden/make_golden_beam.py        (needs the reference checkout; about a minute)

The branch reads `method_params.b` and `.k`, which the reference's SamplingParams does not define (:140), so as shipped it raises
AttributeError on entry.  Here the module global `SamplingParams` is bound, for the duration of a run, to a stand-in dataclass with the
fields `b`, `k`, `scorer`; the branch then runs to the end.  Import recipe, network stand-in and loggers: make_golden.py.

Writes tests/golden/beam_golden.npz + beam_manifest.json: arrays and scalars only (no weights: the tiny networks are re-created by
diffusion_tts_amd.init and pinned by the checksums of manifest.json).

  k = 1 (any batch size): the branch is a correct greedy best-of-b-per-sigma-step search.  Cases `beam_k1_adm` (b = 4, one image, ADM) and
      `beam_k1_ddpmpp` (b = 3, two images, DDPM++): per-step rewards [S, b], the final fp64 state, the PNG array, the denoiser call and row
      counts.
  k > 1: the survivor gather (:375-379) reads every survivor from beam row `sample_idx`, whichever beam the top-k index points to.  Not
      reproduced by this project.  What the branch computes before a wrong gather can matter is still the reference's arithmetic: until
      noise enters all beams of an image are the same row.  Case `beam_k2_prefix` (k = 2, b = 2, one image) stores the rewards of the
      sigma steps up to and including the first one with gamma > 0; the manifest records that step's index.

Seeds as in make_golden.py: the first search seed for which every decision is an exact tie or has a gap >= MARGIN -- for top-k of k*b
rewards, every gap between neighbours among the best k + 1 (they fix the survivors AND their rank order).  The restatement
(tests/beam_reference.py, over the oracle's networks) is run beside every case: the number of decisions of the reference that its
reward deviation cannot decide (gap <= 4 x deviation) is recorded and must not exceed one per case.
"""
import json
import os
import sys
from dataclasses import dataclass
from typing import Any

assert os.environ.get('PYTHONHASHSEED') == '0', 'run with PYTHONHASHSEED=0 (edm/main.py:776 hashes strings)'

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                       # the import recipe, the loggers, the tiny configurations  # noqa: E402

import numpy as np                             # noqa: E402
import torch                                   # noqa: E402

from diffusion_tts_amd import init as dinit    # noqa: E402
import beam_reference as br                    # noqa: E402
from helpers import oracle_net                 # noqa: E402
from oracle import scorers as oscore           # noqa: E402

MARGIN = 4e-5                                  # make_golden.py
STEPS = 6
CHURN = dict(S_churn=40, S_min=0.05, S_max=50, S_noise=1.003)      # what mg.run_ref_search passes


@dataclass
class BeamParams:                              # stands in for SamplingParams while the branch runs: the fields it reads
    b: int = 4
    k: int = 1
    scorer: Any = None


def run_beam(net, scorer, lat, lab, b, k, seed):
    saved = mg.ref_main.SamplingParams
    mg.ref_main.SamplingParams = BeamParams
    try:
        lg, sl, png, err = mg.run_ref_search(net, scorer, lat, lab, 'BEAM_SEARCH', dict(b=b, k=k), STEPS, seed=seed)
    finally:
        mg.ref_main.SamplingParams = saved
    assert err is None, err
    return lg, sl, png


def step_rewards(sl, S, b, k):
    """the scorer is called once per beam with its b candidates (:336), beams in row order: [steps][S, k*b]"""
    calls = sl.calls[:-1]
    assert len(calls) == STEPS * S * k and all(c[1].numel() == b for c in calls)
    return [torch.cat([c[1].reshape(-1) for c in calls[i * S * k:(i + 1) * S * k]]).reshape(S, k * b).float() for i in range(STEPS)]


def decision_gaps(r, k):
    t = r.sort(dim=1, descending=True).values
    return [float(t[s, q] - t[s, q + 1]) for s in range(r.shape[0]) for q in range(min(k, r.shape[1] - 1))]


def main():
    out, cases = {}, {}
    nets = {}
    for name, cfg in mg.TINY.items():
        mod = mg.ref_edm(cfg, mg.NET_SEED)
        sd, _ = dinit.refill_degenerate(dinit.edm_state_dict(cfg, mg.NET_SEED), mg.NET_SEED)
        mg.load_refilled(mod, sd)
        nets[name] = (mod, cfg, sd, dinit.checksum(sd))
    bright = mg.ref_scorers.BrightnessScorer()
    lat_g = torch.Generator().manual_seed(99)              # make_golden.py's search inputs (edm_golden.npz: search_latents1 / 2)
    latents1 = torch.randn(1, 3, 16, 16, generator=lat_g)
    latents2 = torch.randn(2, 3, 16, 16, generator=lat_g)
    lab1, lab2 = torch.eye(10)[torch.tensor([4])], torch.eye(10)[torch.tensor([4, 8])]
    g0 = np.load(os.path.join(HERE, 'edm_golden.npz'))
    assert np.array_equal(g0['search_latents1'], latents1.numpy()) and np.array_equal(g0['search_latents2'], latents2.numpy())
    assert np.array_equal(g0['search_lab1'], lab1.numpy()) and np.array_equal(g0['search_lab2'], lab2.numpy())

    for case, netname, b, k, S in (('beam_k1_adm', 'adm_tiny', 4, 1, 1), ('beam_k1_ddpmpp', 'ddpmpp_tiny', 3, 1, 2),
                                   ('beam_k2_prefix', 'adm_tiny', 2, 2, 1)):
        mod, cfg, sd, ck = nets[netname]
        lat, lab = (latents1, lab1) if S == 1 else (latents2, lab2)
        onet = oracle_net(cfg, sd)
        t_steps = br.osamp.sigma_schedule(onet, STEPS)
        gam = br.gammas(t_steps, STEPS, CHURN['S_churn'], CHURN['S_min'], CHURN['S_max'])
        first_noisy = next(i for i, g in enumerate(gam) if g > 0)
        keep = STEPS if k == 1 else first_noisy + 1        # k > 1: the steps before a wrong gather can matter
        for seed in range(64):
            lg, sl, png = run_beam(mod, bright, lat, lab, b, k, seed)
            rew = step_rewards(sl, S, b, k)
            gaps = [g for r in rew[:keep] for g in decision_gaps(r, k)]
            if all(g == 0 or g >= MARGIN for g in gaps):
                break
        else:
            raise RuntimeError(f'{case}: no seed with safe decision margins')
        # the restatement beside it (B = k, N = b)
        mine = br.beam_search(onet, lat, lab, B=k, N=b, scorer=oscore.BrightnessOracle(), seed=seed, num_steps=STEPS, stop_after=keep, **CHURN)
        undecided, max_dev = 0, 0.0
        for i in range(keep):
            dev = float((mine['rewards'][i] - rew[i]).abs().max())
            max_dev = max(max_dev, dev)
            open_here = sum(1 for g in decision_gaps(rew[i], k) if 0 < g <= 4 * dev)
            undecided += open_here
            assert open_here or torch.equal(mine['selected'][i], br.select(rew[i], k)), (case, i)
        assert undecided <= 1, (case, undecided)
        meta = dict(net=netname, scorer='brightness', b=b, k=k, B=k, N=b, batch=S, num_steps=STEPS, seed=seed, steps_stored=keep,
                    first_noisy_step=first_noisy, gammas=gam, sigmas=[float(t) for t in t_steps],
                    min_gap=min([g for g in gaps if g > 0], default=None), exact_ties=sum(1 for g in gaps if g == 0),
                    restatement_max_reward_dev=max_dev, undecidable_vs_restatement=undecided, checksum=ck, **CHURN)
        out[f'{case}_rewards'] = torch.stack(rew[:keep]).numpy()                       # [steps, S, k*b] float32
        if k == 1:
            calls = lg.calls
            meta.update(net_calls=len(calls), net_rows=int(sum(c[0].shape[0] for c in calls)), scorer_calls=len(sl.calls))
            assert meta['net_rows'] == S * k * b * (2 * STEPS - 1)
            # the final state: the last step's calls are one per beam (x_hat [b rows], t_hat, D); x_next = x_hat + (0 - t_hat) * d_cur (:88-89)
            last = calls[-S:]
            win = rew[-1].argmax(dim=1)
            rows = []
            for s in range(S):
                x_hat, t_hat, D = last[s][0], last[s][1].to(torch.float64), last[s][2].to(torch.float64)
                assert x_hat.shape[0] == b and x_hat.dtype == torch.float64
                d_cur = (x_hat - D) / t_hat
                rows.append((x_hat + (torch.zeros((), dtype=torch.float64) - t_hat) * d_cur)[int(win[s])])
            x_final = torch.stack(rows)
            img = (x_final * 127.5 + 128).clip(0, 255).to(torch.uint8)
            grid = img.reshape(1, S, *img.shape[1:]).permute(0, 3, 1, 4, 2).reshape(16, S * 16, 3).numpy()
            assert np.array_equal(grid, png), case                                    # the state rebuilt here IS what the reference wrote
            out[f'{case}_x_final'], out[f'{case}_image'] = x_final.numpy(), png
            out[f'{case}_final_score'] = sl.calls[-1][1].numpy()
            full = br.beam_search(onet, lat, lab, B=k, N=b, scorer=oscore.BrightnessOracle(), seed=seed, num_steps=STEPS, **CHURN)
            meta['restatement_x_err'] = float((full['x'] - x_final).abs().max())
        cases[case] = meta
        print(case, {k_: v for k_, v in meta.items() if k_ not in ('checksum',)}, flush=True)

    np.savez_compressed(os.path.join(HERE, 'beam_golden.npz'), **out)
    manifest = {'torch': torch.__version__, 'numpy': np.__version__, 'python': sys.version.split()[0], 'margin': MARGIN,
                'latent_generator_seed': 99, 'label_idx': {'1': [4], '2': [4, 8]}, 'cases': cases}
    with open(os.path.join(HERE, 'beam_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, default=lambda o: o.item() if isinstance(o, (np.floating, np.integer)) else o)
    print('wrote', len(out), 'arrays;', os.path.getsize(os.path.join(HERE, 'beam_golden.npz')), 'bytes')


if __name__ == '__main__':
    main()
