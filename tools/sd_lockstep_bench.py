#!/usr/bin/env python3
"""Measurement of the SD backend's lock-step searches (SDSearchPipeline(row_seeds=...)): searches per second for the same seeds run as
sequential single-search `pipe()` calls (the loop's one-search case on the global generator), as `row_seeds` batches of one, and as batches
of --search-batches seeds.  Random-init SDUNet and VAEDecoder at SD-1.5's shapes (as tools/sd_unet_bench.py / tools/sd_bench.py build
them), float16, [1,4,64,64] latents, brightness scorer, eps-greedy with --N candidates, --K iterations, --steps DDIM steps.  GPU only.

Every configuration runs the same seeds; one warm-up batch per configuration (every launch shape it uses is then loaded and its U-Net
graph captured: a shape is captured on its third call, which --steps >= 3 gives within one batch), then --reps timed passes, the
configurations ALTERNATING pass by pass; a pass is timed by the host clock around work that ends in a device synchronise.  Prints ONE JSON
line: per configuration the median / min / max seconds per pass and searches per second from the median, the U-Net rows and decoded images
per pass (equal across configurations: the searches do the same work), and whether every configuration selected the same candidates.
--decode-rows (default 8) caps the rows per VAE decode: 8 x [3,512,512] keeps every decoder activation below 2 GiB.  No pass/fail threshold."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diffusion_tts_amd import init as dinit
from diffusion_tts_amd.scorers import BrightnessScorer
from diffusion_tts_amd.sd_pipeline import SDSearchPipeline
from diffusion_tts_amd.sd_unet import SDUNet
from diffusion_tts_amd.vae import VAEDecoder


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, default=16)
    ap.add_argument('--search-batches', default='4,8')
    ap.add_argument('--N', type=int, default=4)
    ap.add_argument('--K', type=int, default=2)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--decode-rows', type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sd_lockstep_bench: needs a GPU (no CPU fallback, nothing is measured without one)')
    dev = torch.device('cuda')
    unet = SDUNet(dinit.sd_unet_state_dict(seed=0), device=dev, dtype=torch.float16)
    dec = VAEDecoder(dinit.vae_decoder_state_dict(seed=5), device=dev, dtype=torch.float16)
    pipe = SDSearchPipeline(unet, dec, device=dev)
    g = torch.Generator().manual_seed(0)
    pe, ne = torch.randn(1, 77, 768, generator=g), torch.randn(1, 77, 768, generator=g)
    params = {'N': a.N, 'K': a.K, 'lambda': 0.15, 'eps': 0.4}
    common = dict(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=a.steps, score_function=BrightnessScorer(dtype=torch.float32),
                  method='eps_greedy', params=params, output_type='latent')
    seeds = list(range(a.seeds))

    def picks(scores):
        return [v.index(max(v)) for v in (scores[i:i + a.N] for i in range(0, len(scores), a.N))]

    def sequential(these):
        """the single-search call per seed, as main.py makes it"""
        rows = decoded = 0
        sel = {}
        for s in these:
            torch.manual_seed(s)
            lat = torch.randn(1, 4, 64, 64)
            out, _ = pipe(latents=lat, **common)
            rows, decoded = rows + out.unet_rows, decoded + out.decoded
            sel[s] = picks(out.scores)
        return rows, decoded, sel

    def lockstep(batch):
        def run(these):
            rows = decoded = 0
            sel = {}
            for lo in range(0, len(these), batch):
                out, _ = pipe(row_seeds=these[lo:lo + batch], decode_rows=a.decode_rows, **common)
                rows, decoded = rows + out.unet_rows, decoded + out.decoded
                sel.update({s: picks(out.scores[k]) for k, s in enumerate(these[lo:lo + batch])})
            return rows, decoded, sel
        return run

    configs = {'sequential_pipe_calls': sequential, 'search_batch_1': lockstep(1)}
    for b in (int(v) for v in a.search_batches.split(',') if v):
        configs[f'search_batch_{b}'] = lockstep(b)
    for name, f in configs.items():                                   # warm-up: one batch of every configuration
        f(seeds[:max(2, int(name.rsplit('_', 1)[1]) if name.startswith('search_batch') else 2)])
    torch.cuda.synchronize()
    times = {name: [] for name in configs}
    work, sels = {}, {}
    for _ in range(a.reps):
        for name, f in configs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows, decoded, sel = f(seeds)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            work[name], sels[name] = (rows, decoded), sel
    base = sels['sequential_pipe_calls']
    res = {'what': 'SD lock-step searches: SDUNet + VAEDecoder, SD-1.5 shapes, random-init weights, float16, brightness scorer, eps-greedy',
           'device': torch.cuda.get_device_name(0), 'seeds': a.seeds, 'N': a.N, 'K': a.K, 'steps': a.steps, 'reps': a.reps,
           'decode_rows': a.decode_rows, 'unet_path': unet._graphs.path_report(), 'configs': {}}
    for name, ts in times.items():
        med = statistics.median(ts)
        res['configs'][name] = {'s_per_pass_median': round(med, 3), 's_min': round(min(ts), 3), 's_max': round(max(ts), 3),
                                'searches_per_s': round(a.seeds / med, 3), 'unet_rows_per_pass': work[name][0], 'decoded_per_pass': work[name][1],
                                'seeds_with_the_sequential_selections': sum(sels[name][s] == base[s] for s in seeds)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
