#!/usr/bin/env python3
"""Time of one CompressibilityScorer call with either codec: 'pil' (every image copied to the host and encoded by Pillow, one after the other)
against 'hip' (ops.jpeg_size on the GPU, one copy of n int32 back).  GPU only.

Two workloads: N=64 images of 64x64 (a search iteration of the EDM loop with its default scorer) and N=4 of 512x512 (a decoded batch of the SD
loop).  The images are uint8 GPU tensors, as both loops hand them over; contents are a low-frequency wave plus noise, the sizes they give are
printed.  Both codecs ALTERNATE in the same process on the same tensor: `--warmup` calls each, then `--iters` timed calls each; a call is timed
with the host clock from the call to its return -- both codecs end by building the reward tensor on the host, so the return is behind the
device-to-host copy and nothing is left in flight.  The figure is the median; the minimum is printed beside it.  The rewards of the two codecs
must be equal before anything is timed.  Prints ONE JSON line per workload and appends it to profiles/jpeg_codec_time.jsonl; there is no
pass/fail threshold."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from diffusion_tts_amd import ops
from diffusion_tts_amd.scorers import CompressibilityScorer


def images(n, hw, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:hw, 0:hw]
    ph = g.uniform(0, 6.28, (n, 3, 1, 1))
    wave = 128 + 100 * np.sin(xx / 9.0 + ph) * np.cos(yy / 7.0 + ph)
    return torch.from_numpy(np.clip(wave + g.normal(0, 12, (n, 3, hw, hw)), 0, 255).astype(np.uint8)).cuda()


def timed(fn, img):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(img, None, None)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_codec_time.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('jpeg_codec_time: needs a GPU (a host run says nothing about either path)')
    for n, hw, max_size in ((64, 64, 3000), (4, 512, 150000)):
        img = images(n, hw, seed=hw)
        codecs = {c: CompressibilityScorer(max_size=max_size, codec=c) for c in ('pil', 'hip')}
        ref = codecs['pil'](img, None, None)
        assert torch.equal(codecs['hip'](img, None, None), ref), 'the two codecs disagree: nothing is timed'
        for _ in range(args.warmup):
            for c in codecs.values():
                c(img, None, None)
        ms = {c: [] for c in codecs}
        for _ in range(args.iters):
            for name, c in codecs.items():
                ms[name].append(timed(c, img))
        med = {c: statistics.median(v) for c, v in ms.items()}
        row = dict(tool='jpeg_codec_time', device=torch.cuda.get_device_name(0), n=n, height=hw, width=hw, quality=80, iters=args.iters,
                   warmup=args.warmup, jpeg_bytes_mean=float(ops.jpeg_size(img).float().mean()),
                   pil_ms_median=round(med['pil'], 4), hip_ms_median=round(med['hip'], 4),
                   pil_ms_min=round(min(ms['pil']), 4), hip_ms_min=round(min(ms['hip']), 4),
                   pil_over_hip=round(med['pil'] / med['hip'], 2))
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
