#!/usr/bin/env python3
"""Throughput of the NCSN++ CIFAR-32 denoiser beside DDPM++'s, by the timing method of bench.py's `ddpmpp32_rejection` workload: one step =
one Heun step of N = 16 rejection trajectories at sigma step 5 (2 N candidate U-Net evaluations) + the brightness score of the predicted
images; 3 setup steps (kernel attributes, graph capture), W warm-up steps, then K steps between synchronisations.  One JSON line per network.

  python tools/ncsnpp_bench.py [--dtype f16x3] [--steps 20] [--warmup 3] [--nets ncsnpp_cifar10,ddpmpp_cifar10]
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ncsnpp_bench.py --nets ncsnpp_cifar10 --steps 5     (per-kernel shares)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault('DTS_GRAPHS_STRICT', '1')

import torch                                                    # noqa: E402

import bench                                                    # noqa: E402  (sigma_steps, torch_dtype)
from diffusion_tts_amd import init as dinit                     # noqa: E402
from diffusion_tts_amd import config as dcfg                    # noqa: E402
from diffusion_tts_amd.networks import EDMPrecond               # noqa: E402
from diffusion_tts_amd.parallel import CandidateShards          # noqa: E402
from diffusion_tts_amd.sampler import _Loop                     # noqa: E402
from diffusion_tts_amd.scorers import BrightnessScorer          # noqa: E402


def measure(name, dtype, steps, warmup, n=16):
    dev = torch.device('cuda')
    cfg = getattr(dcfg, name)()
    sd, _ = dinit.refill_degenerate(dinit.edm_state_dict(cfg, 0), 0)
    net = EDMPrecond(cfg, sd, device=dev, dtype=dtype)
    scorer, shards = BrightnessScorer(), CandidateShards()
    L = _Loop(net, dev, 18, 40, 0.05, 50, 1.003, None, shards)
    t = bench.sigma_steps()
    g = torch.Generator().manual_seed(99)
    r = cfg.img_resolution
    x = (torch.randn(n, 3, r, r, generator=g, dtype=torch.float64) * t[5]).to(dev).contiguous()
    eps = [torch.randn(n, 3, r, r, generator=g, dtype=torch.float64).to(dev).contiguous() for _ in range(4)]
    lab = torch.eye(10)[torch.tensor([3])].repeat(n, 1).to(dev).contiguous() if cfg.label_dim else None

    def one_step(s):
        xn, _ = L.step(x, t[5], t[6], 5, eps[s % 4], lab, nb=n)
        loc = L.score(scorer, xn, lab).to(dev, torch.float32)
        return int(shards.gather_rewards(loc, n, 1).cpu().argmax())

    for s in range(3 + warmup):
        one_step(s)
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for s in range(steps):
        one_step(warmup + s)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    return dict(network=name, metric=f'candidate U-Net steps/sec, {name} rejection N={n}', value=round(2 * n * steps / dt, 1),
                ms_per_step=round(dt / steps * 1e3, 3), steps=steps, warmup=warmup, path=net._graphs.path_report())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', default='f16x3')
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--nets', default='ncsnpp_cifar10,ddpmpp_cifar10,ncsnpp_cifar10,ddpmpp_cifar10')
    a = ap.parse_args()
    for name in a.nets.split(','):
        print(json.dumps(dict(measure(name, bench.torch_dtype(a.dtype), a.steps, a.warmup), dtype=a.dtype)), flush=True)


if __name__ == '__main__':
    main()
