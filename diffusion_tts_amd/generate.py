"""`python -m diffusion_tts_amd.generate`: the reference's bulk generator (edm/generate.py) on MI355X, with its option names.

    python -m diffusion_tts_amd.generate --network random:ddpmpp_cifar10 --outdir out --seeds 0-63 --batch 64
    python -m diffusion_tts_amd.generate --network random:vp_cifar10 --outdir out --seeds 0-63 --solver euler --disc vp --schedule vp --scaling vp
    python -m torch.distributed.run --standalone --nproc_per_node=8 -m diffusion_tts_amd.generate --network net.pkl --outdir out --seeds 0-49999 --subdirs

--network takes what sampler.load_network takes (a local EDM network .pkl, a .pt bundle, random:<preset>[:seed]).  Any of --solver / --disc /
--schedule / --scaling selects the ablation sampler, otherwise the EDM sampler runs.  Under torch.distributed.run every process takes its share
of the seed batches (RANK / WORLD_SIZE / LOCAL_RANK of the environment); no process group is created because no collective is needed.
"""
import argparse
import os
import time

import torch

from . import bulk
from .ops import F16X3

DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32, 'f16x3': F16X3, 'auto': 'auto'}


def _positive(text):
    v = float(text)
    if not v > 0:
        raise argparse.ArgumentTypeError(f'{text}: must be > 0')
    return v


def _non_negative(text):
    v = float(text)
    if not v >= 0:
        raise argparse.ArgumentTypeError(f'{text}: must be >= 0')
    return v


def parser():
    p = argparse.ArgumentParser(prog='python -m diffusion_tts_amd.generate', description='Generate images with the EDM or the ablation sampler')
    p.add_argument('--network', required=True, help='EDM network .pkl (local path), .pt bundle or random:<preset>[:seed]')
    p.add_argument('--outdir', required=True, help='where the images go')
    p.add_argument('--seeds', type=bulk.parse_int_list, default='0-63', help='random seeds, e.g. 1,2,5-10')
    p.add_argument('--subdirs', action='store_true', help='one subdirectory per 1000 seeds')
    p.add_argument('--class', dest='class_idx', type=int, default=None, help='class label (default: random per seed)')
    p.add_argument('--batch', dest='max_batch_size', type=int, default=64, help='largest batch')
    p.add_argument('--steps', dest='num_steps', type=int, default=18, help='number of sampling steps')
    p.add_argument('--sigma_min', type=_positive, default=None, help='lowest noise level (default: by sampler)')
    p.add_argument('--sigma_max', type=_positive, default=None, help='highest noise level (default: by sampler)')
    p.add_argument('--rho', type=_positive, default=7, help='time step exponent')
    p.add_argument('--S_churn', type=_non_negative, default=0, help='stochasticity strength')
    p.add_argument('--S_min', type=_non_negative, default=0, help='lowest noise level that is churned')
    p.add_argument('--S_max', type=_non_negative, default=float('inf'), help='highest noise level that is churned')
    p.add_argument('--S_noise', type=float, default=1, help='noise inflation')
    p.add_argument('--solver', choices=['euler', 'heun'], default=None, help='ablation: ODE solver')
    p.add_argument('--disc', dest='discretization', choices=['vp', 've', 'iddpm', 'edm'], default=None, help='ablation: time steps')
    p.add_argument('--schedule', choices=['vp', 've', 'linear'], default=None, help='ablation: noise schedule sigma(t)')
    p.add_argument('--scaling', choices=['vp', 'none'], default=None, help='ablation: signal scaling s(t)')
    p.add_argument('--dtype', choices=sorted(DTYPES), default='f16x3', help="compute mode; auto: float16 when the checkpoint records use_fp16")
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    if args.class_idx is not None and args.class_idx < 0:
        raise SystemExit('--class: a class index >= 0')
    if args.max_batch_size < 1 or args.num_steps < 1:
        raise SystemExit('--batch and --steps: at least 1')
    rank, world, local = (int(os.environ.get(k, d)) for k, d in (('RANK', '0'), ('WORLD_SIZE', '1'), ('LOCAL_RANK', '0')))
    device = torch.device('cuda', local)
    torch.cuda.set_device(device)
    kw = {k: getattr(args, k) for k in ('num_steps', 'sigma_min', 'sigma_max', 'rho', 'S_churn', 'S_min', 'S_max', 'S_noise', 'solver',
                                        'discretization', 'schedule', 'scaling')}
    if rank == 0:
        print(f'Generating {len(args.seeds)} images to "{args.outdir}"...')
    t0 = time.time()
    done = bulk.generate_images(args.network, args.seeds, args.outdir, class_idx=args.class_idx, max_batch_size=args.max_batch_size,
                                subdirs=args.subdirs, device=device, compute_dtype=DTYPES[args.dtype], rank=rank, world=world, **kw)
    torch.cuda.synchronize()
    print(f'[rank {rank}/{world}] {len(done)} images in {time.time() - t0:.1f} s')
    return done


if __name__ == '__main__':
    main()
