"""Seed-sharded bulk generation: many independent searches, one image per seed, seeds split over the ranks with NO data-path
collective (the second way the path shards; the candidates of ONE search are sharded by
parallel.CandidateShards instead).

Mirrors the batch bookkeeping of the reference's bulk generator (edm/generate.py:254-309): seeds are split into
`ceil(len(seeds) / (batch * world)) * world` batches by `tensor_split` and rank r takes batches r, r+world, ...; images are
written as `<outdir>/<seed:06d>.png` (`--subdirs`: one directory per 1000 seeds).  Each image runs the search loop of
`generate_image_grid` with `seed` as its RNG seed -- `search_batch` seeds at a time in lock-step as one batch, every image on its own
seed's stream (`row_seeds`) -- so a seed's result does not depend on the number of ranks or on its batch.  Latents and
labels come from a per-seed CPU generator (the reference's StackedRandomGenerator draws on the CUDA device, a stream no
other device reproduces; its per-seed independence is what is kept).

`generate_images` is that generator itself: no search, one BATCHED plain-sampler call (plain.edm_sampler / plain.ablation_sampler) per batch of
seeds, every row with its own generator."""
import os
from typing import Any, Dict, Iterable, List, Optional

import torch
import torch.distributed as dist

from . import ops
from .sampler import SamplingMethod, generate_image_grid, load_network


def parse_int_list(s):
    """'1,2,5-10' -> [1, 2, 5, 6, 7, 8, 9, 10]  (edm/generate.py:197-207)."""
    if isinstance(s, (list, tuple)):
        return [int(v) for v in s]
    out: List[int] = []
    for part in str(s).split(','):
        if '-' in part:
            lo, hi = part.split('-')
            out.extend(range(int(lo), int(hi) + 1))
        else:
            out.append(int(part))
    return out


def rank_batches(seeds: Iterable[int], max_batch_size: int, rank: int, world: int):
    """The reference's split (edm/generate.py:259-261)."""
    seeds = list(seeds)
    num_batches = ((len(seeds) - 1) // (max_batch_size * world) + 1) * world
    return torch.as_tensor(seeds, dtype=torch.int64).tensor_split(num_batches)[rank::world]


def rank_world(rank=None, world=None):
    """(rank, world) as given; where either is missing, torch.distributed's when it is initialised, else (0, 1)"""
    if rank is None or world is None:
        dist_on = dist.is_available() and dist.is_initialized()
        rank, world = (dist.get_rank(), dist.get_world_size()) if dist_on else (0, 1)
    return rank, world


def seed_png_path(outdir, seed, subdirs=False):
    """<outdir>/<seed:06d>.png (`subdirs`: one directory per 1000 seeds), its directory created"""
    image_dir = os.path.join(outdir, f'{seed - seed % 1000:06d}') if subdirs else outdir
    os.makedirs(image_dir, exist_ok=True)
    return os.path.join(image_dir, f'{seed:06d}.png')


def seed_inputs(seed: int, net, class_idx: Optional[int] = None):
    g = torch.Generator().manual_seed(int(seed))
    latents = torch.randn([1, net.img_channels, net.img_resolution, net.img_resolution], generator=g)
    labels = None
    if net.label_dim:
        idx = int(torch.randint(net.label_dim, size=[1], generator=g)) if class_idx is None else int(class_idx)
        labels = torch.zeros(1, net.label_dim)
        labels[0, idx] = 1
    return latents, labels


def image_result(res, b, count, local_search, mcts=False):
    """Image b's part of the result dict of a lock-step generate_image_grid(row_seeds=...) call over `count` images, shaped like a one-image
    call's: the image's slice of x, image, final_scores, rewards, selected, beam_parents and best_noises; `net_rows` is the call's count
    divided by the batch size (exact: the searches run in lock-step); `row_seeds` stays the whole batch's.  local_search: eps-greedy /
    zero-order, whose rewards are [N, B] (every other trace tensor has the image first).  mcts: a lock-step MCTS call (mcts_lockstep=True),
    whose trees are ragged: the image's rewards are its rows [group] of the [S, group] tensors, what its one-image call appends, and its
    `net_rows` is its own entry of `search_rows`."""
    one = dict(res)
    for key in ('x', 'image', 'final_scores'):
        one[key] = res[key][b:b + 1]
    one['avg_score'] = float(one['final_scores'].float().mean())
    one['rewards'] = [r[b] if mcts else r[:, b:b + 1] if local_search else r[b:b + 1] for r in res['rewards']]
    one['selected'] = [s[b:b + 1] for s in res['selected']]
    one['beam_parents'] = [s[b:b + 1] for s in res['beam_parents']]
    one['best_noises'] = {i: v[:, b:b + 1] for i, v in res['best_noises'].items()}
    if mcts:
        one['net_rows'] = res['search_rows'][b]
        return one
    assert res['net_rows'] % count == 0, (res['net_rows'], count)
    one['net_rows'] = res['net_rows'] // count
    return one


@torch.no_grad()
def generate_seeds(network, seeds, outdir, *, sampling_method=SamplingMethod.NAIVE, sampling_params: Optional[Dict[str, Any]] = None,
                   class_idx: Optional[int] = None, max_batch_size: int = 64, subdirs: bool = False, device='cuda',
                   compute_dtype=ops.F16X3, verbose=False, search_batch: int = 1, rank: Optional[int] = None, world: Optional[int] = None,
                   mcts_lockstep: bool = False, **sampler_kwargs):
    """Returns {seed: result dict of generate_image_grid} for the seeds this rank generated.  This rank's seeds are split into batches of up to
    `search_batch` (rank_batches; rank / world default to torch.distributed's when it is initialised, else 0 / 1) and the searches of a batch
    run in lock-step as ONE generate_image_grid(row_seeds=batch) call -- search_batch x the rows in every denoiser and scorer call; image b
    draws from its own seed's stream, so a seed's search is the one it runs alone (search_batch=1: bit for bit the `seed=` call's; larger
    batches: up to the launch forms the row count selects).  One PNG per seed; each seed's dict is its slice of the call's (image_result).
    MCTS, and calls with forced_selections / precomputed_noise (per search by nature), run one `seed=` call per seed as before --
    unless `mcts_lockstep=True` (MCTS only): then the trees of a batch's seeds advance as one batch too (generate_image_grid(row_seeds=batch,
    mcts_lockstep=True)), seed s on its own torch stream and on numpy.random.RandomState(s) for its rollout child draws.
    `max_batch_size` is accepted for the reference's signature; the split is by `search_batch`.  sampler_kwargs go to every call:
    `share_identical=True` (eps-greedy / zero-order / beam_search=True) evaluates the identical candidates of a sigma step without churn
    noise once per image -- the same PNGs from fewer denoiser rows."""
    rank, world = rank_world(rank, world)
    if int(search_batch) < 1:
        raise ValueError(f'search_batch: a positive number of seeds per lock-step batch, got {search_batch}')
    if mcts_lockstep and sampling_method != SamplingMethod.MCTS:
        raise ValueError(f'mcts_lockstep=True: SamplingMethod.MCTS only, got {sampling_method.name}')
    per_search = any(sampler_kwargs.get(k) is not None for k in ('forced_selections', 'precomputed_noise'))
    if mcts_lockstep and per_search:
        raise ValueError('mcts_lockstep=True: forced_selections / precomputed_noise are not supported with per-image random streams')
    net = load_network(network, device=device, dtype=compute_dtype)
    lock_step = (sampling_method != SamplingMethod.MCTS or mcts_lockstep) and not per_search
    if mcts_lockstep:
        sampler_kwargs = dict(sampler_kwargs, mcts_lockstep=True)
    local_search = sampling_method in (SamplingMethod.EPS_GREEDY, SamplingMethod.ZERO_ORDER)
    done = {}

    for batch in rank_batches(parse_int_list(seeds), int(search_batch), rank, world):
        batch = batch.tolist()
        if not batch:
            continue
        inputs = [seed_inputs(seed, net, class_idx) for seed in batch]
        common = dict(gridw=1, gridh=1, device=device, sampling_method=sampling_method, sampling_params=sampling_params,
                      compute_dtype=compute_dtype, verbose=verbose, shard_candidates=False, **sampler_kwargs)
        if not lock_step:
            for seed, (latents, labels) in zip(batch, inputs):
                done[seed] = generate_image_grid(net, seed_png_path(outdir, seed, subdirs), latents, labels, seed=seed, **common)
            continue
        latents = torch.cat([lat for lat, _ in inputs], dim=0)
        labels = None if inputs[0][1] is None else torch.cat([lab for _, lab in inputs], dim=0)
        res = generate_image_grid(net, None, latents, labels, row_seeds=batch, **common)
        for b, seed in enumerate(batch):
            done[seed] = image_result(res, b, len(batch), local_search, mcts=mcts_lockstep)
            save_image(done[seed]['image'][0].permute(1, 2, 0).contiguous().numpy(), seed_png_path(outdir, seed, subdirs))
    return done


@torch.no_grad()
def generate_sd_seeds(pipe, prompt, seeds, outdir, *, method='naive', params=None, search_batch: int = 1, num_inference_steps=50,
                      score_function=None, subdirs: bool = False, decode_rows: Optional[int] = None, rank: Optional[int] = None,
                      world: Optional[int] = None, save=True, **pipe_kwargs):
    """The SD backend's bulk mode: one search per seed with `pipe` (sd_pipeline.SDSearchPipeline), `<outdir>/<seed:06d>.png` per seed.  This
    rank's seeds (rank_batches; rank / world default to torch.distributed's when it is initialised, else 0 / 1; no collective is used) run
    `search_batch` at a time in lock-step as ONE `pipe(..., row_seeds=batch)` call; seed s draws what `main.py --backend sd --seed s` draws,
    so its search does not depend on its batch or on the number of ranks.  `method='rejection'` is the reference's N-trajectory loop as N
    rows per seed; `method='mcts'` (ragged trees) runs one single-search call per seed after `torch.manual_seed(seed)`.  decode_rows caps the
    rows per VAE decode.  pipe_kwargs (prompt_embeds=, negative_prompt_embeds=, guidance_scale=, eta=, ...) go to the call.
    Returns {seed: maximum score} for the seeds this rank generated."""
    rank, world = rank_world(rank, world)
    if int(search_batch) < 1:
        raise ValueError(f'search_batch: a positive number of seeds per lock-step batch, got {search_batch}')
    params = {} if params is None else params
    done = {}

    def write(image, seed):
        if save:
            arr = (image.clamp(0, 1).permute(1, 2, 0).float().cpu().numpy() * 255).round().astype('uint8')
            save_image(arr, seed_png_path(outdir, seed, subdirs))

    def number(v):
        return float(v.item() if torch.is_tensor(v) else v)

    for batch in rank_batches(parse_int_list(seeds), int(search_batch), rank, world):
        batch = batch.tolist()
        if not batch:
            continue
        if method == 'mcts':
            cfg = pipe.unet.config
            for seed in batch:
                torch.manual_seed(seed)
                lat = torch.randn(1, cfg.in_channels, cfg.sample_size, cfg.sample_size)
                out, score = pipe(prompt=prompt, latents=lat, num_inference_steps=num_inference_steps, score_function=score_function,
                                  method=method, params=params, output_type='pt', **pipe_kwargs)
                done[seed] = number(score)
                write(out.images[0], seed)
            continue
        out, scores = pipe(prompt=prompt, num_inference_steps=num_inference_steps, score_function=score_function, method=method,
                           params=params, output_type='pt', row_seeds=batch, decode_rows=decode_rows, **pipe_kwargs)
        for k, seed in enumerate(batch):
            done[seed] = number(scores[k])
            write(out.images[k], seed)
    return done


def batch_inputs(batch_seeds, net, class_idx: Optional[int] = None):
    """(rnd, latents, labels) of one batch as edm/generate.py:281-288 picks them: a StackedRandomGenerator over the batch's seeds, latents drawn
    first, then the label indices; `class_idx` overrides the drawn classes (the draw is still made)."""
    from .plain import StackedRandomGenerator
    rnd = StackedRandomGenerator(batch_seeds)
    n = len(batch_seeds)
    latents = rnd.randn([n, net.img_channels, net.img_resolution, net.img_resolution])
    labels = None
    if net.label_dim:
        labels = torch.eye(net.label_dim)[rnd.randint(net.label_dim, size=[n])]
    if class_idx is not None:
        if labels is None:
            raise ValueError('class_idx: the network is unconditional')
        labels[:, :] = 0
        labels[:, int(class_idx)] = 1
    return rnd, latents, labels


ABLATION_KEYS = ('solver', 'discretization', 'schedule', 'scaling')


def pick_sampler(sampler_kwargs):
    """ablation_sampler if any of its four choices is given, else edm_sampler (edm/generate.py:291-293); None values are dropped"""
    from . import plain
    kw = {k: v for k, v in sampler_kwargs.items() if v is not None}
    return (plain.ablation_sampler if any(k in kw for k in ABLATION_KEYS) else plain.edm_sampler), kw


def save_image(image_hwc, path):
    """one uint8 [h, w, c] image as PNG: grey for one channel (edm/generate.py:302-305)"""
    import PIL.Image
    if image_hwc.shape[2] == 1:
        PIL.Image.fromarray(image_hwc[:, :, 0], 'L').save(path)
    else:
        PIL.Image.fromarray(image_hwc, 'RGB').save(path)


@torch.no_grad()
def generate_images(network, seeds, outdir, *, class_idx: Optional[int] = None, max_batch_size: int = 64, subdirs: bool = False,
                    device='cuda', compute_dtype=ops.F16X3, rank: Optional[int] = None, world: Optional[int] = None, sampler_fn=None,
                    **sampler_kwargs):
    """The reference's bulk generator (edm/generate.py:254-309): this rank's batches of `rank_batches`, ONE batched sampler call per batch
    (plain.edm_sampler, or plain.ablation_sampler when solver / discretization / schedule / scaling is given), each row with its own CPU
    generator, quantised by ops.quantize_u8 and written as `<outdir>/<seed:06d>.png`.  rank / world default to torch.distributed's when it is
    initialised, else 0 / 1; no collective is used.  `sampler_fn(net, latents, labels, randn_like=..., **kwargs)` replaces the choice of
    sampler.  Returns {seed: uint8 image [c, h, w] (CPU)} for the seeds this rank generated."""
    rank, world = rank_world(rank, world)
    net = load_network(network, device=device, dtype=compute_dtype)
    picked, kw = pick_sampler(sampler_kwargs)
    sampler_fn = picked if sampler_fn is None else sampler_fn
    done = {}
    for batch in rank_batches(parse_int_list(seeds), max_batch_size, rank, world):
        batch_seeds = batch.tolist()
        if not batch_seeds:
            continue
        rnd, latents, labels = batch_inputs(batch_seeds, net, class_idx)
        x = sampler_fn(net, latents, labels, randn_like=rnd.randn_like, **kw)
        images = ops.quantize_u8(x).cpu()
        for seed, image in zip(batch_seeds, images):
            save_image(image.permute(1, 2, 0).contiguous().numpy(), seed_png_path(outdir, seed, subdirs))
            done[seed] = image
    return done
