"""The EDM noise-trajectory-search sampling loop on MI355X: drop-in for `generate_image_grid`
(edm/main.py:47-886) with the same `SamplingMethod` / `SamplingParams` plugin surface (edm/main.py:27-43).

What stays on the host (as in the reference): the sigma schedule, the search control flow, the RNG.  All search
randomness is drawn from the torch *CPU* global generator (and numpy's for MCTS) in exactly the reference's call
order -- including draws whose values the reference throws away -- and uploaded, because the parity oracle is the
reference's `--device cpu` run and a device Philox stream could not reproduce it (hard part 2).
What runs on the GPU: every tensor operation -- candidate construction (K14), the fp64 Heun/Euler step (K9), the
denoiser, quantisation (K10) and the scorer.  A batch draws from L lanes (`_Source`): L = 1, the global stream for all its images, or with
`row_seeds` L = B, a CPU generator per image: the searches of several seeds run in lock-step as one batch, each the search its seed runs alone.
The sigma schedule, the churn rule and the Heun step are plain.py's (`edm_sigmas`, `churn_of`, `heun_step`): the plain sampler is this loop without a search.

With torch.distributed initialised (one process per GPU) the N candidates of each search iteration are sharded
across ranks (parallel.CandidateShards): one all-gather of N*B rewards per iteration, identical argmax on every rank.
"""
import os
from dataclasses import dataclass, field
from enum import Enum, auto
from typing import Any, Callable, Dict, Optional, Sequence

import numpy as np
import torch

from . import ops
from .hashing import builtin_scale
from .parallel import CandidateShards
from .plain import churn_of, edm_sigmas, heun_loop, heun_step, heun_step_rows
from .scorers import Scorer, CompressibilityScorer


class SamplingMethod(Enum):          # edm/main.py:27-33
    MCTS = auto()
    BEAM_SEARCH = auto()
    ZERO_ORDER = auto()
    NAIVE = auto()
    REJECTION_SAMPLING = auto()
    EPS_GREEDY = auto()


@dataclass
class SamplingParams:                # edm/main.py:35-43
    B: int = 2
    N: int = 4
    K: int = 20
    lambda_param: float = 0.15
    eps: float = 0.4
    S: int = 8
    scorer: Scorer = field(default_factory=lambda: CompressibilityScorer(dtype=torch.float32))


def load_network(spec, device='cuda', dtype=ops.F16X3):
    """`network_pkl` argument of generate_image_grid.  The reference unpickles an NVIDIA EDM checkpoint from a URL
    (edm/main.py:69-70); URLs cannot be fetched here, so accepted forms are: a ready network object; the local path of
    an EDM network pickle (`*.pkl`, read by checkpoint.load_edm_pickle without executing its embedded source); a
    torch-saved dict {'cfg': EDMConfig kwargs, 'state_dict': {...reference keys...}}; or 'random:<preset>[:seed]'
    with preset in {adm_imagenet64, ddpmpp_cifar10, ncsnpp_cifar10, ncsnpp_ffhq64, vp_cifar10, ve_cifar10, iddpm_imagenet64} (random init +
    the documented weight rule; the last three are the VP, VE and iDDPM preconditioners over DDPM++, NCSN++ and ADM).  A pickle or bundle
    carries its preconditioner (`EDMConfig.precond`) with it.  dtype='auto': float16 when the file records use_fp16=True, else ops.F16X3."""
    from . import init as dinit
    from .config import (EDMConfig, adm_imagenet64, ddpmpp_cifar10, ncsnpp_cifar10, ncsnpp_ffhq64, vp_cifar10, ve_cifar10,
                         iddpm_imagenet64)
    from .networks import EDMPrecond
    if callable(spec) and hasattr(spec, 'round_sigma'):
        return spec

    def mode(cfg):
        return dtype if dtype != 'auto' else (torch.float16 if cfg.use_fp16 else ops.F16X3)
    if isinstance(spec, str) and spec.startswith('random:'):
        parts = spec.split(':')
        presets = {'adm_imagenet64': adm_imagenet64, 'ddpmpp_cifar10': ddpmpp_cifar10, 'ncsnpp_cifar10': ncsnpp_cifar10,
                   'ncsnpp_ffhq64': ncsnpp_ffhq64, 'vp_cifar10': vp_cifar10, 've_cifar10': ve_cifar10, 'iddpm_imagenet64': iddpm_imagenet64}
        if parts[1] not in presets:
            raise ValueError(f'unknown preset {parts[1]!r}: one of {sorted(presets)}')
        preset = presets[parts[1]]()
        seed = int(parts[2]) if len(parts) > 2 else 0
        sd, _ = dinit.refill_degenerate(dinit.edm_state_dict(preset, seed), seed)
        return EDMPrecond(preset, sd, device=device, dtype=mode(preset))
    if isinstance(spec, str) and spec.endswith(('.pt', '.pth')):
        blob = torch.load(spec, map_location='cpu')
        cfg = EDMConfig(**blob['cfg'])
        return EDMPrecond(cfg, blob['state_dict'], device=device, dtype=mode(cfg))
    if isinstance(spec, str) and spec.endswith('.pkl'):
        # an NVIDIA EDM network pickle, e.g. a downloaded edm-imagenet-64x64-cond-adm.pkl (the reference's `network_pkl`,
        # main.py:157-158): weights and constructor arguments are read without executing the source embedded in the file
        from .checkpoint import load_edm_pickle
        cfg, sd = load_edm_pickle(spec)
        return EDMPrecond(cfg, sd, device=device, dtype=mode(cfg))
    raise ValueError(f'cannot load network from {spec!r}: pass a network object, an EDM network .pkl (local path), a .pt '
                     f'state-dict bundle or "random:<preset>[:seed]" (URLs cannot be fetched here)')


def _side_by_side(parts):
    """the draws of the lanes as one batch [B, ...]: the one lane's draw is the batch itself, not a copy of it"""
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


class _Source:
    """Where the host draws of a search come from.  row_seeds=None: torch's global CPU generator, one stream for the whole batch (the
    reference's).  row_seeds given: image b draws from its own torch.Generator().manual_seed(row_seeds[b]) in exactly the order and shapes
    a one-image call seeded row_seeds[b] draws from the global stream -- which such a generator replays bit for bit -- so an image's
    numbers do not depend on its companions in the batch.  torch's CPU generator keeps the low 32 bits of a seed and nothing else (seed
    s + 2^32 replays seed s): a seed outside [0, 2^32) is refused by name, not reduced in silence.
    Either way it is L lanes, a lane being one stream and the images it covers: the lane None (generator=None, the global one) covers the whole
    batch, lane b of row_seeds covers image b; every draw is a lane's `randn` / `rand1`."""

    def __init__(self, row_seeds=None):
        for s in row_seeds or ():
            if not 0 <= int(s) < 2 ** 32:
                raise ValueError(f'row_seeds: seed {int(s)} is outside [0, 2^32): torch\'s CPU generator would keep its low 32 bits '
                                 f'(the stream of seed {int(s) % 2 ** 32})')
        self.gens = {None: None} if row_seeds is None else {b: torch.Generator().manual_seed(int(s)) for b, s in enumerate(row_seeds)}
        self.L = len(self.gens)                                          # lanes: 1 for the whole batch, or one per image

    def _gen(self, image):
        return self.gens[image if image in self.gens else None]          # the image's own lane, or the one lane of all

    def randn(self, image, shape, dtype=torch.float64):
        """one draw of `shape` from the stream of lane (or image) `image`"""
        return torch.randn(shape, dtype=dtype, generator=self._gen(image))

    def rand1(self, image):
        return torch.rand(1, generator=self._gen(image))

    def lanes(self, shape):
        """the L lanes behind a batch of `shape` [B, ...] as (lane, shape of one draw): [B, ...] for the one lane of all, [1, ...] for an image's own"""
        assert self.L in (1, shape[0]), f'{self.L} lanes for a batch of {shape[0]} images: one lane in all, or one per image'
        return [(lane, (shape[0] // self.L,) + tuple(shape[1:])) for lane in self.gens]

    def images(self, B, rows, shape1):
        """[B * rows, *shape1] float64 normals, image-major: per lane one draw of `rows` rows for each image it covers"""
        return _side_by_side([self.randn(lane, (n * rows,) + tuple(shape1)) for lane, (n, *_) in self.lanes((B,))])

    def beams(self, S, B, N, shape1):
        """[S * B, N, *shape1] float64 normals: one draw of N candidates per beam row in row order (image-major: image s draws its B blocks in order)"""
        return torch.stack([self.randn(r // B, (N,) + tuple(shape1)) for r in range(S * B)])


def grid_schedule(net, num_steps, sigma_min, sigma_max, rho):
    """t_steps of generate_image_grid (edm/main.py:78-80): `edm_sigmas` of the range as given -- not clamped to the network's -- rounded, then 0"""
    t_steps = edm_sigmas(num_steps, sigma_min, sigma_max, rho)
    return torch.cat([net.round_sigma(t_steps), torch.zeros_like(t_steps[:1])])


def identical_steps(t_steps, num_steps, S_churn, S_min, S_max, S_noise, round_sigma):
    """The sigma steps at which every candidate of a search is the same row: those whose noise coefficient (`churn_of`, the number the
    step hands to ops.heun_xhat) is exactly 0.0, so x_hat = x_cur + 0 * eps whatever eps is.  The test is on the coefficient, not on
    gamma: a `round_sigma` that moves t_hat off t_cur (VP, VE, iDDPM) adds noise without churn, and such a step is not listed.
    t_steps: the schedule, a float64 tensor of at least num_steps levels.  Pure host arithmetic."""
    t = torch.as_tensor(t_steps, dtype=torch.float64)
    return [i for i in range(num_steps) if churn_of(t[i], num_steps, S_churn, S_min, S_max, S_noise, round_sigma)[1] == 0.0]


def shared_rows_saved(shared, num_steps, N, K, B=1):
    """Denoiser rows an eps-greedy / zero-order search over B images does not launch with share_identical=True: at each sigma step of
    `shared` its K candidate batches of N * B rows, two Heun stages each, one at the last step.  (The batch-B pivot step of every sigma
    step is made either way.)  Sharded over ranks: N is the rank's own share of the candidates."""
    return sum(K * N * B * (1 if i == num_steps - 1 else 2) for i in shared)


class _Loop:
    """State shared by the search methods: schedule, device step, bookkeeping."""

    def __init__(self, net, device, num_steps, S_churn, S_min, S_max, S_noise, scale_fn, shards):
        self.net, self.dev, self.num_steps = net, device, num_steps
        self.S_churn, self.S_min, self.S_max, self.S_noise = S_churn, S_min, S_max, S_noise
        self.scale_fn, self.shards = scale_fn, shards
        self.rewards, self.selected = [], []
        self.beam_parents = []                # generate_image_grid(beam_search=True): selected // N per sigma step
        self.record_noises, self.best_noises = False, {}
        self.reuse_winner = False
        self.forced = None                    # generate_image_grid(forced_selections=...)
        self.chunk = None                     # generate_image_grid(candidate_chunk=...)
        self.src = _Source()                  # generate_image_grid(row_seeds=...): one stream per image
        self.shared = frozenset()             # generate_image_grid(share_identical=True): identical_steps(...) of this schedule
        self.row_seeds = None                 # generate_image_grid(row_seeds=...) as given: the MCTS lock-step's numpy streams are seeded from it
        self.mcts_ragged_launches = self.mcts_mixed_launches = 0    # mcts_lockstep=True: per-row step launches; those over >= 2 sigma steps
        self.search_rows = None               # mcts_lockstep=True: the denoiser rows of each search

    def up(self, t, dtype=None):
        return t.to(self.dev, dtype).contiguous() if dtype is not None else t.to(self.dev).contiguous()

    def churn(self, t_cur):
        return churn_of(t_cur, self.num_steps, self.S_churn, self.S_min, self.S_max, self.S_noise, self.net.round_sigma)

    def step(self, x_cur, t_cur, t_next, i, eps, labels, nb=None, interleave=False, live=None, first_denoised=False):
        """edm/main.py:82-96 on the device.  x_cur [xb,...] f64 is broadcast to nb rows; eps [nb,...] f64|f32.
        live: rows that are real candidates (the rest is batch-shape padding): only those count as candidate evaluations.
        first_denoised: return D(x_hat, t_hat) instead of the second-order output (the beam branch's own step, edm/main.py:161-212)."""
        nb = eps.shape[0] if nb is None else nb
        evals0 = getattr(self.net, 'evals', None)
        x_next, D1, D = heun_step(self.net, x_cur, eps, self.churn(t_cur), t_next, i >= self.num_steps - 1, labels, nb, interleave)
        if live is not None and live != nb and evals0 is not None:       # padding rows went through the denoiser but are not counted
            self.net.evals = evals0 + (self.net.evals - evals0) // nb * live
        return x_next, (D1 if first_denoised else D)

    def step_rows(self, x_cur, t_hat, coef, t_next, eps, labels, live=None):
        """`step` with the scalars of the sigma step per row (plain.heun_step_rows): x_cur [xb, ...] in repeat_interleave form, never the last
        sigma step; live as in `step`.  Returns x_next."""
        nb = eps.shape[0]
        evals0 = getattr(self.net, 'evals', None)
        x_next = heun_step_rows(self.net, x_cur, eps, t_hat, coef, t_next, labels)
        if live is not None and live != nb and evals0 is not None:
            self.net.evals = evals0 + (self.net.evals - evals0) // nb * live
        return x_next

    def score(self, scorer, x, labels):
        img = ops.quantize_u8(x)
        ts = torch.zeros(img.shape[0], device=self.dev)
        return scorer(img, labels, ts)

    def winner_rows(self, x, best, N, row):
        """[B, ...]: for image b the row of its winner best[b] among N candidates, sent by the rank that owns that candidate.  x: the rows of
        this rank's share [lo, hi); row(b, j) is where it keeps its j-th candidate of image b."""
        lo, hi = self.shards.span(N)
        mine = lambda b, j: x[row(b, j - lo)].clone() if lo <= j < hi else torch.empty(x.shape[1:], dtype=torch.float64, device=self.dev)
        return torch.stack([self.shards.broadcast_from_owner(mine(b, j), j, N) for b, j in enumerate(best.tolist())])


# ---------------------------------------------------------------------------------------------------------
def _naive(L: _Loop, t_steps, x_next, labels, p, pre):
    return heun_loop(L.net, x_next, labels, t_steps, L.churn, lambda x: L.src.images(x.shape[0], 1, x.shape[1:]))   # edm/main.py:865


def _rejection(L: _Loop, t_steps, x_next, labels, p, pre):
    """edm/main.py:101-137; rows are b-major (repeat_interleave).  Sharded: rank r carries candidates [lo,hi) of
    every sample through all steps; rewards all-gathered once; the winner's image broadcast from its owner."""
    N, B = p.N, x_next.shape[0]
    L.shards.require_candidates(N, 'rejection sampling')
    lo, hi = L.shards.span(N)
    nl = hi - lo
    shape1 = tuple(x_next.shape[1:])
    lab = None if labels is None else labels.repeat_interleave(nl, dim=0).contiguous()
    x = x_next
    for i in range(L.num_steps):
        if pre is not None and i in pre:
            eps = pre[i][:, :N].reshape(B * N, *shape1).to(torch.float64)
        else:
            eps = L.src.images(B, N, shape1)                                         # edm/main.py:120
        eps_l = L.up(eps.view(B, N, *shape1)[:, lo:hi].reshape(B * nl, *shape1))
        x, _ = L.step(x, t_steps[i], t_steps[i + 1], i, eps_l, lab, interleave=(i == 0))      # the first step fans every image out to its nl rows
    loc = L.score(p.scorer, x, lab).to(L.dev, torch.float32).view(B, nl).t().contiguous().reshape(-1)   # candidate-major
    allr = L.shards.gather_rewards(loc, N, B).view(N, B).t().contiguous().cpu()                # [B, N]
    best = allr.argmax(dim=1)                                                                  # edm/main.py:136
    L.rewards.append(allr)
    L.selected.append(best)
    return L.winner_rows(x, best, N, lambda b, j: b * nl + j)


def _beam(L: _Loop, t_steps, x_next, labels, p, pre):
    # The reference branch is dead code: it reads method_params.b / .k, which SamplingParams does not define
    # (edm/main.py:140), so `--method beam` raises AttributeError on entry.  Kept verbatim for drop-in behaviour.
    b, k = p.b, p.k
    raise RuntimeError('unreachable')


def beam_select(rewards, B):
    """Top B of each row of `rewards` [S, B*N] (host, float32), best first; exact ties go to the lower flat index j*N + n.
    A stable host sort, as the SD beam's (sd_pipeline.py): torch.topk leaves the order of exact ties unspecified."""
    r = rewards.to(torch.float32).cpu()
    rows = [sorted(range(r.shape[1]), key=v.__getitem__, reverse=True)[:B] for v in r.tolist()]
    return torch.tensor(rows, dtype=torch.int64).reshape(r.shape[0], B)


def _beam_search(L: _Loop, t_steps, x_next, labels, p, pre):
    """generate_image_grid(beam_search=True): the search edm/main.py:138-404 sets out to do -- B = p.B beams per image (the reference's k),
    N = p.N candidates per beam (its b) -- with the survivor gather fixed (:375-379 reads every survivor from beam row `sample_idx`).
    Beam rows are image-major (row s*B + j, :155); per sigma step one host draw [N, C, H, W] per beam row in row order (:257), drawn at
    gamma = 0 steps too; every candidate takes the full step with churn and Heun and is scored on the step's returned `denoised`
    (:319-336) -- the branch's own step_with_microbatch (:161-212) returns the FIRST denoiser output, D(x_hat, t_hat), its Heun stage
    keeps a `denoised_2` of its own; the reference's k = 1 runs pin that (tests/golden/make_golden_beam.py); per image the top
    B of the B*N rewards survive in rank order (beam_select); the result is beam 0 (:404).  All S*B*N rows of a step go through the
    denoiser and the scorer in one call each (the reference's micro-batches are memory workarounds over independent rows).
    Sharded: rank r owns candidates [lo, hi) of EVERY beam; per step one reward all-gather and one exchange of the S*B survivor rows."""
    B, N, S = p.B, p.N, x_next.shape[0]
    shape1 = tuple(x_next.shape[1:])
    L.shards.require_candidates(N, 'EDM beam search')
    lo, hi = L.shards.span(N)
    nl = hi - lo
    lab = None if labels is None else labels.repeat_interleave(B * nl, dim=0).contiguous()
    x = x_next.repeat_interleave(B, dim=0).contiguous()                               # [S*B, ...] (:155)

    def draw(i):
        if pre is not None and i in pre:
            if tuple(pre[i].shape) != (S, B, N) + shape1:
                raise ValueError(f'precomputed_noise[{i}]: beam search takes [S, B, N, C, H, W] = {(S, B, N) + shape1}, got {tuple(pre[i].shape)}')
            return pre[i].to(torch.float64).reshape(S * B, N, *shape1)
        return L.src.beams(S, B, N, shape1)                                            # :257, one draw per beam

    def decide(allr):
        """a sigma step's decision on its rewards allr [S, B*N], recorded: the survivors sel [S, B] (flat j*N + n) and their parent beam rows [S*B]"""
        sel = beam_select(allr, B)
        L.rewards.append(allr)
        L.selected.append(sel)
        L.beam_parents.append(sel // N)
        return sel, (torch.arange(S).reshape(S, 1) * B + sel // N).reshape(-1)

    # share_identical: cls[r] is the lowest beam row known to hold the state of beam row r (same image).  The B beams of an image start as
    # copies of one state: one class.  A step without noise keeps equal rows equal, so its survivors inherit their parents' classes; any
    # other step gives every survivor a noise of its own
    cls = [r - r % B for r in range(S * B)]
    eps = draw(0)
    for i in range(L.num_steps):
        if i in L.shared:
            # all N candidates of a beam row are that row, and rows of one class are one row: one row per class goes through the step and
            # the scorer, on every rank alike (no reward all-gather, no survivor exchange); rewards and survivors are expanded from it
            reps = sorted(set(cls))
            at = {r: q for q, r in enumerate(reps)}
            x_rep = x.index_select(0, L.up(torch.tensor(reps))) if len(reps) < S * B else x
            lab_rep = None if labels is None else labels.index_select(0, L.up(torch.tensor([r // B for r in reps]))).contiguous()
            x_cand, x0 = L.step(x_rep, t_steps[i], t_steps[i + 1], i, torch.zeros_like(x_rep), lab_rep, first_denoised=True)
            loc = L.score(p.scorer, x0, lab_rep).to(L.dev, torch.float32)
            eps = draw(i + 1) if i + 1 < L.num_steps else None
            of_row = torch.tensor([at[c] for c in cls])
            allr = loc.cpu()[of_row].reshape(S, B, 1).expand(S, B, N).reshape(S, B * N).contiguous()
            sel, rows = decide(allr)
            x = x_cand.index_select(0, L.up(of_row[rows]))
            old = [cls[r] for r in rows.tolist()]
            first = {}
            for r, c in enumerate(old):                                                # a class is named by its lowest member among the NEW rows
                first.setdefault(c, r)
            cls = [first[c] for c in old]
            continue
        cls = list(range(S * B))
        eps_l = L.up(eps[:, lo:hi].reshape(S * B * nl, *shape1))
        x_cand, x0 = L.step(x, t_steps[i], t_steps[i + 1], i, eps_l, lab, interleave=True, first_denoised=True)
        loc = L.score(p.scorer, x0, lab).to(L.dev, torch.float32).view(S * B, nl).t().contiguous().reshape(-1)   # candidate-major
        # the draws never depend on search results: the next step's are made (in the reference's order) while the GPU runs this step --
        # in line they left it idle for the 10 ms that 64 x [3, 64, 64] float64 normals take on the host
        eps = draw(i + 1) if i + 1 < L.num_steps else None
        allr = L.shards.gather_rewards(loc, N, S * B).view(N, S * B).t().contiguous().cpu().reshape(S, B * N)
        sel, rows = decide(allr)
        # survivor (s, rank q) is candidate n = sel % N of beam row s*B + sel // N: this rank holds it iff lo <= n < hi
        cand = (sel % N).reshape(-1)
        src = rows * nl + (cand - lo).clamp(0, nl - 1)                                 # any valid row where the survivor is another rank's
        x = L.shards.exchange_rows(x_cand.index_select(0, L.up(src)), [L.shards.owner(n, N) for n in cand.tolist()])
    return x.view(S, B, *shape1)[:, 0].contiguous()


class _Lookahead:
    """Pulls items of a generator up to `depth` ahead of their use.  The search randomness never depends on search
    results (only the pivot does), so the host can draw iteration k+1's numbers -- in the reference's order -- while the
    GPU is still busy with iteration k.  `stage(item)` (optional) starts the item's host->device copy right away."""

    def __init__(self, gen, depth=2, stage=None):
        self.gen, self.depth, self.buf, self.stage = gen, depth, [], stage

    def prefetch(self):
        while len(self.buf) < self.depth:
            try:
                item = next(self.gen)
            except StopIteration:
                break
            self.buf.append(item if self.stage is None else self.stage(item))

    def get(self):
        if not self.buf:
            self.prefetch()
        return self.buf.pop(0)


def _eps_greedy_draws(L, p, pre, shape, lam):
    """The host-RNG stream of edm/main.py:724-797 in call order: per timestep one pivot, then per local-search
    iteration the N coins / Gaussians / hash-derived scales, each candidate's taken lane by lane (_Source.lanes).  An iteration yields the
    Gaussians as [N] tensors of [B, ...], mode int32 and scale float32 [N, L]: L = 1, the whole batch shares the coin of a candidate, or
    L = B, every image flips its own."""
    N, K, eps_p, src = p.N, p.K, p.eps, L.src
    lanes = src.lanes(shape)

    def candidate(i, k, n, lane, lshape):
        """(Gaussian [lshape], mode, scale) of candidate n as one lane draws it"""
        if src.rand1(lane) < (1 - eps_p):                                             # :751
            if pre is not None and i in pre and k < pre[i].shape[1] and n < pre[i].shape[2]:
                g = pre[i][:, k, n].reshape(lshape).to(torch.float64)
            else:
                g = src.randn(lane, lshape)                                           # :767
            s = torch.ones([lshape[0], 1, 1, 1]) * L.scale_fn(i, k, n) * lam          # float32, :779
            return g, 1, float(s.flatten()[0])
        key = f'fresh_{i}_{k}_{n}'
        return (pre[key].to(torch.float64) if (pre is not None and key in pre) else src.randn(lane, lshape)), 0, 0.0

    if not (pre is not None and 'pivot' in pre):
        src.images(shape[0], 1, shape[1:])                                            # :727, overwritten at :737
    for i in range(L.num_steps):
        yield pre[f'pivot_{i}'] if (pre is not None and f'pivot_{i}' in pre) else src.images(shape[0], 1, shape[1:])
        for k in range(K):
            rows = [[candidate(i, k, n, lane, lshape) for lane, lshape in lanes] for n in range(N)]      # candidate by candidate, lane by lane
            g_h = [_side_by_side([g for g, _, _ in r]) for r in rows]
            mode = torch.tensor([[m for _, m, _ in r] for r in rows], dtype=torch.int32)
            yield g_h, mode, torch.tensor([[s for _, _, s in r] for r in rows], dtype=torch.float32)


def _eps_greedy(L: _Loop, t_steps, x_next, labels, p, pre):
    """edm/main.py:714-860 (ZERO_ORDER and EPS_GREEDY share this branch in the reference)."""
    lam = p.lambda_param * np.sqrt(3 * 64 * 64)            # scaled by 3*64*64 whatever the resolution (:716)
    N, K, B = p.N, p.K, x_next.shape[0]
    shape = tuple(x_next.shape)
    L.shards.require_candidates(N, 'eps-greedy / zero-order search')
    if not L.shards.solo:
        # hash()-derived step sizes are salted per process (PYTHONHASHSEED): ranks must share ONE table or their candidates and
        # rebuilt pivots diverge.  Rank 0's table == the single-process run's.
        L.scale_fn = L.shards.replicate_scale_table(L.scale_fn, L.num_steps, K, N)
    lo, hi = L.shards.span(N)
    nl = hi - lo
    lab_l = None if labels is None else labels.repeat(nl, 1).contiguous()
    own = torch.arange(B)
    copy_stream = torch.cuda.Stream(device=L.dev)

    def stage(item):
        # candidate directions of this rank (6.3 MB of fp64 at N=64): pinned and sent on a side stream while the GPU runs the
        # previous iteration -- an in-line pageable upload left the GPU idle for ~3 ms of every 41 ms iteration
        sigma_step, stage.items = stage.items // (K + 1), stage.items + 1              # the stream is one pivot, then K iterations, per sigma step
        if not isinstance(item, tuple):
            return item                                                                # a pivot draw
        g_h, mode_t, scale_t = item
        if sigma_step in L.shared:
            return g_h, mode_t, scale_t, None, None, None                              # drawn as ever, not uploaded: no candidate batch is built
        host = pinned[stage.n % len(pinned)]                                           # ring: depth + 2 buffers, reused
        stage.n += 1
        if hi > lo:
            torch.cat(g_h[lo:hi], dim=0, out=host)
        with torch.cuda.stream(copy_stream):
            g_dev = host.to(L.dev, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(copy_stream)
        return g_h, mode_t, scale_t, g_dev, ready, host                                # `host` stays alive until the copy has run

    def decide(i, pivot, scores, g_h, mode_t, scale_t):
        """the end of a local-search iteration on its rewards `scores` [N, B]: the winners, recorded, and the pivot moved to them"""
        best = scores.argmax(dim=0)                                                    # first max (:842)
        L.rewards.append(scores)
        L.selected.append(best)
        if L.forced is not None:                                                       # follow another run's trajectory (B == 1)
            best = torch.tensor([L.forced[len(L.selected) - 1]])
        # rebuilt from the replicated host noise (no second collective) in one launch of B rows: row b carries its winner's mode and scale,
        # [N, L] read as [N, B] -- its own lane's, or the one lane's for every image
        g_w = torch.stack([g_h[j][b] for b, j in enumerate(best.tolist())])
        m_w, s_w = mode_t.expand(N, B)[best, own], scale_t.expand(N, B)[best, own]
        pivot = ops.candidate_noise_rows(pivot, L.up(g_w), L.up(m_w), L.up(s_w))
        if L.record_noises:                                                            # best_noises_this_timestep (:741, :854)
            L.best_noises.setdefault(i, []).append(pivot.cpu())
        return best, pivot

    stage.n = stage.items = 0
    pinned = [torch.empty((nl * B,) + shape[1:], dtype=torch.float64).pin_memory() for _ in range(4)]
    draws = _Lookahead(_eps_greedy_draws(L, p, pre, shape, lam), stage=stage)
    for i in range(L.num_steps):
        t_cur, t_next = t_steps[i], t_steps[i + 1]
        x_cur = x_next
        pivot = L.up(draws.get(), torch.float64)
        if i in L.shared:
            # share_identical: the noise coefficient of this step is 0, so all K * N candidates of an image are x_cur itself, every decision
            # is an exact tie (index 0) and the step taken is the pivot step, whatever the pivot: it is made first, on the drawn pivot, and
            # its second output -- what a candidate row scores -- is the reward of every candidate, computed once, by every rank for itself
            # (no candidate batch, no collective).  The draws are consumed and the pivot is rebuilt as ever (the stream of the later steps
            # and best_noises do not move)
            x_next, x0 = L.step(x_cur, t_cur, t_next, i, pivot, labels)                # :860
            loc = L.score(p.scorer, x0, labels).to(L.dev, torch.float32)
            draws.prefetch()
            scores = loc.reshape(1, B).cpu().expand(N, B)
            for k in range(K):
                _, pivot = decide(i, pivot, scores.clone(), *draws.get()[:3])
            continue
        for k in range(K):
            g_h, mode_t, scale_t, g_l, ready, _pinned = draws.get()                    # n-major rows (:800)
            torch.cuda.current_stream(L.dev).wait_event(ready)
            g_l.record_stream(torch.cuda.current_stream(L.dev))
            # one lane (B = 1 with its own seed included): a coin per candidate, the per-candidate launch; a lane per image: the per-row one
            build = ops.candidate_noise if L.src.L == 1 else ops.candidate_noise_rows
            cand = build(pivot, g_l, L.up(mode_t[lo:hi].reshape(-1)), L.up(scale_t[lo:hi].reshape(-1)))
            if L.chunk is None or L.chunk * B >= nl * B:
                x_cand, x0 = L.step(x_cur, t_cur, t_next, i, cand, lab_l, nb=nl * B)
                loc = L.score(p.scorer, x0, lab_l).to(L.dev, torch.float32)
            else:
                # candidate_chunk: this rank's candidates go through the denoiser and the scorer in sequential pieces of `chunk` candidates
                # (n-major rows, so a piece is chunk * B consecutive rows) -- exactly the launches rank r of N / chunk ranks issues for
                # its share, on one GPU
                xs, locs = [], []
                for a in range(0, nl * B, L.chunk * B):
                    z = min(nl * B, a + L.chunk * B)
                    lab_c = None if lab_l is None else lab_l[a:z].contiguous()
                    xc_, x0_ = L.step(x_cur, t_cur, t_next, i, cand[a:z].contiguous(), lab_c, nb=z - a)
                    xs.append(xc_.clone())
                    locs.append(L.score(p.scorer, x0_, lab_c).to(L.dev, torch.float32).clone())
                x_cand, loc = torch.cat(xs, dim=0), torch.cat(locs, dim=0)
            draws.prefetch()                                                           # host draws overlap the queued GPU work
            best, pivot = decide(i, pivot, L.shards.gather_rewards(loc, N, B).reshape(N, B).cpu(), g_h, mode_t, scale_t)
        if L.reuse_winner and K > 0:       # the step the reference recomputes at :860 for the final pivot IS the winner's row of the last iteration
            x_next = L.winner_rows(x_cand, best, N, lambda b, j: j * B + b)
        else:
            x_next, _ = L.step(x_cur, t_cur, t_next, i, pivot, labels)                 # :860
    return x_next


class _Node:
    __slots__ = ('x', 'children', 'reward', 'visit')

    def __init__(self, x, visit=0):
        self.x, self.children, self.reward, self.visit = x, [], 0, visit


# granularity the ragged rollout batches are padded to (copies of row 0, not counted as evaluations).  1 = no padding: every batch size
# 1 .. 16 gets its own captured HIP graph (graphs.py SMALL budget); 4 = the former rule (four batch shapes, up to 3 wasted rows per forward)
# DTS_MCTS_PAD_ROWS sets it.  DTS_MCTS_PAD keeps the boolean meaning it had through round 4 ('1' = pad to multiples of four, '0' = no padding).
def _mcts_pad_rows():
    v = os.environ.get('DTS_MCTS_PAD_ROWS')
    if v is None:
        legacy = os.environ.get('DTS_MCTS_PAD')
        return 4 if legacy is not None and legacy.strip() not in ('', '0') else 1
    try:
        return max(1, min(16, int(v)))
    except ValueError:
        import warnings
        warnings.warn(f'DTS_MCTS_PAD_ROWS={v!r} is not an integer: rollout batches are not padded')
        return 1


MCTS_PAD_ROLLOUTS = _mcts_pad_rows()


def _mcts(L: _Loop, t_steps, x_next, labels, p, pre):
    """edm/main.py:405-713.  Tree statistics, UCB1 selection and the numpy child draw are the reference's; the
    tensor work is re-batched without changing any value: a node's b expansions are one batched step (same x,
    b noises) and the group's deterministic zero-noise rollouts advance together, one batched step per timestep
    over the simulations that have reached it (the reference runs them one by one, batch 1)."""
    b, S, B, ns = p.N, p.S, x_next.shape[0], L.num_steps
    shape1 = tuple(x_next.shape[1:])
    results = []
    L.shards.sync_numpy_rng()                         # replicas must draw the same rollout children (edm/main.py:593)
    mbs = min(2, B)
    for mb0 in range(0, B, mbs):
        xb = x_next[mb0:mb0 + mbs]
        lb = None if labels is None else labels[mb0:mb0 + mbs]
        m = xb.shape[0]
        noise = {}
        for i in range(ns):
            if pre is not None and i in pre:
                noise[i] = L.up(pre[i].repeat(m, 1, 1, 1, 1))
            else:
                noise[i] = L.up(torch.randn(m, b, *shape1))                           # float32 (:446)
        roots = [_Node(xb[s:s + 1].clone(), visit=1) for s in range(m)]
        lab1 = lambda s: None if lb is None else lb[s:s + 1]
        for i in range(ns):
            t_cur, t_next = t_steps[i], t_steps[i + 1]
            todo = [(s, j) for s in range(m) if not roots[s].children for j in range(b)]
            if todo:
                xe = torch.cat([roots[s].x for s, j in todo], dim=0)
                ne = torch.cat([noise[i][s:s + 1, j] for s, j in todo], dim=0).contiguous()
                le = None if lb is None else torch.cat([lb[s:s + 1] for s, j in todo], dim=0).contiguous()
                xn, _ = L.step(xe, t_cur, t_next, i, ne, le)
                for q, (s, j) in enumerate(todo):
                    roots[s].children.append(_Node(xn[q:q + 1]))
            group = min(16, S * m)
            for g0 in range(0, S * m, group):
                paths, starts = [], []
                for sim in range(g0, min(g0 + group, S * m)):
                    s = sim % m
                    node, it = roots[s], i
                    tc, tn = t_cur, t_next
                    path = [node]
                    while node.children:
                        ucb = [float('inf') if c.visit == 0 else
                               c.reward / c.visit + np.sqrt(2 * np.log(node.visit) / c.visit) for c in node.children]
                        node = node.children[int(np.argmax(ucb))]
                        it += 1
                        if it < ns:
                            tc, tn = t_steps[it], t_steps[it + 1]
                        path.append(node)
                    if it < ns - 1:
                        for j in range(b):
                            torch.randn(1, *shape1)            # the reference's eager .get() default (:578-579): drawn, unused
                        eb = noise[it][s].contiguous()                                  # [b, ...] f32
                        lbb = None if lb is None else lb[s:s + 1].repeat(b, 1).contiguous()
                        xc, _ = L.step(node.x, tc, tn, it, eb, lbb, nb=b)
                        for j in range(b):
                            node.children.append(_Node(xc[j:j + 1]))
                        node = node.children[np.random.randint(0, len(node.children))]   # numpy global RNG (:593)
                        it += 1
                        path.append(node)
                    paths.append(path)
                    starts.append((node.x, it, s))
                # batched ragged rollouts; sharded: rank r advances the simulations [lo, hi) of this group and the
                # group's rewards are all-gathered (the tree itself is replicated: SURVEY.md section 8e)
                nsim = len(starts)
                slo, shi = L.shards.span(nsim)
                mine = list(range(slo, shi))
                cur = {q: starts[q][0].clone() for q in mine}
                if mine:
                    for j in range(min(starts[q][1] for q in mine), ns):
                        act = [q for q in mine if starts[q][1] <= j]
                        xa = torch.cat([cur[q] for q in act], dim=0)
                        la = None if lb is None else torch.cat([lb[starts[q][2]:starts[q][2] + 1] for q in act], dim=0).contiguous()
                        # the number of live rollouts changes from step to step (1 .. 16).  Every size replays its own captured HIP graph
                        # (graphs.py keeps up to 16 small shapes per module) instead of launching ~600 kernels one by one from the host.
                        # DTS_MCTS_PAD_ROWS=4 restores the former rule -- sizes rounded up to a multiple of 4 with copies of row 0, four shapes --
                        # which cost up to 3 wasted rows per forward at ~0.5 ms per row (profiles/r05_experiments.txt item 13).  Rows are
                        # independent of each other's VALUES; they can depend on the batch SIZE in the last bits, because the conv launchers
                        # choose the split-K factor / launch form from the row count (another fixed f32 summation order -- as is every
                        # batch size against the reference's batch-1 rollouts, edm/main.py:640-660).  Padding rows are not counted as evaluations.
                        ka = len(act)
                        g_ = MCTS_PAD_ROLLOUTS if (ka <= 16 and getattr(L.net, 'dtype', None) != torch.float32) else 1
                        kp = -(-ka // g_) * g_
                        if kp > ka:
                            xa = torch.cat([xa, xa[:1].expand(kp - ka, *xa.shape[1:])], dim=0)
                            if la is not None:
                                la = torch.cat([la, la[:1].expand(kp - ka, la.shape[1])], dim=0).contiguous()
                        xo, _ = L.step(xa, t_steps[j], t_steps[j + 1], j, torch.zeros_like(xa), la, live=ka)
                        for r_, q in enumerate(act):
                            cur[q] = xo[r_:r_ + 1]
                    den = torch.cat([cur[q] for q in mine], dim=0)
                    sl = None if lb is None else torch.cat([lb[starts[q][2]:starts[q][2] + 1] for q in mine], dim=0).contiguous()
                    loc = L.score(p.scorer, den, sl).to(L.dev, torch.float32)
                else:
                    loc = torch.empty(0, dtype=torch.float32, device=L.dev)
                rew = L.shards.gather_rewards(loc, nsim, 1).cpu()
                L.rewards.append(rew)
                for path, r in zip(paths, rew):
                    for nd in path:
                        nd.reward += r.item()
                        nd.visit += 1
            for s in range(m):
                best, best_r, best_j = None, -float('inf'), -1
                for j, c in enumerate(roots[s].children):
                    if c.visit > 0 and c.reward / c.visit > best_r:
                        best, best_r, best_j = c, c.reward / c.visit, j
                assert best is not None
                L.selected.append(torch.tensor([best_j]))
                roots[s] = best
        results += [r.x for r in roots]
    return torch.cat(results, dim=0)


# granularity the lock-step MCTS batches ABOVE 16 rows are padded to (copies of row 0, not counted as evaluations): with S searches the
# expansion and rollout batches take every size up to 16 * S, and each size would be a launch form and a captured graph of its own (graphs.py
# keeps 4 large shapes per module).  Batches of at most 16 rows keep the rule above.  DTS_MCTS_LOCKSTEP_PAD_ROWS sets it (1 = no padding);
# the choice is measured: DESIGN.md section 5, "MCTS in lock-step".
def _mcts_lockstep_pad_rows():
    v = os.environ.get('DTS_MCTS_LOCKSTEP_PAD_ROWS')
    try:
        return 32 if v is None else max(1, int(v))
    except ValueError:
        import warnings
        warnings.warn(f'DTS_MCTS_LOCKSTEP_PAD_ROWS={v!r} is not an integer: the default granule is used')
        return 32


MCTS_LOCKSTEP_PAD_ROWS = _mcts_lockstep_pad_rows()


def _pad_rows(t, rows):
    """t [k, ...] with copies of its row 0 appended up to `rows` rows"""
    return t if t.shape[0] >= rows else torch.cat([t, t[:1].expand(rows - t.shape[0], *t.shape[1:])], dim=0).contiguous()


def _mcts_lockstep(L: _Loop, t_steps, x_next, labels, p, pre):
    """generate_image_grid(row_seeds=..., mcts_lockstep=True): the MCTS searches of n seeds as one batch.  Search s is `_mcts` with B = 1 (one
    tree; the reference's micro-batch of two images does not arise) on streams of its own: its torch draws -- the num_steps float32 draws
    [1, b, C, H, W] up front, then the b discarded [1, C, H, W] draws of every expanding simulation -- come from lane s of `L.src`, its
    child draws from numpy.random.RandomState(row_seeds[s]), the stream numpy's global generator gives after numpy.random.seed(row_seeds[s]);
    the global generator is neither read nor advanced.  The trees are aligned by simulation index.  Per sigma step i (all roots at depth i):
      root expansions   of every search whose root has no children: one scalar-sigma step of <= n * b rows;
      simulation k      (serial: simulation k + 1 of a search may descend into the node simulation k made) every search descends its own
                        tree on the host; the expansions of all searches that expand at k -- each at the sigma step of its own leaf --
                        are ONE `heun_step_rows` of <= n * b rows with t_hat, noise coefficient, t_next and the network's sigma per row;
      rollouts          of the group's simulations of all searches advance together, one scalar step per sigma step j over those that have
                        reached it (<= 16 * n rows);
      scoring           one scorer call for the group's n * group final states, then back-propagation and the root's best child per search.
    Batches above 16 rows are padded to MCTS_LOCKSTEP_PAD_ROWS (expansions: to whole nodes of b rows); padding is not counted."""
    b, S, n, ns = p.N, p.S, x_next.shape[0], L.num_steps
    shape1 = tuple(x_next.shape[1:])
    rngs = [np.random.RandomState(s) for s in L.row_seeds]
    noise = [torch.stack([L.src.randn(s, (1, b) + shape1, dtype=torch.float32)[0] for i in range(ns)]) for s in range(n)]   # :446, lane by lane
    noise = L.up(torch.stack(noise, dim=1))                                        # [ns, n, b, ...] float32
    roots = [_Node(x_next[s:s + 1].clone(), visit=1) for s in range(n)]
    rows = [0] * n                                                                 # denoiser rows of each search: what its solo call counts
    G = MCTS_LOCKSTEP_PAD_ROWS
    churn = [L.churn(t_steps[i]) for i in range(ns)]
    stages = lambda j: 1 if j >= ns - 1 else 2

    def lab_of(searches, rep=1):
        if labels is None:
            return None
        return labels.index_select(0, L.up(torch.tensor(searches))).repeat_interleave(rep, dim=0).contiguous()

    def padded(k):
        """rows a batch of k live rows is launched with"""
        if k <= 16:
            g_ = MCTS_PAD_ROLLOUTS if getattr(L.net, 'dtype', None) != torch.float32 else 1
            return -(-k // g_) * g_
        return -(-k // G) * G

    def padded_nodes(k):
        """nodes a batch of k expanding nodes (b rows each) is launched with: whole nodes, the rows of a node stay together"""
        unit = max(1, G // b)
        return k if k * b <= 16 else -(-k // unit) * unit

    for i in range(ns):
        todo = [s for s in range(n) if not roots[s].children]
        if todo:
            nodes = padded_nodes(len(todo))
            xe = _pad_rows(torch.cat([roots[s].x for s in todo], dim=0), nodes)
            ne = _pad_rows(noise[i].index_select(0, L.up(torch.tensor(todo))).reshape(len(todo) * b, *shape1), nodes * b)
            xn, _ = L.step(xe, t_steps[i], t_steps[i + 1], i, ne, lab_of(todo + todo[:1] * (nodes - len(todo)), b), interleave=True,
                           live=len(todo) * b)
            for q, s in enumerate(todo):
                roots[s].children = [_Node(xn[q * b + j:q * b + j + 1]) for j in range(b)]
                rows[s] += b * stages(i)
        group = min(16, S)
        for g0 in range(0, S, group):
            sims = range(g0, min(g0 + group, S))
            paths = [[] for _ in range(n)]
            starts = [[] for _ in range(n)]
            for k in sims:
                leaves = []
                for s in range(n):
                    node, it = roots[s], i
                    path = [node]
                    while node.children:
                        ucb = [float('inf') if c.visit == 0 else
                               c.reward / c.visit + np.sqrt(2 * np.log(node.visit) / c.visit) for c in node.children]
                        node = node.children[int(np.argmax(ucb))]
                        it += 1
                        path.append(node)
                    leaves.append((node, it, path))
                grow = [s for s in range(n) if leaves[s][1] < ns - 1]
                if grow:
                    for s in grow:
                        for j in range(b):
                            L.src.randn(s, (1,) + shape1, dtype=torch.float32)    # the reference's eager .get() default (:578-579): drawn, unused
                    its = [leaves[s][1] for s in grow]
                    nodes = padded_nodes(len(grow))
                    xe = _pad_rows(torch.cat([leaves[s][0].x for s in grow], dim=0), nodes)
                    ne = _pad_rows(torch.cat([noise[it][s] for s, it in zip(grow, its)], dim=0), nodes * b)
                    le = lab_of(grow + grow[:1] * (nodes - len(grow)), b)
                    per_row = lambda v: [v[it] for it in its + its[:1] * (nodes - len(its)) for _ in range(b)]
                    xc = L.step_rows(xe, per_row([c[0] for c in churn]), per_row([c[1] for c in churn]),
                                     per_row([float(t) for t in t_steps[1:]]), ne, le, live=len(grow) * b)
                    L.mcts_ragged_launches += 1
                    L.mcts_mixed_launches += len(set(its)) > 1
                    for q, s in enumerate(grow):
                        node, it, path = leaves[s]
                        node.children = [_Node(xc[q * b + j:q * b + j + 1]) for j in range(b)]
                        rows[s] += 2 * b
                        node = node.children[rngs[s].randint(0, b)]                # :593, from the search's own numpy stream
                        path.append(node)
                        leaves[s] = (node, it + 1, path)
                for s in range(n):
                    paths[s].append(leaves[s][2])
                    starts[s].append((leaves[s][0].x, leaves[s][1]))
            # the group's rollouts of all searches, search-major; every live row at sigma step j shares its scalars
            flat = [(s, q) for s in range(n) for q in range(len(sims))]
            cur = {sq: starts[sq[0]][sq[1]][0] for sq in flat}
            for j in range(min(starts[s][q][1] for s, q in flat), ns):
                act = [sq for sq in flat if starts[sq[0]][sq[1]][1] <= j]
                ka = len(act)
                kp = padded(ka)
                xa = _pad_rows(torch.cat([cur[sq] for sq in act], dim=0), kp)
                la = lab_of([s for s, _ in act] + [act[0][0]] * (kp - ka))
                xo, _ = L.step(xa, t_steps[j], t_steps[j + 1], j, torch.zeros_like(xa), la, live=ka)
                for r_, sq in enumerate(act):
                    cur[sq] = xo[r_:r_ + 1]
                    rows[sq[0]] += stages(j)
            den = torch.cat([cur[sq] for sq in flat], dim=0)
            rew = L.score(p.scorer, den, lab_of([s for s, _ in flat])).to(L.dev, torch.float32).cpu().reshape(n, len(sims))
            L.rewards.append(rew)
            for s in range(n):
                for path, r in zip(paths[s], rew[s]):
                    for nd in path:
                        nd.reward += r.item()
                        nd.visit += 1
        chosen = []
        for s in range(n):
            best, best_r, best_j = None, -float('inf'), -1
            for j, c in enumerate(roots[s].children):
                if c.visit > 0 and c.reward / c.visit > best_r:
                    best, best_r, best_j = c, c.reward / c.visit, j
            assert best is not None
            chosen.append(best_j)
            roots[s] = best
        L.selected.append(torch.tensor(chosen))
    L.search_rows = rows
    return torch.cat([r.x for r in roots], dim=0)


_METHODS = {
    SamplingMethod.NAIVE: _naive, SamplingMethod.REJECTION_SAMPLING: _rejection, SamplingMethod.BEAM_SEARCH: _beam,
    SamplingMethod.MCTS: _mcts, SamplingMethod.ZERO_ORDER: _eps_greedy, SamplingMethod.EPS_GREEDY: _eps_greedy,
}


@torch.no_grad()
def generate_image_grid(
    network_pkl, dest_path, latents, class_labels,
    seed=0, gridw=8, gridh=8, device=torch.device('cuda'),
    num_steps=18, sigma_min=0.002, sigma_max=80, rho=7,
    S_churn=0, S_min=0, S_max=float('inf'), S_noise=1,
    sampling_method: SamplingMethod = SamplingMethod.NAIVE,
    sampling_params: Optional[Dict[str, Any]] = None,
    precomputed_noise: Optional[Dict[Any, torch.Tensor]] = None,
    *, scale_fn: Callable[[int, int, int], float] = builtin_scale, compute_dtype=ops.F16X3, verbose=True,
    reuse_winner: Optional[bool] = None, record_noises: bool = False, shard_candidates: bool = True,
    forced_selections: Optional[Sequence[int]] = None, candidate_chunk: Optional[int] = None, beam_search: bool = False,
    row_seeds: Optional[Sequence[int]] = None, share_identical: bool = False, mcts_lockstep: bool = False,
):
    """Same positional/keyword surface as edm/main.py:47-55.  Keyword-only extras: `scale_fn` (the hash-derived step
    table, edm/main.py:776), `compute_dtype` (default ops.F16X3: split precision, the reference's fp32 selections at a third of the 16-bit
    rate; float32 = parity mode on the f32 matrix instruction; bfloat16 / float16 = throughput modes), `verbose`, `reuse_winner` (see below), `record_noises`
    (keep the per-iteration winning noises for `dump_noise_trajectory`; costs one D2H copy per iteration), `forced_selections` (eps-greedy /
    zero-order, one image: decision d continues from candidate forced_selections[d] instead of its own argmax, which is still what
    `selected` records -- how a search is walked along ANOTHER run's trajectory so that every decision of the two stays comparable; the
    parity tests follow the reference's recorded run this way; it must hold num_steps * K indices in [0, N), and in a sharded run every
    rank must pass the same list: the override is applied after the reward all-gather, on every rank alike), `candidate_chunk` (eps-greedy /
    zero-order: evaluate the candidates of an iteration in sequential pieces of that many candidates instead of one batch -- the kernels,
    split-K factors and launch forms a rank of a sharded run uses for a share of that size, on one GPU; values are the batched run's up to
    the f32 summation order those launch forms imply), `beam_search` (SamplingMethod.BEAM_SEARCH only.  False, the default: the reference's
    branch as it stands -- it reads `method_params.b` / `.k`, which SamplingParams does not define, and raises AttributeError.  True: the search
    that branch sets out to do, `_beam_search`: B = sampling_params['B'] beams per image (the reference's k) x N = sampling_params['N']
    candidates per beam (its b), per sigma step the top B of an image's B*N rewards survive in rank order, exact ties to the lower flat index
    j*N + n; `precomputed_noise[i]` of shape [S, B, N, C, H, W] replaces the draws of step i; the result dict gains `beam_parents`, and
    `rewards` / `selected` hold one [S, B*N] / [S, B] tensor per sigma step), `row_seeds` (one seed per image: image b takes every host draw
    of the search from its own generator seeded row_seeds[b], in the order and shapes of a one-image call with seed=row_seeds[b], so its
    search is that call's whatever else is in the batch -- up to the launch forms the row count selects -- and the searches of many seeds
    run in lock-step as one batch (bulk.generate_seeds(search_batch=...)); eps-greedy / zero-order coins then differ from image to image:
    mode / scale are [N, B] instead of [N, 1] and the candidates come from ops.candidate_noise_rows (the rebuilt pivots always do, one launch
    of B rows); the result dict gains `row_seeds`;
    not with MCTS (but see `mcts_lockstep`), forced_selections, precomputed_noise or candidates sharded over ranks), `mcts_lockstep`
    (SamplingMethod.MCTS with row_seeds only; `_mcts_lockstep`: the trees of the seeds advance as one batch, aligned by simulation index, the
    expansions of one index -- each search at the sigma step of its own leaf -- in ONE step with per-row scalars.  Search b is the one-image
    call seed=row_seeds[b] made after numpy.random.seed(row_seeds[b]): its torch draws come from its own generator and its rollout child
    draws from numpy.random.RandomState(row_seeds[b]); numpy's global generator is neither read nor advanced, which is a deviation from
    the reference of this mode alone.  `selected` holds one [S] tensor per sigma step, `rewards` one
    [S, group] tensor per (sigma step, group of simulations); the result dict gains `search_rows` (the denoiser rows of each search; `net_rows` is
    their sum, padding rows are not counted), `mcts_ragged_launches` (per-row step launches) and `mcts_mixed_launches` (those that held rows
    of at least two sigma steps)), `share_identical` (eps-greedy / zero-order and
    beam_search=True; not the reference's.  True: at the sigma steps `identical_steps` lists -- noise coefficient exactly 0, so every
    candidate is the unchanged state -- the identical rows go through the denoiser and the scorer once instead of K * N times per image (beam:
    one row per class of beam rows known to be equal).  Draws, selections (exact ties, index 0), the pivot steps and so `x`, `image` and
    `best_noises` are those of the full run; the rewards of such a step are one value per image up to the launch form of the smaller batch;
    `net_rows` is the actual, lower count (eps-greedy: by `shared_rows_saved`), and a sharded run makes no collective at such a step.  The
    result dict's `shared_steps` lists the steps, [] when the keyword is off).  Writes the PNG grid like the
    reference when `dest_path` is not None and additionally returns a dict with the final state and the search trace."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('generate_image_grid (HIP): device must be a GPU; the CPU path is the reference itself')
    torch.manual_seed(seed)                                                           # edm/main.py:58
    p = SamplingParams(**(sampling_params or {}))
    if verbose:
        print(f'Using sampling method: {sampling_method.name}')
    net = load_network(network_pkl, device=device, dtype=compute_dtype)
    shards = CandidateShards(enabled=shard_candidates)     # False: this rank runs the whole search (bulk.py shards seeds instead)
    t_steps = grid_schedule(net, num_steps, sigma_min, sigma_max, rho)              # edm/main.py:78-80 (host)
    L = _Loop(net, device, num_steps, S_churn, S_min, S_max, S_noise, scale_fn, shards)
    # eps-greedy: the reference re-runs step() at batch 1 for the final pivot of each timestep (edm/main.py:860) although
    # that row was just computed in the last candidate batch.  The default mode (f16x3) and float32 recompute it like the reference, so
    # `net_rows` equals the reference's count (config 3: 8 995); the 16-bit throughput modes reuse the row (8 960 rows, same values).
    L.reuse_winner = (compute_dtype not in (torch.float32, ops.F16X3)) if reuse_winner is None else bool(reuse_winner)
    L.record_noises = bool(record_noises)
    if mcts_lockstep:
        if sampling_method != SamplingMethod.MCTS:
            raise ValueError(f'mcts_lockstep=True: SamplingMethod.MCTS only, got {sampling_method.name}')
        if row_seeds is None:
            raise ValueError('mcts_lockstep=True: needs row_seeds (one seed per image: every search runs on its own torch and numpy streams)')
        for name, given in (('forced_selections', forced_selections is not None), ('precomputed_noise', precomputed_noise is not None)):
            if given:
                raise ValueError(f'mcts_lockstep=True: {name} is not supported with per-image random streams')
        if not shards.solo:
            raise ValueError('mcts_lockstep=True: candidate sharding over more than one rank is not supported (shard_candidates=False: '
                             'lock-step batches go with seed sharding)')
    if row_seeds is not None:
        row_seeds = [int(s) for s in row_seeds]
        if len(row_seeds) != latents.shape[0]:
            raise ValueError(f'row_seeds: need one seed per image, got {len(row_seeds)} seeds for {latents.shape[0]} images')
        if sampling_method == SamplingMethod.MCTS and not mcts_lockstep:
            raise ValueError('row_seeds: SamplingMethod.MCTS is not supported (its numpy child draw and its ragged trees are per search)')
        for name, given in (('forced_selections', forced_selections is not None), ('precomputed_noise', precomputed_noise is not None)):
            if given:
                raise ValueError(f'row_seeds: {name} is not supported with per-image random streams')
        if not shards.solo:
            raise ValueError('row_seeds: candidate sharding over more than one rank is not supported (shard_candidates=False: lock-step '
                             'batches go with seed sharding)')
        L.src, L.row_seeds = _Source(row_seeds), row_seeds
    if forced_selections is not None:
        if sampling_method not in (SamplingMethod.EPS_GREEDY, SamplingMethod.ZERO_ORDER) or latents.shape[0] != 1:
            raise ValueError('forced_selections: eps-greedy / zero-order search of one image only')
        L.forced = [int(v) for v in forced_selections]
        if len(L.forced) != num_steps * p.K or any(not 0 <= v < p.N for v in L.forced):
            raise ValueError(f'forced_selections: need num_steps * K = {num_steps * p.K} indices in [0, {p.N}), got {len(L.forced)} '
                             f'(range {min(L.forced, default=None)} .. {max(L.forced, default=None)})')
    if candidate_chunk is not None:
        if sampling_method not in (SamplingMethod.EPS_GREEDY, SamplingMethod.ZERO_ORDER) or int(candidate_chunk) < 1:
            raise ValueError('candidate_chunk: a positive candidate count, eps-greedy / zero-order search only')
        L.chunk = int(candidate_chunk)
    method_fn = _mcts_lockstep if mcts_lockstep else _METHODS[sampling_method]
    if share_identical:
        if sampling_method not in (SamplingMethod.EPS_GREEDY, SamplingMethod.ZERO_ORDER) and not beam_search:
            raise ValueError(f'share_identical=True: eps-greedy / zero-order search or beam_search=True only, got {sampling_method.name}')
        L.shared = frozenset(identical_steps(t_steps, num_steps, S_churn, S_min, S_max, S_noise, net.round_sigma))
    if beam_search:
        if sampling_method != SamplingMethod.BEAM_SEARCH:
            raise ValueError(f'beam_search=True: SamplingMethod.BEAM_SEARCH only, got {sampling_method.name}')
        for name, given in (('forced_selections', forced_selections is not None), ('candidate_chunk', candidate_chunk is not None),
                            ('record_noises', bool(record_noises))):
            if given:
                raise ValueError(f'beam_search=True: {name} is not supported by the beam search')
        if int(p.B) < 1 or int(p.N) < 1:
            raise ValueError(f'beam_search=True: need B >= 1 beams and N >= 1 candidates per beam, got B={p.B}, N={p.N}')
        method_fn = _beam_search
    x0 = (latents.to(torch.float64).cpu() * t_steps[0]).to(device).contiguous()       # edm/main.py:99
    labels = None if class_labels is None else class_labels.to(device, torch.float32).contiguous()
    evals0 = getattr(net, 'evals', 0)
    x_next = method_fn(L, t_steps, x0, labels, p, precomputed_noise)
    image = ops.quantize_u8(x_next)                                                   # edm/main.py:869
    scores = p.scorer(image.clone(), labels, torch.zeros(image.shape[0], device=device))
    avg_score = float(scores.float().mean())
    if verbose:
        print(f'Average score: {avg_score}')
    img_cpu = image.cpu()
    if dest_path is not None and (shards.rank == 0 or not shard_candidates):
        import PIL.Image
        if verbose:
            print(f'Saving image grid to "{dest_path}"...')
        r, c = net.img_resolution, net.img_channels
        grid = img_cpu.reshape(gridh, gridw, *img_cpu.shape[1:]).permute(0, 3, 1, 4, 2).reshape(gridh * r, gridw * r, c)
        PIL.Image.fromarray(grid.numpy(), 'RGB').save(dest_path)
    if verbose:
        print('Done.')
    res = dict(x=x_next, image=img_cpu, final_scores=scores.cpu(), avg_score=avg_score, t_steps=t_steps,
               rewards=L.rewards, selected=L.selected, beam_parents=L.beam_parents, net_rows=getattr(net, 'evals', 0) - evals0,
               collectives=shards.collectives, shared_steps=sorted(L.shared), best_noises={i: torch.stack(v) for i, v in L.best_noises.items()})
    if row_seeds is not None:
        res['row_seeds'] = row_seeds
    if mcts_lockstep:
        res.update(search_rows=L.search_rows, mcts_ragged_launches=L.mcts_ragged_launches, mcts_mixed_launches=L.mcts_mixed_launches)
    return res


def dump_noise_trajectory(result, directory='.'):
    """Write the winning noise of every local-search iteration in the format the reference's diffusion-map tool loads
    (edm/dmap.py:16-24): `all_timestep_noises.pkl` = {timestep index: Tensor[K, B, C, H, W]} and `t_steps.pkl`.  The
    reference's loop collects exactly this list (edm/main.py:739-741, 853-854) but never writes it; `result` is the
    dict returned by `generate_image_grid(..., record_noises=True)`."""
    import pickle
    if not result.get('best_noises'):
        raise ValueError('no noise trajectory recorded: call generate_image_grid(..., record_noises=True) with a local-search method')
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, 'all_timestep_noises.pkl'), 'wb') as f:
        pickle.dump({int(i): v.cpu() for i, v in result['best_noises'].items()}, f)
    with open(os.path.join(directory, 't_steps.pkl'), 'wb') as f:
        pickle.dump(result['t_steps'].cpu(), f)
