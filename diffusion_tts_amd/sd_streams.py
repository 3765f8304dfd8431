"""Host random streams of the SD backend's search loop (sd_pipeline.SDSearchPipeline): one per search.

A seed `s` gives a `torch.Generator().manual_seed(s)`: its stream is the global CPU generator's after `torch.manual_seed(s)`, so the draws of
seed s in any batch are the draws of `main.py --backend sd --seed s` -- first the float32 latents [1,C,h,w] (main.py's own draw, made here
only when the caller passes none), then everything the reference's loop draws, in the reference's order and in the latents' dtype
(pipeline_stable_diffusion.py:1080, 1109, 1366-1379, 1410; scheduling_ddim.py:457-460).  `seed=None` is the global CPU generator itself, as
it stands: the single search of a call without `row_seeds`.  Host tensors only: nothing here needs a GPU."""
import numpy as np
import torch


class SeedStream:
    """The draws of ONE search.  `shape` is the search's latent shape [1,C,H,W], `dtype` the latents' dtype (a float16 normal draw is
    another stream than a float32 draw rounded to float16, so every loop draw is made in `dtype`, as the reference's `randn_like` does)."""

    def __init__(self, seed, shape, dtype):
        self.seed = None if seed is None else int(seed)
        self.gen = None if seed is None else torch.Generator().manual_seed(self.seed)      # None: torch's global generator, not reseeded
        self.shape, self.dtype = tuple(shape), dtype

    def latents(self):
        """main.py's `torch.randn(1, C, h, w)`: float32 whatever the loop's dtype"""
        return torch.randn(self.shape, generator=self.gen)

    def randn(self):
        return torch.randn(self.shape, dtype=self.dtype, generator=self.gen)

    def rand(self):
        return torch.rand(1, generator=self.gen).item()

    def local_round(self, n, thr, lam):
        """One eps-greedy / zero-order iteration (pipeline...:1371-1379, 1410): per candidate the coin, the Gaussian and -- for a step around
        the pivot -- the step length; then the n variance noises `scheduler.step` draws and drops.  Returns (draws [n,*shape], mode [n],
        scale [n][3] = (rand, lambda, sqrt(numel)), zeros for a fresh Gaussian) as ops.candidate_noise_sd takes them."""
        root = float(np.sqrt(self.shape[-1] * self.shape[-2] * self.shape[-3]))
        draws, mode, scale = [], [], []
        for _ in range(n):
            r = self.rand()
            draws.append(self.randn())
            if r < thr:
                mode.append(0)
                scale.append((0.0, 0.0, 0.0))
            else:
                mode.append(1)
                scale.append((self.rand(), float(lam), root))
        for _ in range(n):
            self.randn()
        return torch.stack(draws), mode, scale

    def beam_round(self, n):
        """One beam of one timestep (pipeline...:1080, 1109): its n candidate noises, then the n dropped variance noises.  -> [n,*shape]"""
        cands = torch.stack([self.randn() for _ in range(n)])
        for _ in range(n):
            self.randn()
        return cands

    def naive_trajectory(self, steps, draw_latents=True):
        """(latents or None, [steps] variance noises): all a naive trajectory draws (main.py's latents, then pipeline...:1366 per step)"""
        lat = self.latents() if draw_latents else None
        return lat, [self.randn() for _ in range(steps)]

    def rejection_trajectories(self, n, steps):
        """The reference's rejection loop (main.py:134) runs n naive trajectories one after the other on ONE stream; a naive trajectory draws
        a fixed number of tensors, so the n trajectories are drawn ahead in that order.  -> [(latents, [steps] noises)] * n"""
        return [self.naive_trajectory(steps) for _ in range(n)]
