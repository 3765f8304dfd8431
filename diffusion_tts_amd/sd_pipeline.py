"""The SD backend's noise-trajectory-search loop (drop-in for the reference's modified
`StableDiffusionPipeline.__call__`, sd/diffusers/.../pipeline_stable_diffusion.py:785-1485, from step 4 on) with
candidate-BATCHED evaluation.

BASELINE config 4 keeps the denoiser and the decoder as the stock diffusers modules ("diffusers U-Net path"): here
`unet` and `vae` are opaque callables with the diffusers call surface
    unet(sample, t, encoder_hidden_states=..., return_dict=False)[0]      vae.decode(z, return_dict=False)[0]
What this build replaces is everything around them: the DDIM scheduler step fused over the N candidates that share one
(x, eps) (`dts_ddim_candidates`, K13), classifier-free-guidance combine (`dts_cfg_combine`), quantisation (K10), and
the loop structure -- the reference evaluates the N candidates of an iteration ONE AT A TIME (batch 2 through the
U-Net, batch 1 through the VAE: pipeline...:1082-1129, 1383-1429); here all N go through the U-Net as one 2N-row call
and through the VAE as one N-row call.  Values are unchanged: rows are independent.

Host RNG: torch's CPU generator in the reference's call order (the pipeline's `--device cpu` run is the parity
oracle), including the variance-noise draws `scheduler.step` makes and drops when called without `variance_noise`
(scheduling_ddim.py:457-460).  Candidate construction (normalise + axpy, pipeline...:1371-1379) is a few KB of f32
arithmetic on the host, bit-identical to the reference, then uploaded.

Reference quirks kept: SD MCTS never scores or back-propagates (pipeline...:1201-1313), so every timestep takes the
FIRST expanded child; its rollouts only consume RNG.  The draws are reproduced; the dead U-Net work is skipped unless
`mcts_dead_compute=True`.  `mcts_backprop=True` (off by default: the default stays reference-faithful) runs the search the
reference's code sets out to do -- UCB1 selection, one expansion per simulation, a stochastic DDIM rollout to the last
timestep, decode + score, visit/reward back-propagation, best-mean child.

Multi-GPU (one process per GPU, torch.distributed over RCCL; parallel.CandidateShards): every rank replays the same
host RNG, so the candidate noises are known everywhere.  eps-greedy / zero-order shard the N candidates of an iteration, beam shards the
B*N candidates of a timestep; each rank runs the U-Net, the VAE decode and the scorer on its own candidates only and ONE all-gather of
the rewards per iteration (eps-greedy) / per timestep (beam) follows.  Survivors never travel: the eps-greedy survivor is a host noise
tensor, and a beam survivor's latent is one fused DDIM step of replicated inputs (the beam, its noise prediction, the candidate noise),
which every rank computes for all B*N candidates anyway (32 KB each) -- so no broadcast is needed and the collective count is exactly one
per search decision.  SD MCTS (reference-faithful default) never scores, so there is nothing to shard; `mcts_backprop` runs replicated.

One loop (`_search`) runs naive, eps-greedy, zero-order, beam and rejection for S searches in lock-step as ONE batch, rows search-major,
every search on its own host stream (sd_streams.SeedStream), selection on the host per search.  The candidates of all searches come from
one `dts_candidate_noise_sd_rows` launch, every DDIM candidate step from one `dts_ddim_candidates_groups` launch (S*B beams x N candidates in
the beam search).  `pipe(..., row_seeds=[s0, s1, ...])` gives it one stream per seed (what `main.py --backend sd --seed s` draws); the call
without `row_seeds` is its one-search case on torch's global generator as it stands, and the only one that shards candidates
(bulk.generate_sd_seeds shards seeds).  The two MCTS variants are single-search code of their own (ragged trees).

Prompt handling (pipeline...:812-814, 976-992, `encode_prompt` :330-460): with a `text_encoder` / `tokenizer` pair the
pipeline encodes `prompt` and `negative_prompt` itself exactly as `encode_prompt` does; `prompt_embeds` /
`negative_prompt_embeds` may be passed instead.  Missing `latents` are drawn like `prepare_latents` (:671-690).
"""
import types
from typing import Callable, Optional

import numpy as np
import torch

from . import ops
from .parallel import CandidateShards
from .sd_streams import SeedStream

LOCKSTEP_METHODS = ('naive', 'eps_greedy', 'zero_order', 'beam', 'rejection')


class DDIMScheduler:
    """Host mirror of the modified DDIMScheduler (scheduling_ddim.py): alpha table, `set_timesteps` ('leading' spacing),
    `_get_variance`, and `step` routed to the fused HIP kernel.  Defaults = SD-1.5's scheduler_config.json."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1, set_alpha_to_one=False):
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.num_train_timesteps, self.steps_offset = num_train_timesteps, steps_offset
        self.num_inference_steps = None
        self.init_noise_sigma = 1.0
        self.order = 1

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.steps_offset
        self.timesteps = torch.from_numpy(ts)
        return self.timesteps

    def scale_model_input(self, sample, timestep=None):
        return sample

    def coefficients(self, timestep, eta=1.0):
        """(alpha_t, alpha_prev, sigma_t) as f32 scalars (scheduling_ddim.py:403-405, 253-261, 431)."""
        timestep = int(timestep)
        prev = timestep - self.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[timestep]
        a_p = self.alphas_cumprod[prev] if prev >= 0 else self.final_alpha_cumprod
        var = ((1 - a_p) / (1 - a_t)) * (1 - a_t / a_p)
        return float(a_t), float(a_p), float(eta * var ** 0.5)

    def step(self, model_output, timestep, sample, eta=1.0, variance_noise=None, return_dict=False, generator=None):
        """(prev_sample, pred_original_sample); variance_noise may hold N candidates ([N, *sample.shape]) -> N prev samples."""
        a_t, a_p, sig = self.coefficients(timestep, eta)
        if variance_noise is None and eta > 0:
            variance_noise = torch.randn(model_output.shape, dtype=sample.dtype).to(sample.device)   # randn_tensor(..., dtype=model_output.dtype) on the CPU run (:457-460)
        z = variance_noise
        if z is not None and z.dim() == sample.dim():
            z = z.unsqueeze(0)
        prev, x0 = ops.ddim_candidates(sample.contiguous(), model_output.contiguous(), None if z is None else z.contiguous(), a_t, a_p, sig)
        if z is None or variance_noise.dim() == sample.dim():
            prev = prev[0]
        return prev, x0


class _MCTSNode:
    __slots__ = ('latents', 'children', 'parent', 'visits', 'total_reward', 'depth')

    def __init__(self, latents, parent=None):
        self.latents, self.children, self.parent = latents, [], parent
        self.visits, self.total_reward = 0, 0.0
        self.depth = 0 if parent is None else parent.depth + 1

    def ucb(self, c):                              # pipeline...:1185-1197
        if self.visits == 0:
            return float('inf')
        pv = self.parent.visits if self.parent else 1
        return self.total_reward / self.visits + c * np.sqrt(np.log(pv) / self.visits)


class SDSearchPipeline:
    def __init__(self, unet, vae, scheduler: Optional[DDIMScheduler] = None, device='cuda', mcts_dead_compute=False,
                 text_encoder=None, tokenizer=None, mcts_backprop=False, shards: Optional[CandidateShards] = None):
        """shards: candidate sharding over the ranks of the process group (default: CandidateShards(), a world of one outside
        torch.distributed); pass CandidateShards(enabled=False) to run the whole search on every rank."""
        self.shards = shards if shards is not None else CandidateShards()
        self.unet, self.vae = unet, vae
        self.scheduler = scheduler or DDIMScheduler()
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('SDSearchPipeline (HIP) needs a GPU device')
        self.mcts_dead_compute = mcts_dead_compute
        self.mcts_backprop = mcts_backprop
        self.text_encoder, self.tokenizer = text_encoder, tokenizer
        self._context_rows = {}                       # int32 device row maps of U-Nets with takes_context_rows (_eps_rows)
        self.unet_rows = 0
        self.decoded = 0                              # images through the VAE decoder on THIS rank
        self.scorer_calls = 0

    @torch.no_grad()
    def encode_prompt(self, prompt, negative_prompt=None):
        """(prompt_embeds, negative_prompt_embeds) as `StableDiffusionPipeline.encode_prompt` computes them for one image per
        prompt with classifier-free guidance (pipeline...:382-460): prompt padded to the tokenizer's model_max_length, the
        negative prompt ("" by default) padded to the same length, attention mask only if the text encoder asks for one."""
        if self.text_encoder is None or self.tokenizer is None:
            raise ValueError('pass prompt_embeds / negative_prompt_embeds, or build the pipeline with text_encoder= and tokenizer=')
        tok, te = self.tokenizer, self.text_encoder
        dev = self.device
        prompts = [prompt] if isinstance(prompt, str) else list(prompt)

        def run(texts, max_length):
            enc = tok(texts, padding='max_length', max_length=max_length, truncation=True, return_tensors='pt')
            mask = enc.attention_mask.to(dev) if getattr(getattr(te, 'config', None), 'use_attention_mask', False) else None
            return te(enc.input_ids.to(dev), attention_mask=mask)[0]
        pe = run(prompts, tok.model_max_length)
        neg = [''] * len(prompts) if negative_prompt is None else ([negative_prompt] * len(prompts) if isinstance(negative_prompt, str) else list(negative_prompt))
        if len(neg) != len(prompts):
            raise ValueError(f'negative_prompt has batch size {len(neg)}, prompt {len(prompts)}')
        ne = run(neg, pe.shape[1])
        dt = getattr(te, 'dtype', pe.dtype)
        return pe.to(dt), ne.to(dt)

    # ------------------------------------------------------------------------------------------
    def _gather(self, local_vals, n_total):
        """rewards of this rank's candidates [lo, hi) -> the rewards of all n_total candidates, identical on every rank (one all-gather)."""
        if self.shards.solo:
            return list(local_vals)
        t = torch.tensor(local_vals, dtype=torch.float64, device=self.device if self.shards.dev_direct else 'cpu')
        return self.shards.gather_rewards(t, n_total, 1).cpu().tolist()

    def _up(self, t, dtype):
        return t.to(self.device, dtype).contiguous()

    def _eps_rows(self, x, t, eu, ec, ctx_of, per, g):
        """CFG noise prediction for the rows of S searches, search-major: row r belongs to search r // per, whose context pair is
        ctx_of[r // per] of the D pairs in eu / ec.  One 2R-row U-Net call (the reference: R calls of 2 rows).  A U-Net that announces
        `takes_context_rows` (sd_unet.SDUNet) gets the 2D distinct contexts (negative, then positive) and an int32 row map built once per
        (rows, prompts) -- nothing for it to group and no host synchronisation in the call; every other U-Net the expanded tensor."""
        rows, d = x.shape[0], eu.shape[0]
        own = [ctx_of[r // per] for r in range(rows)]
        if getattr(self.unet, 'takes_context_rows', False):
            key = rows if d == 1 else (rows, per, tuple(ctx_of))             # one pair: the row count alone fixes the map
            cmap = self._context_rows.get(key)
            if cmap is None:
                cmap = self._context_rows[key] = torch.tensor(own + [d + c for c in own], dtype=torch.int32).to(self.device)
            out = self.unet(torch.cat([x, x]), t, encoder_hidden_states=torch.cat([eu, ec]), context_rows=cmap, return_dict=False)[0].contiguous()
        else:
            idx = torch.tensor(own, dtype=torch.int64, device=eu.device)
            out = self.unet(torch.cat([x, x]), t, encoder_hidden_states=torch.cat([eu[idx], ec[idx]]), return_dict=False)[0].contiguous()
        self.unet_rows += 2 * rows
        return ops.cfg_combine(out[:rows].contiguous(), out[rows:].contiguous(), g)

    def _score_images(self, score_function, u8, prompts):
        """rewards of quantised images [n,3,H,W], `prompts` one per image: a `batched` scorer (this package's CLIP / brightness scorers) gets
        ONE call -- `prompts=` the one shared prompt, or one entry per image when they differ -- every other scorer the reference's
        per-image calls (pipeline...:1114)."""
        n = u8.shape[0]
        shared = all(p == prompts[0] for p in prompts)
        if n > 1 and getattr(score_function, 'batched', False):
            s = score_function(images=[u8[j:j + 1] for j in range(n)], prompts=[prompts[0]] if shared else list(prompts), timesteps=None)
            self.scorer_calls += 1
            return [float(v) for v in (s.float().cpu().tolist() if torch.is_tensor(s) else s)]
        vals = []
        for j in range(n):
            s = score_function(images=[u8[j:j + 1]], prompts=[prompts[j]], timesteps=None)
            self.scorer_calls += 1
            vals.append(s.item() if torch.is_tensor(s) else float(s))
        return vals

    def _decode_rows(self, x, decode_rows):
        """the VAE decode of latents [R,...] in chunks of `decode_rows` rows (None: all at once)"""
        step = x.shape[0] if decode_rows is None else int(decode_rows)
        parts = [self.vae.decode(x[lo:lo + step].contiguous() / self.vae.config.scaling_factor, return_dict=False)[0] for lo in range(0, x.shape[0], step)]
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def _score_rows(self, score_function, x0, row_prompts, decode_rows):
        """decode + quantise + score the rows, `decode_rows` rows per decode and scorer call (None: all at once) -> the rows' rewards.
        Chunks change the launch forms, never the values' order or the draws."""
        rows = x0.shape[0]
        step = rows if decode_rows is None else int(decode_rows)
        vals = []
        for lo in range(0, rows, step):
            image = self._decode_rows(x0[lo:lo + step], None).float().contiguous()
            self.decoded += image.shape[0]
            vals += self._score_images(score_function, ops.quantize_u8(image, f32_math=True), row_prompts[lo:lo + step])
        return vals

    def _latent_shape(self, height, width):
        """[1,C,h,w] of `prepare_latents` (pipeline...:671-690)"""
        cfgu = self.unet.config
        vsf = 2 ** (len(getattr(self.vae.config, 'block_out_channels', [0] * 4)) - 1)
        return (1, cfgu.in_channels, (height // vsf) if height else cfgu.sample_size, (width // vsf) if width else cfgu.sample_size)

    def _output(self, x, image, output_type, **fields):
        """the call's result: `images` as `output_type` asks ('latent': x; 'pt': [R,3,H,W] in [0,1]; else PIL), the counters of this call"""
        if output_type == 'latent':
            images = x
        elif output_type == 'pt':
            images = (image / 2 + 0.5).clamp(0, 1)
        else:
            import PIL.Image
            arr = ((image / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float().cpu().numpy() * 255).round().astype('uint8')
            images = [PIL.Image.fromarray(a) for a in arr]
        return types.SimpleNamespace(images=images, nsfw_content_detected=None, latents=x, unet_rows=self.unet_rows, decoded=self.decoded,
                                     scorer_calls=self.scorer_calls, **fields)

    # ---- the search loop ------------------------------------------------------------------------
    def _search(self, streams, latents, prompt_embeds, negative_prompt_embeds, ctx_of, search_prompts, *, num_inference_steps, guidance_scale,
                eta, score_function, method, params, output_type, decode_rows):
        """The searches of S = len(streams) host streams in lock-step as ONE batch -> (output, [max_score] * S).

        Search k draws from streams[k] (sd_streams.SeedStream) in the reference's order and in the latents' dtype, so a search is the one
        it runs alone, whatever its companions.  Rows are search-major everywhere (naive 1 row per search, eps-greedy / zero-order N, beam
        B*N, rejection N); selection stays on the host per search (first maximum, stable sort).  The candidates of all searches come from ONE
        `dts_candidate_noise_sd_rows` launch and every DDIM candidate step from ONE `dts_ddim_candidates_groups` launch; the U-Net sees all
        rows in one call, the decoder and the scorer `decode_rows` rows at a time (None: all).  `method='rejection'` (the reference's
        main.py:134 loop: N naive trajectories on one stream) pre-draws a stream's N trajectories in that order and runs them as rows; best
        of N, ties to the first.

        Candidate sharding (one search only: the callers refuse more): the first DDIM candidate step runs for all rows on every rank
        (replicated inputs, 32 KB per candidate: this is what makes every candidate latent available everywhere), the U-Net second pass,
        decode and score only for this rank's span of the candidate rows, then ONE all-gather of the rewards per decision.

        latents [S,C,H,W] (None for rejection, which draws its own); prompt_embeds / negative_prompt_embeds D rows, ctx_of[k] search k's
        pair; search_prompts one prompt per search (for the scorer).
        output: images / latents [S,...], scores / max_scores per search, unet_rows / decoded / scorer_calls as totals."""
        S = len(streams)
        sch, dev = self.scheduler, self.device
        shape, dtype = streams[0].shape, streams[0].dtype
        eu, ec = self._up(negative_prompt_embeds, dtype), self._up(prompt_embeds, dtype)
        timesteps = sch.set_timesteps(num_inference_steps)
        nT = len(timesteps)
        g = float(guidance_scale)
        self.unet_rows = self.decoded = self.scorer_calls = 0
        coll0 = self.shards.collectives
        scores = [[] for _ in range(S)]
        stack = lambda parts: self._up(torch.cat(parts), dtype)               # host [1,...] / [n,...] pieces, search-major -> device rows

        def per_search(vals, per):
            return [vals[k * per:(k + 1) * per] for k in range(S)]

        def step_rows(x, e, z_rows, t):
            """the DDIM step of every row with its own noise: one launch, G = rows groups of one candidate"""
            a_t, a_p, sig = sch.coefficients(t, eta)
            prev, _ = ops.ddim_candidates_groups(x, e, z_rows.reshape(x.shape[0], 1, *x.shape[1:]), a_t, a_p, sig, want_x0=False)
            return prev.reshape(x.shape)

        def evaluate(x, e, cands, per, t):
            """cands [R*per,...] search-major over the R rows of (x, e) -> (candidate latents [R*per,...], rewards of all): steps 1083-1114"""
            a_t, a_p, sig = sch.coefficients(t, eta)
            prev, _ = ops.ddim_candidates_groups(x, e, cands.reshape(x.shape[0], per, *x.shape[1:]), a_t, a_p, sig, want_x0=False)
            lat_c = prev.reshape(x.shape[0] * per, *x.shape[1:])
            rows = lat_c.shape[0]
            rows_per_search = rows // S
            lo, hi = self.shards.span(rows)                                   # a world of one: all rows
            vals = []
            if hi > lo:
                mine = lat_c[lo:hi].contiguous()
                np2 = self._eps_rows(mine, t, eu, ec, ctx_of, rows_per_search, g)            # same t, not t-1 (:1090)
                _, x0 = ops.ddim_candidates_groups(mine, np2, None, a_t, a_p, sig, want_x0=True)
                vals = self._score_rows(score_function, x0, [search_prompts[r // rows_per_search] for r in range(lo, hi)], decode_rows)
            return lat_c, self._gather(vals, rows)

        max_scores = [None] * S
        per_final = 1
        if method == 'rejection':
            N = params['N']
            trajs = [st.rejection_trajectories(N, nT) for st in streams]       # [S][N] of (latents, [nT] noises), pre-drawn in stream order
            x = stack([lat * sch.init_noise_sigma for tr in trajs for lat, _ in tr])
            for i, t in enumerate(timesteps):
                e = self._eps_rows(x, t, eu, ec, ctx_of, N, g)
                x = step_rows(x, e, stack([zs[i] for tr in trajs for _, zs in tr]), t)
            per_final = N
        else:
            x = self._up(latents * sch.init_noise_sigma, dtype)
            if method == 'beam':
                B, N = params['B'], params['N']
                self.shards.require_candidates(B * N, 'SD beam search')
                x = x.repeat_interleave(B, dim=0)                              # [S*B,...]: every search starts with B copies (:1047)
                for i, t in enumerate(timesteps):
                    e = self._eps_rows(x, t, eu, ec, ctx_of, B, g)             # the beams' noise predictions in ONE call (the reference: one per beam)
                    cands = stack([st.beam_round(N) for st in streams for _ in range(B)])     # per search, per beam: the reference's order
                    lat_all, vals = evaluate(x, e, cands, N, t)                # [S*B*N,...], (search, beam, candidate)-major
                    keep = []
                    for k, v in enumerate(per_search(vals, B * N)):
                        scores[k] += v
                        order = sorted(range(B * N), key=lambda j: v[j], reverse=True)        # stable: first wins ties (:1132)
                        keep += [k * B * N + j for j in order[:B]]
                    x = lat_all[torch.tensor(keep, dtype=torch.int64, device=dev)].contiguous()      # survivors: already on every rank
                per_final = B
            else:
                local = method in ('eps_greedy', 'zero_order')
                if local:
                    N = params['N']
                    self.shards.require_candidates(N, 'SD eps-greedy / zero-order search')
                    thr = params['eps'] if method == 'eps_greedy' else 0.0
                for i, t in enumerate(timesteps):
                    e = self._eps_rows(x, t, eu, ec, ctx_of, 1, g)
                    pivot = stack([st.randn() for st in streams])              # :1366
                    for _ in range(params['K'] if local else 0):
                        # host RNG in the reference's call order (:1371-1379, SeedStream.local_round); the candidate ARITHMETIC (normalise,
                        # scale, add the pivot) runs on the device in the latents' dtype
                        rounds = [st.local_round(N, thr, params['lambda']) for st in streams]
                        mode = torch.tensor([m for _, ms, _ in rounds for m in ms], dtype=torch.int32, device=dev)
                        scale = torch.tensor([s_ for _, _, sc in rounds for s_ in sc], dtype=torch.float32, device=dev)
                        cands = ops.candidate_noise_sd_rows(pivot, stack([u.reshape(N, *shape[1:]) for u, _, _ in rounds]), mode, scale)
                        _, vals = evaluate(x, e, cands, N, t)
                        best = []
                        for k, v in enumerate(per_search(vals, N)):
                            scores[k] += v
                            max_scores[k] = max(v)
                            best.append(k * N + v.index(max_scores[k]))         # first max (:1432-1433)
                        pivot = cands[torch.tensor(best, dtype=torch.int64, device=dev)].contiguous()
                    x = step_rows(x, e, pivot, t)
        # beam: the beams' own latents are decoded and scored (:1157-1170; B images: replicated), the winner is decoded for the output;
        # naive / rejection: the final image is what is scored (:1457-1485, main.py:134-140).  Best per search, ties to the first
        final_prompts = [search_prompts[r // per_final] for r in range(x.shape[0])]
        image = None
        if method == 'beam':
            finals = self._score_rows(score_function, x, final_prompts, decode_rows)
        elif method in ('naive', 'rejection'):
            image = self._decode_rows(x, decode_rows)
            finals = self._score_images(score_function, ops.quantize_u8(image.float().contiguous(), f32_math=True), final_prompts)
        if method in ('beam', 'naive', 'rejection'):
            win = []
            for k, v in enumerate(per_search(finals, per_final)):
                scores[k] += v
                max_scores[k] = max(v)
                win.append(k * per_final + v.index(max_scores[k]))
            win = torch.tensor(win, dtype=torch.int64, device=dev)
            x = x[win].contiguous()
            image = None if image is None else image[win].contiguous()
        if image is None:
            image = self._decode_rows(x, decode_rows)
        out = self._output(x, image, output_type, scores=scores, max_scores=max_scores, collectives=self.shards.collectives - coll0)
        return out, max_scores

    def _call_rows(self, row_seeds, *, prompt, negative_prompt, latents, prompt_embeds, negative_prompt_embeds, method, height, width,
                   decode_rows, **loop_kw):
        """`pipe(..., row_seeds=[s0, s1, ...]) -> (output, [max_score] * S)`: the searches of S seeds through `_search`, search k on its own
        `torch.Generator().manual_seed(row_seeds[k])`, which draws what `main.py --backend sd --seed` draws from the global generator: the
        float32 latents [1,C,h,w] first (only when `latents` is None), then the loop's draws.

        latents [S,C,H,W] or None; prompt a string or a list of 1 or S strings; prompt_embeds / negative_prompt_embeds 1 or S rows.
        output: `_search`'s, and `searches` (one record per seed) / `row_seeds`."""
        seeds = [int(s) for s in row_seeds]
        S = len(seeds)
        if S < 1:
            raise ValueError('row_seeds: need at least one seed')
        if method == 'mcts':
            raise ValueError("row_seeds: method 'mcts' is not supported (with or without mcts_backprop: its trees are ragged per search)")
        if method not in LOCKSTEP_METHODS:
            raise ValueError(f'row_seeds: unknown method {method!r}')
        if not self.shards.solo:
            raise ValueError('row_seeds: candidate sharding over more than one rank is not supported (shards=CandidateShards(enabled=False): '
                             'lock-step batches go with seed sharding)')
        if decode_rows is not None and int(decode_rows) < 1:
            raise ValueError(f'decode_rows: a positive number of rows per VAE decode, got {decode_rows}')
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f'Cannot forward both `prompt`: {prompt} and `prompt_embeds`. Please make sure to only forward one of the two.')
        prompts = None
        if prompt is not None:
            prompts = [prompt] if isinstance(prompt, str) else list(prompt)
            if len(prompts) not in (1, S):
                raise ValueError(f'row_seeds: prompt: need 1 or {S} prompts (one per seed), got {len(prompts)}')
        if prompt_embeds is None or negative_prompt_embeds is None:
            if prompts is None:
                raise ValueError('pass `prompt` (with a text_encoder/tokenizer in the pipeline) or prompt_embeds + negative_prompt_embeds')
            shared_negative = negative_prompt is None or isinstance(negative_prompt, str)
            distinct = list(dict.fromkeys(prompts)) if shared_negative else prompts      # each distinct prompt is encoded once
            pe, ne = self.encode_prompt(distinct, negative_prompt)
            ctx_of = [distinct.index(p) if shared_negative else k for k, p in enumerate(prompts)] * (S // len(prompts))
            prompt_embeds = pe if prompt_embeds is None else prompt_embeds
            negative_prompt_embeds = ne if negative_prompt_embeds is None else negative_prompt_embeds
        else:
            ctx_of = None
        d = prompt_embeds.shape[0]
        if negative_prompt_embeds.shape[0] != d:
            raise ValueError(f'row_seeds: prompt_embeds has {d} rows, negative_prompt_embeds {negative_prompt_embeds.shape[0]}')
        if ctx_of is None or max(ctx_of) >= d:                                # embeddings given: one pair for all, or one per seed
            if d not in (1, S):
                raise ValueError(f'row_seeds: prompt_embeds: need 1 or {S} rows (one per seed), got {d}')
            ctx_of = [0] * S if d == 1 else list(range(S))
        search_prompts = [None] * S if prompts is None else prompts * (S // len(prompts))
        if latents is not None:
            if method == 'rejection':
                raise ValueError("row_seeds: method 'rejection' draws the latents of its N trajectories itself: pass latents=None")
            if latents.dim() != 4 or latents.shape[0] != S:
                raise ValueError(f'row_seeds: latents: need [{S}, C, H, W] (one row per seed), got {tuple(latents.shape)}')
            shape = (1,) + tuple(latents.shape[1:])
        else:
            shape = self._latent_shape(height, width)
        streams = [SeedStream(s, shape, getattr(self.unet, 'dtype', torch.float32)) for s in seeds]
        if latents is None and method != 'rejection':
            latents = torch.cat([st.latents() for st in streams])
        out, max_scores = self._search(streams, latents, prompt_embeds, negative_prompt_embeds, ctx_of, search_prompts, method=method,
                                       decode_rows=decode_rows, **loop_kw)
        out.row_seeds = seeds
        out.searches = [types.SimpleNamespace(seed=seeds[k], images=out.images[k:k + 1], latents=out.latents[k:k + 1], scores=out.scores[k],
                                              max_score=max_scores[k], prompt=search_prompts[k]) for k in range(S)]
        return out, max_scores

    # ---- MCTS: single-search code (ragged trees) ------------------------------------------------
    def _mcts_reference(self, timesteps, latents, params, eps, step, randn):
        """The reference's MCTS branch as it runs (pipeline...:1201-1313): never scores, so every timestep takes the FIRST expanded child;
        the rollouts only consume RNG (their U-Net work runs with `mcts_dead_compute` only).  -> (latents, None)"""
        for i, t in enumerate(timesteps):
            children = []
            for _ in range(params['S']):
                node = latents
                if len(children) < params['N']:
                    node = step(node, t)
                    children.append(node)
                tmp = node
                if self.mcts_dead_compute:
                    eps(node, t)
                for j in range(i, len(timesteps)):                            # rollout: consumes RNG, result never used
                    if self.mcts_dead_compute:
                        tmp = step(tmp, timesteps[j])
                    else:
                        randn()
            if children:
                latents = children[0]
        return latents, None

    def _mcts_backprop(self, timesteps, latents, params, step, score):
        """The tree search the reference's MCTS branch sets out to do but never completes (pipeline...:1201-1313 builds the nodes
        and runs the rollouts, then drops `pred_x0`: no decode, no score, `visits` / `total_reward` never updated, so `best_child`
        is always the first child).  Behind `mcts_backprop=True` only.  Differences from the reference code, all required for the
        statistics to mean anything: a node at depth d is expanded and rolled out from timestep index i+d (the reference uses
        the root's `t` and `range(i, ...)` for every node); the rollout's final latents are decoded and scored; the reward is
        added along the path to the root.  Host RNG order: per simulation, the expansion noise (if any), then one variance
        noise per rollout step.  -> (latents, best reward)"""
        S, N, c = params['S'], params['N'], params.get('c', 1.414)
        nT = len(timesteps)
        best_reward = None
        for i in range(nT):
            root = _MCTSNode(latents)
            root.visits = 1
            for _ in range(S):
                node = root
                while node.children and all(ch.visits > 0 for ch in node.children) and len(node.children) >= N:
                    node = max(node.children, key=lambda ch: ch.ucb(c))
                ti = i + node.depth
                if ti < nT and len(node.children) < N:                         # expansion
                    node = _MCTSNode(step(node.latents, timesteps[ti]), parent=node)
                    node.parent.children.append(node)
                tmp = node.latents
                for j in range(i + node.depth, nT):                            # stochastic DDIM rollout to the last timestep
                    tmp = step(tmp, timesteps[j])
                r = score(tmp)
                best_reward = r if best_reward is None else max(best_reward, r)
                while node is not None:                                        # back-propagation
                    node.visits += 1
                    node.total_reward += r
                    node = node.parent
            kids = [ch for ch in root.children if ch.visits > 0]
            if kids:
                latents = max(kids, key=lambda ch: ch.total_reward / ch.visits).latents
        return latents, best_reward

    def _call_mcts(self, latents, prompt_embeds, negative_prompt_embeds, prompt, *, num_inference_steps, guidance_scale, eta, score_function,
                   params, output_type):
        """method='mcts' of the single call (either variant) on torch's global generator -> (output, max_score)"""
        sch = self.scheduler
        dtype = getattr(self.unet, 'dtype', torch.float32)
        eu, ec = self._up(negative_prompt_embeds, dtype), self._up(prompt_embeds, dtype)
        timesteps = sch.set_timesteps(num_inference_steps)
        x = self._up(latents * sch.init_noise_sigma, dtype)
        g = float(guidance_scale)
        self.unet_rows = self.decoded = self.scorer_calls = 0
        coll0 = self.shards.collectives
        scores = []
        randn = SeedStream(None, tuple(x.shape), dtype).randn

        def eps(x, t):
            return self._eps_rows(x, t, eu, ec, [0], x.shape[0], g)

        def step(x, t):
            """one stochastic DDIM step: the noise prediction, then a fresh variance noise from the stream"""
            return sch.step(eps(x, t), t, x, eta, variance_noise=self._up(randn(), dtype))[0]

        def score(x):
            scores.extend(self._score_rows(score_function, x, [prompt], None))
            return scores[-1]
        if self.mcts_backprop:
            x, max_score = self._mcts_backprop(timesteps, x, params, step, score)
        else:
            x, max_score = self._mcts_reference(timesteps, x, params, eps, step, randn)
        image = self._decode_rows(x, None)
        if max_score is None:                                                 # the final image is what is scored (:1457-1485)
            s = score_function(images=[ops.quantize_u8(image.float().contiguous(), f32_math=True)], prompts=[prompt], timesteps=None)
            max_score = s.item() if torch.is_tensor(s) else float(s)
            scores.append(max_score)
        return self._output(x, image, output_type, scores=scores, collectives=self.shards.collectives - coll0), max_score

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, prompt=None, num_inference_steps=100, guidance_scale=7.5, negative_prompt=None, eta=1.0, latents=None,
                 prompt_embeds=None, negative_prompt_embeds=None, score_function: Optional[Callable] = None, method='eps_greedy',
                 params=None, output_type='pt', height=None, width=None, row_seeds=None, decode_rows=None):
        """Keyword surface of the reference call (pipeline...:785-817) for the arguments the search path uses:
        `pipe(prompt=..., num_inference_steps=..., score_function=..., method=..., params=...) -> (output, max_score)`: one search on
        torch's global CPU generator as it stands, its candidates sharded over the ranks of `shards`.
        row_seeds=[s0, s1, ...] (this build's keyword) runs the searches of those seeds in lock-step as one batch: see `_call_rows`."""
        loop_kw = dict(num_inference_steps=num_inference_steps, guidance_scale=guidance_scale, eta=eta, score_function=score_function,
                       params=params, output_type=output_type)
        if row_seeds is not None:
            return self._call_rows(row_seeds, prompt=prompt, negative_prompt=negative_prompt, latents=latents, prompt_embeds=prompt_embeds,
                                   negative_prompt_embeds=negative_prompt_embeds, method=method, height=height, width=width,
                                   decode_rows=decode_rows, **loop_kw)
        if decode_rows is not None:
            raise ValueError('decode_rows goes with row_seeds (the lock-step search loop)')
        if method == 'rejection':
            raise ValueError("method 'rejection': the single call runs one trajectory (main.py loops over N calls of 'naive'); "
                             'row_seeds=[...] runs the N trajectories of a seed as rows')
        if method != 'mcts' and method not in LOCKSTEP_METHODS:
            raise ValueError(f'unknown method {method!r}')
        if prompt is not None and prompt_embeds is not None:                  # check_inputs (:657-661)
            raise ValueError(f'Cannot forward both `prompt`: {prompt} and `prompt_embeds`. Please make sure to only forward one of the two.')
        if prompt_embeds is None or negative_prompt_embeds is None:
            if prompt is None:
                raise ValueError('pass `prompt` (with a text_encoder/tokenizer in the pipeline) or prompt_embeds + negative_prompt_embeds')
            pe, ne = self.encode_prompt(prompt, negative_prompt)
            prompt_embeds = pe if prompt_embeds is None else prompt_embeds
            negative_prompt_embeds = ne if negative_prompt_embeds is None else negative_prompt_embeds
        if isinstance(prompt, list):
            if len(prompt) != 1:
                raise ValueError('the search loop runs one prompt per call (as main.py:135 of the reference does)')
            prompt = prompt[0]
        # randn_like(latents) on the reference's CPU run draws in the LATENTS' dtype (fp16 latents -> fp16 normal sampler, a different
        # stream from f32 draws rounded to fp16); so does prepare_latents (:671-690), unlike main.py's float32 draw (SeedStream.latents)
        dtype = getattr(self.unet, 'dtype', torch.float32)
        if latents is None:
            latents = torch.randn(self._latent_shape(height, width), dtype=dtype)
        if method == 'mcts':
            return self._call_mcts(latents, prompt_embeds, negative_prompt_embeds, prompt, **loop_kw)
        out, max_scores = self._search([SeedStream(None, tuple(latents.shape), dtype)], latents, prompt_embeds, negative_prompt_embeds, [0],
                                       [prompt], method=method, decode_rows=None, **loop_kw)
        out.scores = out.scores[0]
        del out.max_scores
        return out, max_scores[0]
