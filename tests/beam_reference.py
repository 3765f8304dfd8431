"""CPU restatement of the EDM beam search that `generate_image_grid(..., beam_search=True)` runs, over the oracle's networks
(oracle/): B beams per image (the reference's k) x N candidates per beam (its b).

It is the reference's branch, edm/main.py:138-404, with the survivor gather fixed: the reference reads every survivor from beam row
`sample_idx` (:375-379, `sample_beam_indices[beam_idx] // k == sample_idx`), whichever beam the top-k index points to; here survivor q of
image s is candidate `sel % N` of beam row `s * B + sel // N`.  With k = 1 the two are the same search, and
tests/test_beam_reference.py holds this file to the reference's own runs (tests/golden/make_golden_beam.py).

  beams       image-major rows s*B + j; at the start every image's x = latents * sigma_0 appears B times (:155)
  draws       per sigma step, per beam row in row order, ONE torch.randn([N, C, H, W], float64) from the global CPU generator (:257);
              made at gamma = 0 steps too; precomputed_noise[i] of shape [S, B, N, C, H, W] replaces the draws of step i
  step        the full step with churn and Heun for every candidate (`step`: the branch's own step_with_microbatch, :161-212, the
              arithmetic of :82-96 without the micro-batches); labels are the beam's image row
  reward      scorer(to_uint8(denoised), labels, zeros) on the step's returned `denoised` (:319-336).  step_with_microbatch returns
              the FIRST denoiser output, D(x_hat, t_hat) (:183, :212) -- its Heun stage keeps its own `denoised_2` (:204) -- unlike
              step() of :82-96, whose `denoised` is overwritten by the second-order output (:92).  The reference's own k = 1 runs pin
              this: with the second-order output every reward but the last step's differs at the 1e-3 level
  selection   per image the top B of its B*N float32 rewards, best first, exact ties to the lower flat index j*N + n (`select`)
  survivors   the candidates' x_next rows, in rank order
  result      beam 0 of every image (:404)
"""
import torch

from oracle import sampler as osamp


def select(rewards, B):
    """[S, B*N] rewards -> [S, B] flat indices: a stable descending sort of the float32 values (torch.topk leaves tie order unspecified)."""
    r = rewards.to(torch.float32)
    return torch.tensor([sorted(range(r.shape[1]), key=row.__getitem__, reverse=True)[:B] for row in r.tolist()], dtype=torch.int64).reshape(r.shape[0], B)


def gammas(t_steps, num_steps, S_churn, S_min, S_max):
    """gamma of every sigma step (edm/main.py:83)"""
    return [min(S_churn / num_steps, 2 ** 0.5 - 1) if S_min <= float(t) <= S_max else 0.0 for t in t_steps[:-1]]


def step(net, x_cur, t_cur, t_next, i, eps_i, labels, num_steps, S_churn, S_min, S_max, S_noise):
    """edm/main.py:161-212 over the whole batch: returns (x_next, the first-order denoised)"""
    gamma = min(S_churn / num_steps, 2 ** 0.5 - 1) if S_min <= t_cur <= S_max else 0
    t_hat = net.round_sigma(t_cur + gamma * t_cur)
    x_hat = x_cur + (t_hat ** 2 - t_cur ** 2).sqrt() * S_noise * eps_i
    denoised = net(x_hat, t_hat, labels).to(torch.float64)
    d_cur = (x_hat - denoised) / t_hat
    x_next = x_hat + (t_next - t_hat) * d_cur
    if i < num_steps - 1:
        denoised_2 = net(x_next, t_next, labels).to(torch.float64)
        d_prime = (x_next - denoised_2) / t_next
        x_next = x_hat + (t_next - t_hat) * (0.5 * d_cur + 0.5 * d_prime)
    return x_next, denoised


@torch.no_grad()
def beam_search(net, latents, labels, *, B, N, scorer, seed=0, num_steps=18, sigma_min=0.002, sigma_max=80, rho=7,
                S_churn=0, S_min=0, S_max=float('inf'), S_noise=1, precomputed_noise=None, stop_after=None):
    """Returns dict(x, image, final_scores, t_steps, rewards [S, B*N] per step, selected [S, B] per step, beam_parents).
    stop_after: return after that many sigma steps (x = the beams then, [S, B, ...])."""
    torch.manual_seed(seed)
    t_steps = osamp.sigma_schedule(net, num_steps, sigma_min, sigma_max, rho)
    S, shape1 = latents.shape[0], tuple(latents.shape[1:])
    x = (latents.to(torch.float64) * t_steps[0]).repeat_interleave(B, dim=0)
    lab = None if labels is None else labels.repeat_interleave(B * N, dim=0)
    rewards, selected, parents = [], [], []
    for i in range(num_steps):
        if precomputed_noise is not None and i in precomputed_noise:
            eps = precomputed_noise[i].to(torch.float64).reshape(S * B * N, *shape1)
        else:
            eps = torch.cat([torch.randn((N,) + shape1, dtype=torch.float64) for _ in range(S * B)])
        x_cand, x0 = step(net, x.repeat_interleave(N, dim=0), t_steps[i], t_steps[i + 1], i, eps, lab, num_steps, S_churn, S_min, S_max, S_noise)
        r = scorer(osamp.to_uint8(x0), lab, torch.zeros(x0.shape[0])).to(torch.float32).reshape(S, B * N)
        sel = select(r, B)
        rewards.append(r.clone())
        selected.append(sel)
        parents.append(sel // N)
        x = torch.stack([x_cand.view(S, B * N, *shape1)[s, f] for s in range(S) for f in sel[s].tolist()])
        if stop_after is not None and i + 1 == stop_after:
            return dict(x=x.view(S, B, *shape1), t_steps=t_steps, rewards=rewards, selected=selected, beam_parents=parents)
    x = x.view(S, B, *shape1)[:, 0]
    image = osamp.to_uint8(x)
    final = scorer(image.clone(), labels, torch.zeros(S))
    return dict(x=x, image=image, final_scores=final, t_steps=t_steps, rewards=rewards, selected=selected, beam_parents=parents)
