#!/usr/bin/env python3
"""Golden vectors of the two plain samplers (edm/generate.py: edm_sampler, ablation_sampler) from THE REFERENCE ITSELF, imported on the CPU.

Run:  PYTHONHASHSEED=0 python tests/golden/make_golden_ablation.py      (needs the reference checkout; about a minute)

Writes tests/golden/ablation_golden.npz + ablation_manifest.json: arrays and scalars only.  No weights and nothing of the reference's text is
stored: the tiny networks are those of make_golden_preconds.TINY (VP, VE, iDDPM) and make_golden.TINY['ddpmpp_tiny'] (EDM), re-created by
diffusion_tts_amd.init and proven equal to the reference constructors there.

Inputs of every case: 3 rows from the reference's StackedRandomGenerator('cpu', [3, 4, 5]) -- latents first, then the label indices -- and
8 steps.  The step noise comes from the same per-row generators (randn_like).  Per case c:
  <c>_t_steps                       the reference's time steps (9 entries, the last one 0)
  <c>_t_hat, _sigma_hat             per step: the churned time and the noise level the denoiser is called with
  <c>_ratio, _noise_coef, _a, _b, _h   per step: the host scalars of x_hat = ratio x + noise_coef eps and d = a x - b D, formed here from the
                                    reference's OWN schedule functions (read out of the running sampler's frame) at its own t_cur / t_hat
  <c>_x, _image                     final state (float64) and its uint8 image [3, 16, 16, 3]
  <c>_x64                           the same run with the denoiser in float64 (make_golden_preconds.forward_f64's recipe)
  manifest[c].ref_f32_vs_f64        max|x - x64| / max|x64|;   manifest[c].net_rows: rows pushed through the denoiser
"""
import copy
import json
import os
import sys
import time

assert os.environ.get('PYTHONHASHSEED') == '0', 'run with PYTHONHASHSEED=0 (the import recipe of make_golden.py asks for it)'

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                       # noqa: E402  (the import recipe)
import make_golden_preconds as mp              # noqa: E402  (the tiny VP / VE / iDDPM networks, forward_f64)

import numpy as np                             # noqa: E402
import torch                                   # noqa: E402

import generate as ref_generate                # noqa: E402  edm/generate.py

from diffusion_tts_amd import init as dinit    # noqa: E402

torch.set_num_threads(4)
SEEDS = [3, 4, 5]
NUM_STEPS = 8
CHURN = dict(S_churn=4, S_min=0.05, S_max=50, S_noise=1.003)
# case -> (network, sampler, keyword arguments)
CASES = {
    'vp_euler': ('vp', 'ablation', dict(solver='euler', discretization='vp', schedule='vp', scaling='vp')),
    've_euler': ('ve', 'ablation', dict(solver='euler', discretization='ve', schedule='ve', scaling='none')),
    'iddpm_heun': ('iddpm', 'ablation', dict(solver='heun', discretization='iddpm', schedule='linear', scaling='none', alpha=0.75)),
    'vp_heun_churn': ('vp', 'ablation', dict(solver='heun', discretization='edm', schedule='vp', scaling='vp', **CHURN)),
    've_heun_vpdisc': ('ve', 'ablation', dict(solver='heun', discretization='vp', schedule='ve', scaling='none')),
    'edm_ablation_defaults': ('edm', 'ablation', dict(**CHURN)),
    'edm_sampler': ('edm', 'edm', dict(**CHURN)),
}


def edm_forward_f64(mod, x, sigma, labels):
    """EDMPrecond's forward with every step in float64: D = c_skip x + c_out F(c_in x; ln(sigma) / 4)"""
    m64 = copy.deepcopy(mod).double()
    s = sigma.to(torch.float64).reshape(-1, 1, 1, 1)
    sd = mod.sigma_data
    q = s ** 2 + sd ** 2
    F = m64.model(x / q.sqrt(), (s.log() / 4).flatten(), class_labels=None if labels is None else labels.to(torch.float64))
    assert F.dtype == torch.float64
    return sd ** 2 / q * x + s * sd / q.sqrt() * F


class Net:
    """What the samplers need of a network, around a reference module; records every call and, at the first call of a step, the host scalars
    of that step from the running sampler's frame.  f64: the denoiser in float64."""

    def __init__(self, mod, kind, f64=False):
        self.mod, self.kind, self.f64 = mod, kind, f64
        self.sigma_min, self.sigma_max = float(mod.sigma_min), float(mod.sigma_max)
        self.img_channels, self.img_resolution, self.label_dim = mod.img_channels, mod.img_resolution, mod.label_dim
        self.rows, self.steps, self.seen, self.extra = 0, [], set(), {}

    def round_sigma(self, sigma):
        return self.mod.round_sigma(sigma)

    def __call__(self, x, sigma, class_labels=None):
        loc = sys._getframe(1).f_locals
        if loc['i'] not in self.seen:
            self.seen.add(loc['i'])
            self.steps.append(step_scalars(loc))
            self.extra['t_steps'] = loc['t_steps'].clone()
            if 'u_filtered' in loc:
                self.extra['n_filtered'] = len(loc['u_filtered'])
        self.rows += x.shape[0]
        sigma = torch.as_tensor(sigma)
        if not self.f64:
            return self.mod(x, sigma, class_labels)
        if self.kind == 'edm':
            return edm_forward_f64(self.mod, x, sigma.expand(x.shape[0]), class_labels)
        return mp.forward_f64(self.mod, self.kind, x, sigma.expand(x.shape[0]), class_labels)


def step_scalars(loc):
    """the step's host scalars from the sampler's local variables"""
    t_cur, t_hat, t_next = loc['t_cur'], loc['t_hat'], loc['t_next']
    if 'sigma_deriv' not in loc:                                   # edm_sampler: sigma(t) = t, s = 1
        return dict(t_hat=t_hat, sigma_hat=t_hat, ratio=1.0, noise_coef=(t_hat ** 2 - t_cur ** 2).sqrt() * loc['S_noise'], a=1 / t_hat, b=1 / t_hat,
                    h=t_next - t_hat)
    sig, dsig, s, ds = loc['sigma'], loc['sigma_deriv'], loc['s'], loc['s_deriv']
    coef = (sig(t_hat) ** 2 - sig(t_cur) ** 2).clip(min=0).sqrt() * s(t_hat) * loc['S_noise']
    return dict(t_hat=t_hat, sigma_hat=sig(t_hat), ratio=s(t_hat) / s(t_cur), noise_coef=coef,
                a=dsig(t_hat) / sig(t_hat) + ds(t_hat) / s(t_hat), b=dsig(t_hat) * s(t_hat) / sig(t_hat), h=t_next - t_hat)


def networks():
    nets = {}
    for kind, cfg in mp.TINY.items():
        nets[kind], _, _ = mp.ref_full(cfg, mg.NET_SEED)
    cfg = mg.TINY['ddpmpp_tiny']
    mod = mg.ref_edm(cfg, mg.NET_SEED)
    sd = dinit.edm_state_dict(cfg, mg.NET_SEED)
    mg.assert_same_params(mod, sd, 'ddpmpp_tiny')
    mg.load_refilled(mod, dinit.refill_degenerate(sd, mg.NET_SEED)[0])
    nets['edm'] = mod
    return nets


def run(mod, kind, sampler, kw, f64):
    net = Net(mod, kind, f64)
    rnd = ref_generate.StackedRandomGenerator('cpu', SEEDS)
    latents = rnd.randn([len(SEEDS), net.img_channels, net.img_resolution, net.img_resolution])
    idx = rnd.randint(net.label_dim, size=[len(SEEDS)])
    fn = ref_generate.ablation_sampler if sampler == 'ablation' else ref_generate.edm_sampler
    with torch.no_grad():
        x = fn(net, latents, torch.eye(net.label_dim)[idx], randn_like=rnd.randn_like, num_steps=NUM_STEPS, **kw)
    assert x.dtype == torch.float64
    return net, latents, idx, x


def main():
    t00 = time.time()
    out, man = {}, dict(torch=torch.__version__, numpy=np.__version__, seeds=SEEDS, num_steps=NUM_STEPS, net_seed=mg.NET_SEED,
                        edm_net='ddpmpp_tiny', cases={})
    nets = networks()
    for case, (kind, sampler, kw) in CASES.items():
        net, latents, idx, x = run(nets[kind], kind, sampler, kw, f64=False)
        net64, lat64, idx64, x64 = run(nets[kind], kind, sampler, kw, f64=True)
        assert torch.equal(latents, lat64) and torch.equal(idx, idx64) and net.rows == net64.rows
        if 'latents' in out:
            assert np.array_equal(out['latents'], latents.numpy()) and np.array_equal(out['label_idx'], idx.numpy())
        out['latents'], out['label_idx'] = latents.numpy(), idx.numpy()
        heun = sampler == 'edm' or kw.get('solver', 'heun') == 'heun'
        assert net.rows == len(SEEDS) * (2 * NUM_STEPS - 1 if heun else NUM_STEPS) and len(net.steps) == NUM_STEPS
        for key in ('t_hat', 'sigma_hat', 'ratio', 'noise_coef', 'a', 'b', 'h'):
            out[f'{case}_{key}'] = np.array([float(st[key]) for st in net.steps], dtype=np.float64)
            assert np.array_equal(out[f'{case}_{key}'], np.array([float(st[key]) for st in net64.steps])), (case, key)
        t_steps = net.extra['t_steps']
        assert t_steps.dtype == torch.float64 and t_steps.numel() == NUM_STEPS + 1 and float(t_steps[-1]) == 0.0
        out[f'{case}_t_steps'] = t_steps.numpy()
        if kw.get('discretization') == 'iddpm':
            # the index of the table entry a step takes is a rounded product: keep every product away from a half-integer, where another
            # host's last bit could round it the other way
            pos = (net.extra['n_filtered'] - 1) / (NUM_STEPS - 1) * np.arange(NUM_STEPS)
            assert np.all(np.abs(pos - np.floor(pos) - 0.5) > 1e-6), pos
            man['iddpm_index_positions'] = pos.tolist()
        rel = float((x - x64).abs().max() / x64.abs().max())
        out[f'{case}_x'], out[f'{case}_x64'] = x.numpy(), x64.numpy()
        out[f'{case}_image'] = (x * 127.5 + 128).clip(0, 255).to(torch.uint8).permute(0, 2, 3, 1).numpy()
        man['cases'][case] = dict(net=kind, sampler=sampler, kwargs=kw, net_rows=net.rows, ref_f32_vs_f64=rel, max_abs_x=float(x64.abs().max()),
                                  sigma_min=net.sigma_min, sigma_max=net.sigma_max)
        print(f'[{time.time() - t00:6.1f}s] {case}: rows {net.rows}, max|x| {float(x64.abs().max()):.1f}, ref_f32_vs_f64 {rel:.3e}, '
              f'noise steps {int((out[case + "_noise_coef"] != 0).sum())}', flush=True)
    np.savez_compressed(os.path.join(HERE, 'ablation_golden.npz'), **out)
    with open(os.path.join(HERE, 'ablation_manifest.json'), 'w') as f:
        json.dump(man, f, indent=1)
    print(f'[{time.time() - t00:6.1f}s] wrote ablation_golden.npz ({os.path.getsize(os.path.join(HERE, "ablation_golden.npz"))} bytes)')


if __name__ == '__main__':
    main()
