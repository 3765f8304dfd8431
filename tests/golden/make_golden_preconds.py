#!/usr/bin/env python3
"""Golden vectors of the VP, VE and iDDPM preconditioners (VPPrecond, VEPrecond, iDDPMPrecond: edm/training/networks.py:469-625) from THE
REFERENCE ITSELF, imported on the CPU.

Run:  PYTHONHASHSEED=0 python tests/golden/make_golden_preconds.py      (needs the reference checkout; about a minute)

Writes tests/golden/preconds_golden.npz + preconds_manifest.json: arrays, scalars, key lists and checksums only.  No weights and nothing of
the reference's text is stored: the weights are re-created by diffusion_tts_amd.init, which this script proves equal to the reference
constructors -- parameters AND buffers (iDDPM's `u` table, the 6-channel out_conv draw, NCSN++'s freqs and filters) -- under the documented
weight rule; so are sigma_min / sigma_max of the VP and iDDPM constructors and the three full-size presets of config.py.

Per preconditioner p in (vp, ve, iddpm), on a tiny network (16x16, two levels, one attention block, 10 classes -- the reference's REJECTION
search needs class labels, edm/main.py:108; vp: DDPM++, ve: NCSN++, iddpm: ADM with 6 output channels):
  <p>_x, _sigma, _label_idx, _D    a 2-row forward of the reference (x fp64 -> D fp32), per-row sigma (one large, one small)
  <p>_D64                          the same forward with the module in float64 and the wrapper's formula by hand in float64 (iDDPM: all six
                                   output channels computed, the first three read, as networks.py:614)
  manifest[p].ref_f32_vs_f64       max|D - D64| / max(1, max|D64|)
  <p>_sweep_sigma, _sweep_c_noise  c_noise of the reference's own expression on 64 log-spaced float32 sigmas across [sigma_min, sigma_max]
  iddpm_u                          the table; iddpm_sweep_decided: which sweep sigmas have their two nearest entries >= 5 % apart in distance
  iddpm_round_sigma, _round_index  round_sigma(return_index=True) on log-uniform sigmas with that 5 % margin; the script asserts that the
                                   reference agrees with the exact nearest entry on every one, and that it maps every table entry to itself
  <p>_naive_*, <p>_rej_*           NAIVE (18 steps) and REJECTION N = 4 with the brightness scorer through the reference's generate_image_grid,
                                   sigma_min / sigma_max clamped to the network's range as edm/generate.py:31-32 does
"""
import copy
import json
import os
import sys
import tempfile
import time

assert os.environ.get('PYTHONHASHSEED') == '0', 'run with PYTHONHASHSEED=0 (edm/main.py:776 hashes strings)'

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                       # the import recipe, the loggers, the weight checks  # noqa: E402

import numpy as np                             # noqa: E402
import PIL.Image                               # noqa: E402
import torch                                   # noqa: E402

from diffusion_tts_amd import init as dinit    # noqa: E402
from diffusion_tts_amd import config as dconfig  # noqa: E402
from diffusion_tts_amd.config import EDMConfig  # noqa: E402

torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
KW = dict(num_steps=18, seed=0)
S = dict(S_churn=40, S_min=0.05, S_max=50, S_noise=1.003)
MARGIN = 4e-5                                  # make_golden.py: the top-2 reward gap a decision needs to be reproducible in fp32
NCSNPP = dict(embedding_type='fourier', channel_mult_noise=2, encoder_type='residual', resample_filter=[1, 3, 3, 1])
VP_RANGE = dinit.vp_sigma_range()
U = dinit.iddpm_u()
TINY = {
    'vp': EDMConfig('ddpmpp', 16, 3, 10, 64, [1, 2], 4, 1, [8], 9, precond='vp', sigma_min=VP_RANGE[0], sigma_max=VP_RANGE[1]),
    've': EDMConfig('ddpmpp', 16, 3, 10, 64, [1, 2], 4, 1, [8], 9, precond='ve', sigma_min=0.02, sigma_max=100, **NCSNPP),
    'iddpm': EDMConfig('adm', 16, 3, 10, 64, [1, 2], 4, 1, [8], 0, precond='iddpm', sigma_min=float(U[999]), sigma_max=float(U[0])),
}
# per preconditioner: (generator seed, per-row sigma, label indices)
FWD = {'vp': (6161, [40.0, 0.05], [3, 7]), 've': (6262, [0.03, 60.0], [0, 9]), 'iddpm': (6363, [25.0, 0.08], [1, 8])}
CLASSES = {'vp': 'VPPrecond', 've': 'VEPrecond', 'iddpm': 'iDDPMPrecond'}


def ref_net(cfg, seed):
    """the reference wrapper of cfg.precond with its own default scalars over the denoiser cfg describes"""
    torch.manual_seed(seed)
    kw = dict(model_channels=cfg.model_channels, channel_mult=cfg.channel_mult, num_blocks=cfg.num_blocks,
              attn_resolutions=cfg.attn_resolutions, augment_dim=cfg.augment_dim)
    if cfg.arch == 'adm':
        kw.update(model_type='DhariwalUNet')
    else:
        kw.update(model_type='SongUNet', embedding_type=cfg.embedding_type, encoder_type=cfg.encoder_type, decoder_type='standard',
                  channel_mult_noise=cfg.channel_mult_noise, resample_filter=cfg.resample_filter, dropout=0.13)
    cls = getattr(mg.ref_networks, CLASSES[cfg.precond])
    return cls(img_resolution=cfg.img_resolution, img_channels=cfg.img_channels, label_dim=cfg.label_dim, **kw).eval()


def ref_full(cfg, seed):
    """the reference module carrying the product initialiser's weights (checked equal to its own constructor's) + the weight rule"""
    mod = ref_net(cfg, seed)
    sd = dinit.edm_state_dict(cfg, seed)
    ref_sd = mod.state_dict()
    params = [k for k, _ in mod.named_parameters()]
    # key for key, in state_dict() order, buffers included (iDDPM's `u`, NCSN++'s freqs and filters); the [1, 1] box-filter buffers of the
    # ADM and DDPM++ resampling layers are the one thing the initialiser's dict has never carried (init.edm_state_dict)
    ref_keys = [k for k in ref_sd if cfg.fir or not k.endswith('.resample_filter')]
    assert ref_keys == list(sd.keys()), ([k for k in ref_keys if k not in sd][:5], [k for k in sd if k not in ref_sd][:5])
    for k in ref_keys:
        assert ref_sd[k].shape == sd[k].shape and torch.equal(ref_sd[k], sd[k]), k
    mg.assert_same_params(mod, {k: sd[k] for k in sd if k in params}, cfg.precond)
    assert float(mod.sigma_min) == cfg.sigma_min and float(mod.sigma_max) == cfg.sigma_max, (mod.sigma_min, mod.sigma_max, cfg)
    for k in ('beta_d', 'beta_min', 'M', 'epsilon_t', 'C_1', 'C_2'):     # the config's defaults are the constructors'
        assert not hasattr(mod, k) or getattr(mod, k) == getattr(cfg, k), k
    ck_ref = dinit.checksum({k: ref_sd[k] for k in sd})                   # (before the load below rewrites these tensors in place)
    sd2, refilled = dinit.refill_degenerate(sd, seed)
    if list(ref_sd.keys()) == list(sd.keys()):
        mod.load_state_dict(sd2, strict=True)
    else:
        mg.load_refilled(mod, sd2)
    rec = dict(keys=list(sd.keys()), buffers=[k for k in sd if k not in params], checksum=dinit.checksum(sd2),
               checksum_raw=dinit.checksum(sd), checksum_reference_raw=ck_ref, refilled=len(refilled),
               params=sum(v.numel() for v in sd.values()), sigma_min=cfg.sigma_min, sigma_max=cfg.sigma_max)
    return mod, sd2, rec


def exact_nearest(sig32, u):
    """index of the entry of u nearest to each float32 sigma, first index on a tie, and the ratio of the two smallest distances; float64
    differences of float32 values within 29 binades of each other are exact"""
    d = (torch.as_tensor(sig32, dtype=torch.float32).double().reshape(-1, 1) - u.double().reshape(1, -1)).abs()
    two = d.topk(2, dim=1, largest=False).values
    return d.argmin(1), two[:, 0] / two[:, 1]


def c_noise_ref(mod, kind, sig32):
    """the reference's own c_noise expression on a float32 column of sigmas (networks.py:504, 557, 610)"""
    s = sig32.to(torch.float32).reshape(-1, 1, 1, 1)
    if kind == 'vp':
        return ((mod.M - 1) * mod.sigma_inv(s)).flatten()
    if kind == 've':
        return (0.5 * s).log().flatten()
    return (mod.M - 1 - mod.round_sigma(s, return_index=True).to(torch.float32)).flatten()


def forward_f64(mod, kind, x, sigma, labels):
    """the wrapper's forward (networks.py:495-509 / 548-562 / 601-615) with every step in float64"""
    m64 = copy.deepcopy(mod).double()
    s = sigma.to(torch.float64).reshape(-1, 1, 1, 1)
    if kind == 'vp':
        c_out, c_in = -s, 1 / (s ** 2 + 1).sqrt()
        c_noise = (mod.M - 1) * ((mod.beta_min ** 2 + 2 * mod.beta_d * (1 + s ** 2).log()).sqrt() - mod.beta_min) / mod.beta_d
    elif kind == 've':
        c_out, c_in, c_noise = s, 1, (0.5 * s).log()
    else:
        c_out, c_in = -s, 1 / (s ** 2 + 1).sqrt()
        idx, ratio = exact_nearest(sigma.to(torch.float32), mod.u)
        assert float(ratio.max()) < 0.95, 'pick forward sigmas away from the midpoints of the table'
        assert torch.equal(idx, mod.round_sigma(sigma.to(torch.float32), return_index=True).flatten())
        c_noise = (mod.M - 1 - idx.double()).reshape(-1, 1, 1, 1)
    lab = None if labels is None else labels.to(torch.float64)
    F = m64.model(c_in * x, c_noise.flatten(), class_labels=lab)
    assert F.dtype == torch.float64 and F.shape[1] == mod.img_channels * (2 if kind == 'iddpm' else 1)
    return x + c_out * F[:, :mod.img_channels]


def run_ref_search(net, scorer, latents, labels, method, params, num_steps, seed, sigma_min, sigma_max):
    """make_golden.run_ref_search with the schedule's end points passed on (edm/main.py:50)"""
    logger, slog = mg.NetLogger(net), mg.ScoreLogger(scorer)

    class _HandOver:                      # replaces `pickle.load(f)['ema']`
        @staticmethod
        def load(f):
            return {'ema': logger}

    saved = mg.ref_main.pickle
    mg.ref_main.pickle = _HandOver
    np.random.seed(0)
    with tempfile.TemporaryDirectory() as td:
        png = os.path.join(td, 'out.png')
        try:
            mg.ref_main.generate_image_grid(
                os.path.abspath(__file__), png, latents, labels, seed=seed, gridw=latents.shape[0], gridh=1, device=torch.device('cpu'),
                num_steps=num_steps, sigma_min=sigma_min, sigma_max=sigma_max, sampling_method=getattr(mg.ref_main.SamplingMethod, method),
                sampling_params=dict(scorer=slog, **params), **S)
            img = np.array(PIL.Image.open(png))
        finally:
            mg.ref_main.pickle = saved
    return logger, slog, img


def main():
    t00 = time.time()
    out, man = {}, dict(torch=torch.__version__, numpy=np.__version__, threads=torch.get_num_threads(), net_seed=mg.NET_SEED, S=S, **KW)
    # ---- the full-size presets: initialiser == constructor (keys, parameters, buffers), ranges == the constructors'
    for name in ('vp_cifar10', 've_cifar10', 'iddpm_imagenet64'):
        cfg = getattr(dconfig, name)()
        _, _, rec = ref_full(cfg, mg.NET_SEED)
        man[name] = dict(checksum=rec['checksum'], checksum_raw=rec['checksum_raw'], params=rec['params'], sigma_min=cfg.sigma_min,
                         sigma_max=cfg.sigma_max, n_keys=len(rec['keys']), buffers=len(rec['buffers']))
        print(f'[{time.time() - t00:6.1f}s] preset {name}: {rec["params"]} values, range {cfg.sigma_min:.6g} .. {cfg.sigma_max:.6g}', flush=True)
    bright = mg.ref_scorers.BrightnessScorer()
    for kind, cfg in TINY.items():
        mod, sd2, rec = ref_full(cfg, mg.NET_SEED)
        gseed, sig, lab_idx = FWD[kind]
        g = torch.Generator().manual_seed(gseed)
        sigma = torch.tensor(sig, dtype=torch.float64)
        r = cfg.img_resolution
        x = torch.randn(2, 3, r, r, generator=g, dtype=torch.float64) * (sigma ** 2 + 0.25).sqrt().reshape(-1, 1, 1, 1)
        labels = None if lab_idx is None else torch.eye(cfg.label_dim)[torch.tensor(lab_idx)]
        with torch.no_grad():
            D = mod(x, sigma, labels)
            D64 = forward_f64(mod, kind, x, sigma, labels)
        assert D.dtype == torch.float32 and D.shape == x.shape
        rec['ref_f32_vs_f64'] = float((D.double() - D64).abs().max() / max(1.0, float(D64.abs().max())))
        rec['cfg'] = dict(cfg.__dict__)
        out.update({f'{kind}_x': x.numpy(), f'{kind}_sigma': sigma.numpy(), f'{kind}_D': D.numpy(), f'{kind}_D64': D64.numpy(),
                    f'{kind}_label_idx': np.array([] if lab_idx is None else lab_idx, dtype=np.int64)})
        # ---- c_noise over the network's range
        sw = torch.logspace(np.log10(cfg.sigma_min), np.log10(cfg.sigma_max), 64, dtype=torch.float64).to(torch.float32)
        with torch.no_grad():
            cn = c_noise_ref(mod, kind, sw)
        assert cn.dtype == torch.float32 and bool(torch.isfinite(cn).all())
        out[f'{kind}_sweep_sigma'], out[f'{kind}_sweep_c_noise'] = sw.numpy(), cn.numpy()
        if kind == 'iddpm':
            u = mod.u
            assert torch.equal(u, U)
            out['iddpm_u'] = u.numpy()
            idx, ratio = exact_nearest(sw, u)
            out['iddpm_sweep_decided'] = (ratio <= 0.95).numpy()
            assert torch.equal((mod.M - 1 - cn).long()[ratio <= 0.95], idx[ratio <= 0.95])
            # every table entry rounds to itself
            assert torch.equal(mod.round_sigma(u, return_index=True), torch.arange(u.numel()))
            gg = torch.Generator().manual_seed(6464)
            cand = torch.exp(torch.rand(4096, generator=gg, dtype=torch.float64) * np.log(200 / 1e-3) + np.log(1e-3)).to(torch.float32)
            idx, ratio = exact_nearest(cand, u)
            keep = ratio <= 0.95
            ref_idx = mod.round_sigma(cand, return_index=True)
            assert torch.equal(ref_idx[keep], idx[keep]), 'the reference misses the nearest entry at a 5 % margin'
            out['iddpm_round_sigma'], out['iddpm_round_index'] = cand[keep].numpy(), idx[keep].to(torch.int16).numpy()
            rec['round_sigma'] = dict(drawn=4096, kept=int(keep.sum()), reference_disagrees_without_margin=int((ref_idx != idx).sum()))
        # ---- the two searches, schedule clamped to the network's range
        smin, smax = max(0.002, float(mod.sigma_min)), min(80, float(mod.sigma_max))
        lab1 = None if not cfg.label_dim else torch.eye(cfg.label_dim)[torch.tensor([4])]
        lat = torch.randn(1, 3, r, r, generator=torch.Generator().manual_seed(11))
        with torch.no_grad():
            lg, sl, png = run_ref_search(mod, bright, lat, lab1, 'NAIVE', {}, KW['num_steps'], KW['seed'], smin, smax)
        rows = int(sum(c[0].shape[0] for c in lg.calls))
        assert rows == 35 and len(sl.calls) == 1
        out.update({f'{kind}_naive_latents': lat.numpy(), f'{kind}_naive_x_final': lg.calls[-1][2].double().numpy(), f'{kind}_naive_image': png,
                    f'{kind}_naive_final_score': sl.calls[-1][1].numpy(), f'{kind}_naive_sigmas': np.array([float(c[1][0]) for c in lg.calls])})
        rec['naive'] = dict(label=4 if cfg.label_dim else None, latent_seed=11, net_rows=rows, sigma_min=smin, sigma_max=smax)
        lat = torch.randn(1, 3, r, r, generator=torch.Generator().manual_seed(12))
        for seed in range(64):                                            # the first search seed whose decision has a reproducible margin
            with torch.no_grad():
                lg, sl, png = run_ref_search(mod, bright, lat, lab1, 'REJECTION_SAMPLING', dict(N=4), KW['num_steps'], seed, smin, smax)
            rew = sl.calls[0][1].numpy()
            srt = np.sort(rew)[::-1]
            if srt[0] - srt[1] >= MARGIN:
                break
        else:
            raise RuntimeError(f'{kind}: no seed with a safe decision margin')
        rows = int(sum(c[0].shape[0] for c in lg.calls))
        assert rows == 4 * 35 and len(sl.calls) == 2 and rew.shape[0] == 4
        last = lg.calls[-1][2].double()
        q = (last * 127.5 + 128).clip(0, 255).to(torch.uint8).permute(0, 2, 3, 1).numpy()
        kept = [j for j in range(4) if np.array_equal(q[j], png)]         # the trajectory the reference kept, read off its final image
        assert len(kept) >= 1 and kept[0] == int(rew.argmax())
        out.update({f'{kind}_rej_latents': lat.numpy(), f'{kind}_rej_rewards': rew, f'{kind}_rej_kept': np.array(kept[:1], dtype=np.int64),
                    f'{kind}_rej_x_final': last[kept[0]:kept[0] + 1].numpy(), f'{kind}_rej_image': png,
                    f'{kind}_rej_final_score': sl.calls[-1][1].numpy()})
        rec['rejection'] = dict(label=4 if cfg.label_dim else None, latent_seed=12, seed=seed, params=dict(N=4), net_rows=rows, kept=int(kept[0]),
                                top2_gap=float(srt[0] - srt[1]), sigma_min=smin, sigma_max=smax)
        man[kind] = rec
        print(f'[{time.time() - t00:6.1f}s] {kind}: {len(rec["keys"])} keys, max|D| {float(D.abs().max()):.3f}, ref_f32_vs_f64 '
              f'{rec["ref_f32_vs_f64"]:.3e}; rejection seed {seed} kept {kept[0]} (top-2 gap {srt[0] - srt[1]:.3e})', flush=True)
    np.savez_compressed(os.path.join(HERE, 'preconds_golden.npz'), **out)
    with open(os.path.join(HERE, 'preconds_manifest.json'), 'w') as f:
        json.dump(man, f, indent=1)
    print(f'[{time.time() - t00:6.1f}s] wrote preconds_golden.npz ({os.path.getsize(os.path.join(HERE, "preconds_golden.npz"))} bytes)')


if __name__ == '__main__':
    main()
