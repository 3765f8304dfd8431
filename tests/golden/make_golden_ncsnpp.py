#!/usr/bin/env python3
"""Golden vectors of the NCSN++ denoisers (SongUNet with embedding_type='fourier', channel_mult_noise=2, encoder_type='residual',
resample_filter=[1,3,3,1]: the network of the published `*-ve.pkl` EDM checkpoints) from THE REFERENCE ITSELF, imported on the CPU.

Run:  PYTHONHASHSEED=0 python tests/golden/make_golden_ncsnpp.py      (needs the reference checkout; a few minutes on 8 cores)

Writes tests/golden/ncsnpp_golden.npz + ncsnpp_manifest.json: arrays, scalars, key lists and checksums only.  No weights and nothing of the
reference's text is stored: the weights are re-created by diffusion_tts_amd.init, which this script proves equal to the reference
constructor -- parameters AND buffers (`map_noise.freqs`, the `resample_filter`s) -- for both presets, under the documented weight rule.

What is captured, per preset (ncsnpp_cifar10: 32x32 conditional, [2,2,2]; ncsnpp_ffhq64: 64x64 unconditional, [1,2,2,2])
  <p>_x, _sigma, _label_idx, _D   a 2-row forward of the reference EDMPrecond (x fp64 -> D fp32), per-row sigma (one large, one small)
  <p>_D64                          the same forward with the reference module in float64 (`module.double()`) and the preconditioning
                                   (networks.py:654-668) done by hand in float64
  <p>_freqs                        the Fourier embedding's frequency buffer (also re-created by the initialiser; here for the embedding test)
  manifest[<p>].ref_f32_vs_f64     max|D - D64| / max(1, max|D64|): the reference's own fp32 noise on this architecture
and for the CIFAR network the two searches make_golden_configs01.py records for DDPM++ (NAIVE; REJECTION N = 16 with the brightness
scorer) through the reference's generate_image_grid: rewards, the kept trajectory, final state, PNG.
"""
import copy
import json
import os
import sys
import time

assert os.environ.get('PYTHONHASHSEED') == '0', 'run with PYTHONHASHSEED=0 (edm/main.py:776 hashes strings)'

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                       # the import recipe, run_ref_search, the weight checks  # noqa: E402

import numpy as np                             # noqa: E402
import torch                                   # noqa: E402

from diffusion_tts_amd import init as dinit    # noqa: E402
from diffusion_tts_amd.config import ncsnpp_cifar10, ncsnpp_ffhq64  # noqa: E402

torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
KW = dict(num_steps=18, seed=0)
PRESETS = {'ncsnpp_cifar10': ncsnpp_cifar10, 'ncsnpp_ffhq64': ncsnpp_ffhq64}
# per preset: (generator seed, per-row sigma, label indices)
FWD = {'ncsnpp_cifar10': (5151, [40.0, 0.05], [3, 7]), 'ncsnpp_ffhq64': (5252, [0.02, 60.0], None)}


def ref_ncsnpp(cfg, seed):
    torch.manual_seed(seed)
    return mg.ref_networks.EDMPrecond(
        img_resolution=cfg.img_resolution, img_channels=cfg.img_channels, label_dim=cfg.label_dim, model_type='SongUNet',
        model_channels=cfg.model_channels, channel_mult=cfg.channel_mult, num_blocks=cfg.num_blocks, attn_resolutions=cfg.attn_resolutions,
        augment_dim=cfg.augment_dim, embedding_type=cfg.embedding_type, encoder_type=cfg.encoder_type, decoder_type='standard',
        channel_mult_noise=cfg.channel_mult_noise, resample_filter=cfg.resample_filter, dropout=0.13).eval()


def ref_full(cfg, seed):
    """the reference module carrying the product initialiser's weights (checked equal to its own constructor's) + the weight rule"""
    mod = ref_ncsnpp(cfg, seed)
    sd = dinit.edm_state_dict(cfg, seed)
    ref_sd = mod.state_dict()
    assert list(ref_sd.keys()) == list(sd.keys()), ([k for k in ref_sd if k not in sd][:5], [k for k in sd if k not in ref_sd][:5])
    params = [k for k, _ in mod.named_parameters()]
    mg.assert_same_params(mod, {k: sd[k] for k in params}, cfg.encoder_type)
    for k in ref_sd:                                                      # the buffers too: freqs draw, filter taps
        assert ref_sd[k].shape == sd[k].shape and torch.equal(ref_sd[k], sd[k]), k
    ck_ref = dinit.checksum(ref_sd)                                       # (before the load below rewrites these tensors in place)
    sd2, refilled = dinit.refill_degenerate(sd, seed)
    mod.load_state_dict(sd2, strict=True)
    rec = dict(keys=list(ref_sd.keys()), buffers=[k for k in ref_sd if k not in params],
               checksum=dinit.checksum(sd2), checksum_raw=dinit.checksum(sd), checksum_reference_raw=ck_ref,
               refilled=len(refilled), params=sum(v.numel() for v in sd.values()))
    return mod, sd2, rec


def forward_f64(mod, x, sigma, labels):
    """EDMPrecond.forward (networks.py:654-668) with every step in float64"""
    m64 = copy.deepcopy(mod).double()
    sd_ = float(mod.sigma_data)
    s = sigma.to(torch.float64).reshape(-1, 1, 1, 1)
    c_skip = sd_ ** 2 / (s ** 2 + sd_ ** 2)
    c_out = s * sd_ / (s ** 2 + sd_ ** 2).sqrt()
    c_in = 1 / (sd_ ** 2 + s ** 2).sqrt()
    c_noise = s.log() / 4
    lab = None if labels is None else labels.to(torch.float64)
    F = m64.model(c_in * x, c_noise.flatten(), class_labels=lab)
    assert F.dtype == torch.float64
    return c_skip * x + c_out * F


def main():
    t00 = time.time()
    out, man = {}, dict(torch=torch.__version__, numpy=np.__version__, threads=torch.get_num_threads(), net_seed=mg.NET_SEED,
                        S=dict(S_churn=40, S_min=0.05, S_max=50, S_noise=1.003), **KW)
    nets = {}
    for name, preset in PRESETS.items():
        cfg = preset()
        mod, sd2, rec = ref_full(cfg, mg.NET_SEED)
        nets[name] = mod
        gseed, sig, lab_idx = FWD[name]
        g = torch.Generator().manual_seed(gseed)
        sigma = torch.tensor(sig, dtype=torch.float64)
        r = cfg.img_resolution
        x = torch.randn(2, 3, r, r, generator=g, dtype=torch.float64) * (sigma ** 2 + 0.25).sqrt().reshape(-1, 1, 1, 1)
        labels = None if lab_idx is None else torch.eye(cfg.label_dim)[torch.tensor(lab_idx)]
        with torch.no_grad():
            D = mod(x, sigma, labels)
            D64 = forward_f64(mod, x, sigma, labels)
        assert D.dtype == torch.float32
        rec['ref_f32_vs_f64'] = float((D.double() - D64).abs().max() / max(1.0, float(D64.abs().max())))
        rec['cfg'] = cfg.__dict__
        man[name] = rec
        out[f'{name}_x'], out[f'{name}_sigma'], out[f'{name}_D'], out[f'{name}_D64'] = x.numpy(), sigma.numpy(), D.numpy(), D64.numpy()
        out[f'{name}_label_idx'] = np.array([] if lab_idx is None else lab_idx, dtype=np.int64)
        out[f'{name}_freqs'] = sd2['model.map_noise.freqs'].numpy()
        print(f'[{time.time() - t00:6.1f}s] {name}: {len(rec["keys"])} keys, {rec["params"]} values, max|D| {float(D.abs().max()):.3f}, '
              f'ref_f32_vs_f64 {rec["ref_f32_vs_f64"]:.3e}', flush=True)

    net = nets['ncsnpp_cifar10']
    bright = mg.ref_scorers.BrightnessScorer()
    # ---- NAIVE, 18 Heun steps (the inputs of configs[0])
    lat = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(0))
    lab = torch.eye(10)[torch.tensor([3])]
    with torch.no_grad():
        lg, sl, png, err = mg.run_ref_search(net, bright, lat, lab, 'NAIVE', {}, KW['num_steps'], seed=KW['seed'])
    assert err is None, err
    rows = int(sum(c[0].shape[0] for c in lg.calls))
    assert rows == 35 and len(sl.calls) == 1
    out.update(naive_latents=lat.numpy(), naive_x_final=lg.calls[-1][2].double().numpy(), naive_image=png, naive_final_score=sl.calls[-1][1].numpy())
    man['naive'] = dict(label=3, latent_seed=0, net_rows=rows, scorer_calls=len(sl.calls))
    print(f'[{time.time() - t00:6.1f}s] naive: {rows} rows, final score {float(sl.calls[-1][1][0]):.6f}', flush=True)
    # ---- REJECTION N = 16, brightness (the inputs of configs[1])
    lat = torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    lab = torch.eye(10)[torch.tensor([7])]
    with torch.no_grad():
        lg, sl, png, err = mg.run_ref_search(net, bright, lat, lab, 'REJECTION_SAMPLING', dict(N=16), KW['num_steps'], seed=KW['seed'])
    assert err is None, err
    rows = int(sum(c[0].shape[0] for c in lg.calls))
    assert rows == 16 * 35 and len(sl.calls) == 2 and sl.calls[0][1].shape[0] == 16
    rew = sl.calls[0][1].numpy()
    last = lg.calls[-1][2].double()
    q = (last * 127.5 + 128).clip(0, 255).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    kept = [j for j in range(16) if np.array_equal(q[j], png)]          # the trajectory the reference kept, read off its final image
    assert len(kept) >= 1, 'the final image is none of the 16 trajectories'
    srt = np.sort(rew)[::-1]
    out.update(rej_latents=lat.numpy(), rej_rewards=rew, rej_kept=np.array(kept[:1], dtype=np.int64), rej_x_final=last[kept[0]:kept[0] + 1].numpy(),
               rej_image=png, rej_final_score=sl.calls[-1][1].numpy())
    man['rejection'] = dict(label=7, latent_seed=1, params=dict(N=16), net_rows=rows, scorer_calls=len(sl.calls), kept=int(kept[0]),
                            rows_with_that_image=len(kept), argmax_of_rewards=int(rew.argmax()), top2_gap=float(srt[0] - srt[1]))
    print(f'[{time.time() - t00:6.1f}s] rejection: {rows} rows, kept {kept[0]} (argmax {int(rew.argmax())}, top-2 gap {srt[0] - srt[1]:.3e})', flush=True)
    np.savez_compressed(os.path.join(HERE, 'ncsnpp_golden.npz'), **out)
    with open(os.path.join(HERE, 'ncsnpp_manifest.json'), 'w') as f:
        json.dump(man, f, indent=1)
    print(f'[{time.time() - t00:6.1f}s] wrote ncsnpp_golden.npz ({os.path.getsize(os.path.join(HERE, "ncsnpp_golden.npz"))} bytes)')


if __name__ == '__main__':
    main()
