"""GPU: the SD U-Net on the HIP kernels (diffusion_tts_amd/sd_unet.py) against the reference's UNet2DConditionModel.forward (goldens of
tests/golden/make_golden_sd_unet.py: fp32, CPU), at a narrow width with a head dim that is not a power of two and at SD-1.5's own
configuration, in both activation types; its row independence, timestep forms and weight ingestion; and as the `unet` of the SD search loop
beside the HIP VAE decoder at [1,4,64,64].

Tolerance of the golden comparison: 3 x the reference module's OWN error in that 16-bit type against its fp32 output (manifest
`own_error`, measured by the generator on the CPU): two independent 16-bit pipelines differ in accumulation order and in where they round;
3 x leaves room for that and stays >= 5 x below what ignoring the text or the timestep would cost (manifest `context_swap_change`,
`timestep_shift_change`)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ROOT                                        # noqa: E402
from diffusion_tts_amd import init as dinit                      # noqa: E402

DEV = 'cuda'
DT = {'float16': torch.float16, 'bfloat16': torch.bfloat16}


@pytest.fixture(scope='module')
def gold():
    with open(os.path.join(ROOT, 'tests', 'golden', 'sd_unet_manifest.json')) as f:
        return np.load(os.path.join(ROOT, 'tests', 'golden', 'sd_unet_golden.npz')), json.load(f)


def case_args(c):
    return dict(block_out_channels=tuple(c['block_out_channels']), attention_head_dim=c['heads'], cross_attention_dim=c['cross_attention_dim'],
                layers_per_block=2, sample_size=c['latent'][-1])


def case_state_dict(c):
    return dinit.sd_unet_state_dict(tuple(c['block_out_channels']), c['heads'], c['cross_attention_dim'], 2, seed=c['seed'])


_SD15 = {}


def sd15_unet(gold):
    """the SD-1.5-width model in float16, built once per module (860 M parameters)"""
    if 'fp16' not in _SD15:
        from diffusion_tts_amd.sd_unet import SDUNet
        c = gold[1]['cases']['sd15']
        _SD15['fp16'] = SDUNet(case_state_dict(c), device=DEV, dtype=torch.float16, **dict(case_args(c), sample_size=64))
    return _SD15['fp16']


def rel(got, want):
    return float((got.double().cpu() - want.double()).abs().max() / want.double().abs().max())


@pytest.mark.parametrize('dname', ['float16', 'bfloat16'])
@pytest.mark.parametrize('name', ['narrow', 'sd15'])
def test_hip_sd_unet_matches_reference(gold, name, dname):
    from diffusion_tts_amd.sd_unet import SDUNet
    vg, man = gold
    c = man['cases'][name]
    dtype = DT[dname]
    if name == 'sd15' and dname == 'float16':
        unet = sd15_unet(gold)
    else:
        unet = SDUNet(case_state_dict(c), device=DEV, dtype=dtype, **case_args(c))
    x, ctx, t, want = (torch.from_numpy(vg[f'{name}_{k}']) for k in ('x', 'context', 't', 'y'))
    got = unet(x.to(DEV, dtype), t.to(DEV), encoder_hidden_states=ctx.to(DEV, dtype), return_dict=False)[0]
    assert got.dtype == dtype and tuple(got.shape) == tuple(want.shape) and unet.dtype == dtype and unet.config.in_channels == 4
    tol = man['tolerance_factor'] * c['own_error'][dname]
    err = rel(got.float(), want)
    print(f'SDUNet {name} {dname}: rel. max err {err:.3e} (tolerance {tol:.3e} = {man["tolerance_factor"]} x the reference module\'s own {c["own_error"][dname]:.3e}; '
          f'context swap {c["context_swap_change"]:.2f}, timestep shift {c["timestep_shift_change"]:.2f})')
    assert tol * man['sensitivity_margin'] <= min(c['context_swap_change'], c['timestep_shift_change'])
    assert err < tol, (err, tol)
    del unet
    torch.cuda.empty_cache()


def test_rows_are_independent_identical_rows_are_bit_identical_and_timestep_forms_agree(gold):
    """A 2N-row call (two distinct contexts, as the search loop's cond / uncond halves) equals per-row calls within the golden tolerance;
    identical rows give bit-identical outputs; a scalar timestep equals the same value per row bit for bit."""
    from diffusion_tts_amd.sd_unet import SDUNet
    vg, man = gold
    c = man['cases']['narrow']
    unet = SDUNet(case_state_dict(c), device=DEV, dtype=torch.float16, **case_args(c))
    g = torch.Generator().manual_seed(5)
    x1, x2 = torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 4, 16, 16, generator=g)
    cu, cc = torch.randn(1, c['context_len'], c['cross_attention_dim'], generator=g), torch.randn(1, c['context_len'], c['cross_attention_dim'], generator=g)
    x = torch.cat([x1, x1, x2, x1, x1, x2]).to(DEV, torch.float16)
    ehs = torch.cat([cu.expand(3, -1, -1), cc.expand(3, -1, -1)]).to(DEV, torch.float16)
    out = unet(x, 500, encoder_hidden_states=ehs, return_dict=False)[0]
    assert unet.rows == 6 and torch.isfinite(out).all()
    assert torch.equal(out[0], out[1]) and torch.equal(out[3], out[4])
    assert not torch.equal(out[0], out[2]) and not torch.equal(out[0], out[3])
    per_row = unet(x, torch.full((6,), 500, device=DEV), encoder_hidden_states=ehs, return_dict=False)[0]
    assert torch.equal(per_row, out)
    per_row = unet(x, torch.tensor(500), encoder_hidden_states=ehs, return_dict=False)[0]
    assert torch.equal(per_row, out)
    other_t = unet(x, torch.tensor([500, 480, 500, 500, 500, 500], device=DEV), encoder_hidden_states=ehs, return_dict=False)[0]
    assert torch.equal(other_t[0], out[0]) and not torch.equal(other_t[1], out[1])
    tol = man['tolerance_factor'] * c['own_error']['float16']
    scale = float(out.float().abs().max())
    for r in (2, 3):
        single = unet(x[r:r + 1].contiguous(), 500, encoder_hidden_states=ehs[r:r + 1].contiguous(), return_dict=False)[0]
        err = float((single[0].float() - out[r].float()).abs().max()) / scale
        print(f'SDUNet row {r} alone vs in a batch of 6: rel. max diff {err:.3e} (tolerance {tol:.3e})')
        assert err < tol
    with pytest.raises(ValueError):
        unet(x, 500, encoder_hidden_states=ehs[:2], return_dict=False)
    with pytest.raises(ValueError):
        unet(x, 500, encoder_hidden_states=ehs, class_labels=torch.zeros(6), return_dict=False)


def test_sd_unet_from_a_diffusers_directory(tmp_path, gold):
    """A diffusers `unet/` directory -- config.json + diffusion_pytorch_model.safetensors -- loads into the same model as the state dict does
    (bit-identical outputs), through from_pretrained and through the CLI's load_sd_unet; a directory with only a .bin pickle is refused."""
    from safetensors.torch import save_file
    from diffusion_tts_amd.sd_unet import SDUNet
    vg, man = gold
    c = man['cases']['narrow']
    sd = {k: v.to(torch.float16).contiguous() for k, v in case_state_dict(c).items()}
    d = tmp_path / 'unet'
    d.mkdir()
    save_file(sd, str(d / 'diffusion_pytorch_model.safetensors'))
    (d / 'config.json').write_text(json.dumps({'_class_name': 'UNet2DConditionModel', 'act_fn': 'silu', 'attention_head_dim': c['heads'],
                                               'block_out_channels': c['block_out_channels'], 'cross_attention_dim': c['cross_attention_dim'],
                                               'layers_per_block': 2, 'norm_num_groups': 32, 'sample_size': 16, 'in_channels': 4, 'out_channels': 4,
                                               'down_block_types': ['CrossAttnDownBlock2D'] * 3 + ['DownBlock2D'],
                                               'up_block_types': ['UpBlock2D'] + ['CrossAttnUpBlock2D'] * 3, 'use_linear_projection': False}))
    a = SDUNet.from_pretrained(str(d), device=DEV, dtype=torch.float16)
    sys.path.insert(0, ROOT)
    import main as cli
    os.environ['DTS_SD_UNET_DIR'] = str(d)
    try:
        b = cli.load_sd_unet('runwayml/stable-diffusion-v1-5', torch.device(DEV), 'hip')
    finally:
        del os.environ['DTS_SD_UNET_DIR']
    assert isinstance(b, SDUNet) and b.dtype == torch.float16 and b.config.sample_size == 16
    ref = SDUNet({k: v.float() for k, v in sd.items()}, device=DEV, dtype=torch.float16, **case_args(c))
    x, ctx, t = (torch.from_numpy(vg[f'narrow_{k}']).to(DEV) for k in ('x', 'context', 't'))
    run = lambda u: u(x.half(), t, encoder_hidden_states=ctx.half(), return_dict=False)[0]
    want = run(ref)
    assert torch.equal(run(a), want) and torch.equal(run(b), want)
    empty = tmp_path / 'empty'
    empty.mkdir()
    (empty / 'diffusion_pytorch_model.bin').write_bytes(b'x')
    with pytest.raises(FileNotFoundError):
        SDUNet.from_pretrained(str(empty))


@pytest.mark.parametrize('method,params,rows,scored', [
    ('eps_greedy', {'N': 3, 'K': 1, 'eps': 0.4, 'lambda': 2.0, 'B': 2, 'S': 4}, None, 2 * 3),
    ('beam', {'N': 4, 'B': 2, 'K': 20, 'lambda': 0.15, 'eps': 0.4, 'S': 8}, 2 * 2 * (2 + 2 * 4), 2 * 2 * 4 + 2)])
def test_sd_search_loop_on_the_hip_unet_and_vae(gold, method, params, rows, scored):
    """SDSearchPipeline(SDUNet, VAEDecoder) at the SD-1.5 configuration, [1,4,64,64] fp16 latents, 2 DDIM steps: the loop's U-Net rows all go
    through the HIP U-Net, the row / decode / scorer counts are the reference loop's (as tests/test_gpu_vae.py checks them around the
    stand-in U-Net), everything is finite, and a second run reproduces the first bit for bit."""
    from diffusion_tts_amd.sd_pipeline import SDSearchPipeline
    from diffusion_tts_amd.scorers import BrightnessScorer
    from diffusion_tts_amd.vae import VAEDecoder
    from sd_standins import TinyTextEncoder, TinyTokenizer
    unet = sd15_unet(gold)
    dec = VAEDecoder(dinit.vae_decoder_state_dict(seed=5), device=DEV, dtype=torch.float16)
    te = TinyTextEncoder().half().to(DEV)
    pipe = SDSearchPipeline(unet, dec, device=DEV, text_encoder=te, tokenizer=TinyTokenizer())
    runs = []
    for rep in range(2):
        torch.manual_seed(7)
        lat = torch.randn(1, 4, 64, 64).half()
        r0, d0 = unet.rows, dec.decodes
        out, score = pipe(prompt='a photo of a cat', latents=lat, num_inference_steps=2, score_function=BrightnessScorer(), method=method,
                          params=params, output_type='pt')
        runs.append((out, float(score), unet.rows - r0, dec.decodes - d0))
    out, score, unet_rows, decodes = runs[0]
    assert out.images.shape == (1, 3, 512, 512) and out.images.dtype == torch.float16
    assert unet_rows == out.unet_rows                                   # every row the loop counts went through the HIP U-Net
    if rows is not None:
        assert out.unet_rows == rows                                    # beam: per beam and step, the beam's cond + uncond + 2N candidate rows
    assert len(out.scores) == scored and decodes == scored + 1          # every candidate (and finalist) decoded and scored once, + the returned image
    sc = np.array(out.scores, dtype=np.float64)
    assert np.isfinite(sc).all() and np.isfinite(out.images.float().cpu().numpy()).all() and np.isfinite(score)
    assert runs[1][1] == score and torch.equal(runs[1][0].images, out.images) and runs[1][0].scores == out.scores and runs[1][2] == unet_rows
