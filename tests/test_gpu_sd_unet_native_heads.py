"""GPU: the SD U-Net with head_dims='native' (diffusion_tts_amd/sd_unet.py): SD-1.x's heads of 40 / 80 / 160 channels kept as stored, on the
attention kernels' native forms, against the goldens of tests/test_gpu_sd_unet.py under the same tolerance (manifest `tolerance_factor` x
the reference module's own error in that 16-bit type, and the manifest's sensitivity margin).  The golden latent is 16x16, so the
transformer blocks see 256 / 64 / 16 / 4 tokens: the smallest shape that reaches all three head dims in both attention kernels.
One SD-1.5-width model per dtype per module, one state dict for all of them."""
import json
import os

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


_CACHE = {}


def sd15(gold, dname, head_dims='native'):
    """the SD-1.5-width model, built once per (dtype, mode) per module from one state dict"""
    from diffusion_tts_amd.sd_unet import SDUNet
    c = gold[1]['cases']['sd15']
    if (dname, head_dims) not in _CACHE:
        if 'sd' not in _CACHE:
            _CACHE['sd'] = dinit.sd_unet_state_dict(tuple(c['block_out_channels']), c['heads'], c['cross_attention_dim'], 2, seed=c['seed'])
        _CACHE[dname, head_dims] = SDUNet(_CACHE['sd'], device=DEV, dtype=DT[dname], head_dims=head_dims, **case_args(c))
    return _CACHE[dname, head_dims]


def rel(got, want):
    return float((got.double().cpu() - want.double().cpu()).abs().max() / want.double().abs().max())


def golden_inputs(gold, name, dtype):
    x, ctx, t, want = (torch.from_numpy(gold[0][f'{name}_{k}']) for k in ('x', 'context', 't', 'y'))
    return x.to(DEV, dtype), t.to(DEV), ctx.to(DEV, dtype), want


@pytest.mark.parametrize('dname', ['float16', 'bfloat16'])
def test_native_sd15_matches_reference(gold, dname):
    vg, man = gold
    c = man['cases']['sd15']
    unet = sd15(gold, dname)
    assert unet.head_dims == 'native' and len(unet._tfm) == 16
    boc = c['block_out_channels']
    widths = sorted(A.hp for A in unet._tfm)
    assert all(A.hp in boc and A.w_qkv.shape[0] == 3 * A.hp for A in unet._tfm) and set(widths) == set(boc), widths      # nothing padded
    x, t, ctx, want = golden_inputs(gold, 'sd15', DT[dname])
    got = unet(x, t, encoder_hidden_states=ctx, return_dict=False)[0]
    assert got.dtype == DT[dname] and tuple(got.shape) == tuple(want.shape)
    tol = man['tolerance_factor'] * c['own_error'][dname]
    err = rel(got.float(), want)
    print(f'SDUNet sd15 {dname} head_dims=native: rel. max err {err:.3e} (tolerance {tol:.3e} = {man["tolerance_factor"]} x the reference module\'s own '
          f'{c["own_error"][dname]:.3e})')
    assert tol * man['sensitivity_margin'] <= min(c['context_swap_change'], c['timestep_shift_change'])
    assert bool(torch.isfinite(got).all()) and err < tol, (err, tol)


def test_native_against_padded_reported(gold):
    """a record, not an assertion beyond the golden tolerance each mode meets on its own: the projections may take other launch plans at
    320 than at 512 channels, so the two modes are not expected to agree bit for bit over the whole network"""
    x, t, ctx, want = golden_inputs(gold, 'sd15', torch.float16)
    a = sd15(gold, 'float16')(x, t, encoder_hidden_states=ctx, return_dict=False)[0]
    padded = sd15(gold, 'float16', 'padded')
    assert padded.head_dims == 'padded' and sorted({A.hp for A in padded._tfm}) == [512, 1024, 2048]
    b = padded(x, t, encoder_hidden_states=ctx, return_dict=False)[0]
    print(f'SDUNet sd15 float16: rel. max |native - padded| = {rel(a.float(), b.float()):.3e}; against the golden: native {rel(a.float(), want):.3e}, '
          f'padded {rel(b.float(), want):.3e}')
    del _CACHE['float16', 'padded']
    torch.cuda.empty_cache()


@pytest.mark.parametrize('dname', ['float16', 'bfloat16'])
def test_narrow_model_is_unchanged_by_the_mode(gold, dname):
    """2 heads of 32 / 64 / 96 / 96 channels: 2 x 40 = 80 is no multiple of 64, so native_head_dim falls back to 64 / 64 / 128 / 128 -- the
    padded widths -- and the two modes are the same network, bit for bit"""
    from diffusion_tts_amd.sd_unet import SDUNet
    c = gold[1]['cases']['narrow']
    sd = dinit.sd_unet_state_dict(tuple(c['block_out_channels']), c['heads'], c['cross_attention_dim'], 2, seed=c['seed'])
    x, t, ctx, _ = golden_inputs(gold, 'narrow', DT[dname])
    outs = {}
    for mode in ('padded', 'native'):
        unet = SDUNet(sd, device=DEV, dtype=DT[dname], head_dims=mode, **case_args(c))
        outs[mode] = (unet(x, t, encoder_hidden_states=ctx, return_dict=False)[0], [A.hp for A in unet._tfm])
    assert outs['native'][1] == outs['padded'][1]
    assert torch.equal(outs['native'][0], outs['padded'][0])


def test_native_rows_are_independent_and_identical_rows_bit_identical(gold):
    vg, man = gold
    c = man['cases']['sd15']
    unet = sd15(gold, 'float16')
    g = torch.Generator().manual_seed(5)
    x1, x2 = torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 4, 16, 16, generator=g)
    cu, cc = (torch.randn(1, c['context_len'], c['cross_attention_dim'], generator=g) for _ in range(2))
    x = torch.cat([x1, x1, x2, x1, x1, x2]).to(DEV, torch.float16)
    ehs = torch.cat([cu.expand(3, -1, -1), cc.expand(3, -1, -1)]).to(DEV, torch.float16)
    out = unet(x, 500, encoder_hidden_states=ehs, return_dict=False)[0]
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out[0], out[1]) and torch.equal(out[3], out[4])
    assert not torch.equal(out[0], out[2]) and not torch.equal(out[0], out[3])
    tol = man['tolerance_factor'] * c['own_error']['float16']
    scale = float(out.float().abs().max())
    for r in (2, 3):
        single = unet(x[r:r + 1].contiguous(), 500, encoder_hidden_states=ehs[r:r + 1].contiguous(), return_dict=False)[0]
        err = float((single[0].float() - out[r].float()).abs().max()) / scale
        print(f'SDUNet sd15 native, row {r} alone vs in a batch of 6: rel. max diff {err:.3e} (tolerance {tol:.3e})')
        assert err < tol


def test_native_replay_is_bit_identical_to_eager(gold):
    """a shape no other test of this module uses (3 rows, 3 contexts): the third sighting replays the captured graph"""
    c = gold[1]['cases']['sd15']
    unet = sd15(gold, 'float16')
    G = unet._graphs
    assert G.enabled
    captures, replays = G.captures, G.replays
    calls = []
    for i in range(4):
        g = torch.Generator().manual_seed(200 + i)
        x = torch.randn(3, 4, 16, 16, generator=g).to(DEV, torch.float16)
        ehs = torch.randn(3, c['context_len'], c['cross_attention_dim'], generator=g).to(DEV, torch.float16)
        t = 900 - 170 * i
        calls.append((x, t, ehs, unet(x, t, encoder_hidden_states=ehs, return_dict=False)[0]))
    assert G.captures == captures + 1 and G.replays >= replays + 2, G.path_report()
    G.enabled = False
    try:
        for x, t, ehs, got in calls:
            assert bool(torch.isfinite(got).all())
            assert torch.equal(got, unet(x, t, encoder_hidden_states=ehs, return_dict=False)[0])
    finally:
        G.enabled = True
    assert not torch.equal(calls[2][3], calls[3][3])             # the replays read their own inputs


def test_the_mode_reaches_the_model_through_from_pretrained_and_the_command_lines_loader(tmp_path):
    """a diffusers `unet/` directory of a small model with 8 heads of 8 / 16 / 24 / 24 channels: native_head_dim gives 40 everywhere (padded:
    64), through SDUNet.from_pretrained and through main.load_sd_unet(..., head_dims='native'), bit-identical to the state-dict constructor"""
    import sys
    from safetensors.torch import save_file
    from diffusion_tts_amd.sd_unet import SDUNet
    boc, heads, cd = (64, 128, 192, 192), 8, 64
    sd = {k: v.to(torch.float16).contiguous() for k, v in dinit.sd_unet_state_dict(boc, heads, cd, 2, seed=3).items()}
    d = tmp_path / 'unet'
    d.mkdir()
    save_file(sd, str(d / 'diffusion_pytorch_model.safetensors'))
    (d / 'config.json').write_text(json.dumps({'_class_name': 'UNet2DConditionModel', 'act_fn': 'silu', 'attention_head_dim': heads,
                                               'block_out_channels': list(boc), 'cross_attention_dim': cd, 'layers_per_block': 2,
                                               'norm_num_groups': 32, 'sample_size': 16, 'in_channels': 4, 'out_channels': 4,
                                               'down_block_types': ['CrossAttnDownBlock2D'] * 3 + ['DownBlock2D'],
                                               'up_block_types': ['UpBlock2D'] + ['CrossAttnUpBlock2D'] * 3, 'use_linear_projection': False}))
    a = SDUNet.from_pretrained(str(d), device=DEV, dtype=torch.float16, head_dims='native')
    sys.path.insert(0, ROOT)
    import main as cli
    os.environ['DTS_SD_UNET_DIR'] = str(d)
    try:
        b = cli.load_sd_unet('runwayml/stable-diffusion-v1-5', torch.device(DEV), 'hip', head_dims='native')
        p = cli.load_sd_unet('runwayml/stable-diffusion-v1-5', torch.device(DEV), 'hip')
    finally:
        del os.environ['DTS_SD_UNET_DIR']
    args = dict(block_out_channels=boc, attention_head_dim=heads, cross_attention_dim=cd, layers_per_block=2, sample_size=16)
    ref = SDUNet({k: v.float() for k, v in sd.items()}, device=DEV, dtype=torch.float16, head_dims='native', **args)
    assert a.head_dims == b.head_dims == ref.head_dims == 'native' and p.head_dims == 'padded'
    assert {A.hp for A in b._tfm} == {8 * 40} and {A.hp for A in p._tfm} == {8 * 64}
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 4, 16, 16, generator=g).to(DEV, torch.float16)
    ctx = torch.randn(2, 11, cd, generator=g).to(DEV, torch.float16)
    run = lambda u: u(x, 500, encoder_hidden_states=ctx, return_dict=False)[0]
    want = run(ref)
    assert bool(torch.isfinite(want).all()) and torch.equal(run(a), want) and torch.equal(run(b), want)
    diff = rel(want.float(), run(p).float())
    print(f'SDUNet 8 heads of 8 / 16 / 24 channels, float16: rel. max |native (40) - padded (64)| = {diff:.3e}')
    assert bool(torch.isfinite(run(p)).all())          # (the difference is a record: this model has no golden to take a tolerance from)
