"""GPU: the SD U-Net with downsample='strided' (diffusion_tts_amd/sd_unet.py): the three Downsample2D layers as the stride-2 3x3 convolution
they are (ops.conv2d(stride=2) over C channels) instead of space-to-depth + a stride-1 convolution over 4*C channels, against the goldens of
tests/test_gpu_sd_unet.py under the same tolerance (manifest `tolerance_factor` x the reference module's own error in that 16-bit type, and
the manifest's sensitivity margin).  The golden latent is 16x16: the downsamplers write 8x8 (64 pixels: one strip per sample, so the
epilogue emits the next GroupNorm's statistics), 4x4 and 2x2 (no whole strip: GroupNorm's own pass) -- both branches of the strided launch.
One model per (case, dtype, mode) per module, one state dict per case."""
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


def model(gold, case, dname, downsample='strided', head_dims='padded', **kw):
    """built once per (case, dtype, modes) per module from one state dict per case; downsample=None: the keyword is left out"""
    from diffusion_tts_amd.sd_unet import SDUNet
    c = gold[1]['cases'][case]
    key = (case, dname, downsample, head_dims)
    if key not in _CACHE:
        if case not in _CACHE:
            _CACHE[case] = dinit.sd_unet_state_dict(tuple(c['block_out_channels']), c['heads'], c['cross_attention_dim'], 2, seed=c['seed'])
        mode = {} if downsample is None else {'downsample': downsample}
        _CACHE[key] = SDUNet(_CACHE[case], device=DEV, dtype=DT[dname], head_dims=head_dims, **mode, **case_args(c))
    return _CACHE[key]


def drop(*keys):
    for k in keys:
        _CACHE.pop(k, None)
    torch.cuda.empty_cache()


def rel(got, want):
    return float((got.double().cpu() - want.double().cpu()).abs().max() / want.double().abs().max())


def golden_inputs(gold, name, dtype):
    x, ctx, t, want = (torch.from_numpy(gold[0][f'{name}_{k}']) for k in ('x', 'context', 't', 'y'))
    return x.to(DEV, dtype), t.to(DEV), ctx.to(DEV, dtype), want


def assert_meets_golden(gold, case, dname, unet, what):
    vg, man = gold
    c = man['cases'][case]
    x, t, ctx, want = golden_inputs(gold, case, DT[dname])
    got = unet(x, t, encoder_hidden_states=ctx, return_dict=False)[0]
    assert got.dtype == DT[dname] and tuple(got.shape) == tuple(want.shape)
    tol = man['tolerance_factor'] * c['own_error'][dname]
    err = rel(got.float(), want)
    print(f'SDUNet {case} {dname} {what}: rel. max err {err:.3e} (tolerance {tol:.3e} = {man["tolerance_factor"]} x the reference module\'s own '
          f'{c["own_error"][dname]:.3e})')
    assert tol * man['sensitivity_margin'] <= min(c['context_swap_change'], c['timestep_shift_change'])
    assert bool(torch.isfinite(got).all()) and err < tol, (err, tol)
    return got


@pytest.mark.parametrize('dname', ['float16', 'bfloat16'])
@pytest.mark.parametrize('case', ['sd15', 'narrow'])
def test_strided_matches_reference(gold, case, dname):
    from diffusion_tts_amd import ops
    unet = model(gold, case, dname)
    boc = gold[1]['cases'][case]['block_out_channels']
    assert unet.downsample == 'strided'
    ds = [d for _, d in unet.down]
    assert ds[3] is None and [tuple(d[0].shape) for d in ds[:3]] == [(c, 3, 3, c) for c in boc[:3]]          # plain 3x3 layers over C channels
    assert_meets_golden(gold, case, dname, unet, "downsample='strided'")
    # the launches the forward just made, at its shapes: 16x16 -> 8x8 writes the statistics from the epilogue or the reduce pass, 8x8 -> 4x4
    # and 4x4 -> 2x2 cannot (no whole 64-pixel strip) and leave them to GroupNorm's own pass
    for i, hw in enumerate((16, 8, 4)):
        x = torch.zeros(1, hw, hw, boc[i], dtype=DT[dname], device=DEV)
        plan = ops.conv_plan(x, *ds[i], stride=2, gn_stats=True)
        out = ops.conv2d(x, *ds[i], stride=2, gn_stats=True)
        assert tuple(out.shape) == (1, hw // 2, hw // 2, boc[i]) and (plan['kernel'], plan['refused']) == (0, 0)
        assert (out._gn_stats is not None) == (hw == 16) == bool(plan['stats_written'])
    if case == 'narrow':
        drop((case, dname, 'strided', 'padded'))


@pytest.mark.parametrize('dname', ['float16', 'bfloat16'])
def test_s2d_is_the_default_bit_for_bit(gold, dname):
    """the default model and downsample='s2d' are one network (4*C input channels in the downsamplers: the parent's path)"""
    boc = gold[1]['cases']['narrow']['block_out_channels']
    x, t, ctx, _ = golden_inputs(gold, 'narrow', DT[dname])
    default, s2d, strided = model(gold, 'narrow', dname, None), model(gold, 'narrow', dname, 's2d'), model(gold, 'narrow', dname, 'strided')
    assert default.downsample == s2d.downsample == 's2d' and strided.downsample == 'strided'
    for u, mult in ((default, 4), (s2d, 4), (strided, 1)):
        assert [tuple(d[0].shape) for _, d in u.down[:3]] == [(c, 3, 3, mult * c) for c in boc[:3]]
    a, b = (u(x, t, encoder_hidden_states=ctx, return_dict=False)[0] for u in (default, s2d))
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    drop(*[('narrow', dname, m, 'padded') for m in (None, 's2d', 'strided')])


def test_strided_against_s2d_reported(gold):
    """a record: each mode meets the golden on its own; the two sum the same nine live taps in different orders (and different K splits), so
    they are not expected to agree bit for bit"""
    x, t, ctx, want = golden_inputs(gold, 'sd15', torch.float16)
    a = model(gold, 'sd15', 'float16')(x, t, encoder_hidden_states=ctx, return_dict=False)[0]
    s2d = model(gold, 'sd15', 'float16', 's2d')
    assert [tuple(d[0].shape)[3] for _, d in s2d.down[:3]] == [4 * c for c in gold[1]['cases']['sd15']['block_out_channels'][:3]]
    b = assert_meets_golden(gold, 'sd15', 'float16', s2d, "downsample='s2d'")
    print(f'SDUNet sd15 float16: rel. max |strided - s2d| = {rel(a.float(), b.float()):.3e}; against the golden: strided {rel(a.float(), want):.3e}, '
          f's2d {rel(b.float(), want):.3e}')
    drop(('sd15', 'float16', 's2d', 'padded'))


def test_native_heads_with_strided_meet_the_golden(gold):
    unet = model(gold, 'sd15', 'float16', 'strided', 'native')
    assert (unet.head_dims, unet.downsample) == ('native', 'strided')
    assert_meets_golden(gold, 'sd15', 'float16', unet, "head_dims='native', downsample='strided'")
    drop(('sd15', 'float16', 'strided', 'native'))


def test_strided_rows_are_independent_and_identical_rows_bit_identical(gold):
    vg, man = gold
    c = man['cases']['sd15']
    unet = model(gold, 'sd15', 'float16')
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
        print(f'SDUNet sd15 strided, row {r} alone vs in a batch of 6: rel. max diff {err:.3e} (tolerance {tol:.3e})')
        assert err < tol


def test_strided_replay_is_bit_identical_to_eager(gold):
    """a shape no other test of this module uses (3 rows, 3 contexts): the third sighting replays the captured graph"""
    c = gold[1]['cases']['sd15']
    unet = model(gold, 'sd15', 'float16')
    G = unet._graphs
    assert G.enabled
    captures, replays = G.captures, G.replays
    calls = []
    for i in range(4):
        g = torch.Generator().manual_seed(300 + i)
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
    """a diffusers `unet/` directory of a small model, through SDUNet.from_pretrained and main.load_sd_unet(..., downsample='strided'):
    bit-identical to the state-dict constructor; the loader's default stays 's2d'"""
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
    a = SDUNet.from_pretrained(str(d), device=DEV, dtype=torch.float16, downsample='strided')
    sys.path.insert(0, ROOT)
    import main as cli
    os.environ['DTS_SD_UNET_DIR'] = str(d)
    try:
        b = cli.load_sd_unet('runwayml/stable-diffusion-v1-5', torch.device(DEV), 'hip', downsample='strided')
        p = cli.load_sd_unet('runwayml/stable-diffusion-v1-5', torch.device(DEV), 'hip')
        with pytest.raises(ValueError, match='--unet-downsample'):
            cli.load_sd_unet('runwayml/stable-diffusion-v1-5', torch.device(DEV), 'hip', downsample='bogus')
    finally:
        del os.environ['DTS_SD_UNET_DIR']
    args = dict(block_out_channels=boc, attention_head_dim=heads, cross_attention_dim=cd, layers_per_block=2, sample_size=16)
    ref = SDUNet({k: v.float() for k, v in sd.items()}, device=DEV, dtype=torch.float16, downsample='strided', **args)
    assert a.downsample == b.downsample == ref.downsample == 'strided' and p.downsample == 's2d'
    assert [d_[0].shape[3] for _, d_ in b.down[:3]] == list(boc[:3]) and [d_[0].shape[3] for _, d_ in p.down[:3]] == [4 * c for c in boc[:3]]
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 4, 16, 16, generator=g).to(DEV, torch.float16)
    ctx = torch.randn(2, 11, cd, generator=g).to(DEV, torch.float16)
    run = lambda u: u(x, 500, encoder_hidden_states=ctx, return_dict=False)[0]
    want = run(ref)
    assert bool(torch.isfinite(want).all()) and torch.equal(run(a), want) and torch.equal(run(b), want)
    print(f'SDUNet 64 / 128 / 192 channels, float16: rel. max |strided - s2d| = {rel(want.float(), run(p).float()):.3e}')
    assert bool(torch.isfinite(run(p)).all())          # (the difference is a record: this model has no golden to take a tolerance from)
