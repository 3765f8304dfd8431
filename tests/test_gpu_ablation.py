"""GPU: the general ODE step kernels (dts_ode_xhat / _slope / _correct) against the float64 restatements and bounds of tests/ablation_reference.py,
and the two plain samplers, the per-row generator and the bulk generator against the reference's own runs
(tests/golden/make_golden_ablation.py) on the tiny networks."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ablation_reference as ar                                        # noqa: E402
import precond_helpers as ph                                           # noqa: E402
from elementwise_reference import WRAP                                 # noqa: E402
from helpers import tiny_edm                                           # noqa: E402

DEV = 'cuda'
X3 = 'f16x3'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
COUNTS = (3 * 768, 1, 771, WRAP)                # 3 rows of 3x16x16; one element; odd; the second trip of the grid-stride loop (2048 blocks of 256)
K = dict(ratio=0.93, coef=0.41, a=-1.7, b=0.37, step=-0.6, h=-0.8, alpha=0.75)
SCALES = (1.0, 0.3, 0.37)                       # s = 1: no x_in; 0.37: where a reciprocal-multiply would show (test_ablation_schedule.py)


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLDEN, 'ablation_golden.npz'))


@pytest.fixture(scope='module')
def man():
    with open(os.path.join(GOLDEN, 'ablation_manifest.json')) as f:
        return json.load(f)


def held(name, got, ref, bound):
    ratio, err = ar.worst(got.cpu(), ref, bound)
    print(f'{name}: max err {err:.3e}, {ratio:.3f} of the bound')
    assert ratio <= 1, name


def up(t):
    return None if t is None else t.to(DEV)


# ---- kernels -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('count', COUNTS)
def test_ode_xhat_matches_float64(ops, count):
    """x_hat within 8 e64 (|ratio x| + |coef eps|) for float64, float32 and absent noise; x_in absent at s = 1 (the state itself is the
    denoiser's input) and otherwise equal, bit for bit, to the IEEE quotient of the stored x_hat and s"""
    d = ar.ode_inputs(count, 11 + count % 97)
    for eps in (d['eps'], d['eps'].float(), None):
        coef = 0.0 if eps is None else K['coef']
        for s in SCALES:
            x_hat, x_in = ops.ode_xhat(up(d['x']), up(eps), K['ratio'], coef, s)
            (r_h, b_h), (r_i, b_i) = ar.ode_xhat_ref(d['x'], eps, K['ratio'], coef, s)
            tag = f'count {count}, eps {None if eps is None else eps.dtype}, s {s}'
            held(f'x_hat, {tag}', x_hat, r_h, b_h)
            if s == 1.0:
                assert x_in is x_hat
            else:
                held(f'x_in, {tag}', x_in, r_i, b_i)
                assert torch.equal(x_in.cpu(), ar.true_div(x_hat, s)), tag


@pytest.mark.parametrize('count', COUNTS)
def test_ode_slope_matches_float64(ops, count):
    """d, x_out and x_in for x = base (the sampler's two uses) and for a base of its own; d written and not written"""
    d = ar.ode_inputs(count, 23 + count % 97)
    for base in (None, d['base']):
        for s in SCALES:
            for want_d in (True, False):
                dd, x_out, x_in = ops.ode_slope(up(d['x']), up(d['D']), K['a'], K['b'], K['step'], s, base=up(base), want_d=want_d)
                (r_d, b_d), (r_o, b_o), (r_i, b_i) = ar.ode_slope_ref(d['x'], d['D'], K['a'], K['b'], d['x'] if base is None else base, K['step'], s)
                tag = f'count {count}, own base {base is not None}, s {s}, d {want_d}'
                assert (dd is not None) == want_d
                if want_d:
                    held(f'd, {tag}', dd, r_d, b_d)
                held(f'x_out, {tag}', x_out, r_o, b_o)
                if s == 1.0:
                    assert x_in is x_out
                else:
                    held(f'x_in, {tag}', x_in, r_i, b_i)
                    assert torch.equal(x_in.cpu(), ar.true_div(x_out, s)), tag


@pytest.mark.parametrize('count', COUNTS)
def test_ode_correct_matches_float64(ops, count):
    d = ar.ode_inputs(count, 37 + count % 97)
    for alpha in (1.0, K['alpha']):
        w1 = 1 / (2 * alpha)
        x_next = ops.ode_correct(up(d['base']), up(d['x']), up(d['D']), up(d['d']), K['a'], K['b'], K['h'], 1 - w1, w1)
        held(f'x_next, count {count}, alpha {alpha}', x_next, *ar.ode_correct_ref(d['base'], d['x'], d['D'], d['d'], K['a'], K['b'], K['h'], 1 - w1, w1))


def test_ode_kernels_refuse_bad_arguments(ops):
    x = torch.zeros(4, dtype=torch.float64, device=DEV)
    D = torch.zeros(4, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError):
        ops.ode_xhat(x, None, float('nan'), 0.0)
    with pytest.raises(RuntimeError):
        ops.ode_xhat(x, None, 1.0, 0.0, 0.0)                           # x_in over s = 0
    with pytest.raises(RuntimeError):
        ops.ode_slope(x, D, 1.0, float('inf'), 0.1)
    with pytest.raises(RuntimeError):
        ops.ode_correct(x, x, D, x, 1.0, 1.0, float('nan'), 0.5, 0.5)
    with pytest.raises(ValueError):
        ops.ode_slope(x, D.double(), 1.0, 1.0, 0.1)


# ---- samplers ------------------------------------------------------------------------------------------------------------------------------
CASES = ('vp_euler', 've_euler', 'iddpm_heun', 'vp_heun_churn', 've_heun_vpdisc', 'edm_ablation_defaults', 'edm_sampler')
SEEDS = [3, 4, 5]
_NETS = {}


def _net(kind, dtype):
    from diffusion_tts_amd.networks import EDMPrecond
    if (kind, dtype) not in _NETS:
        if kind == 'edm':
            with open(os.path.join(GOLDEN, 'manifest.json')) as f:
                cfg, sd = tiny_edm(json.load(f), 'ddpmpp_tiny')
        else:
            cfg, sd = ph.tiny_weights(ph.manifest(), kind)
        _NETS[(kind, dtype)] = EDMPrecond(cfg, sd, device=DEV, dtype=dtype)
    return _NETS[(kind, dtype)]


def _sample(case, net, seeds, num_steps):
    from diffusion_tts_amd import bulk, plain
    rnd, latents, labels = bulk.batch_inputs(seeds, net)
    fn = plain.edm_sampler if case['sampler'] == 'edm' else plain.ablation_sampler
    rows0 = net.evals
    x = fn(net, latents, labels, randn_like=rnd.randn_like, num_steps=num_steps, **case['kwargs'])
    assert x.dtype == torch.float64 and x.is_cuda and x.shape == latents.shape
    return x, latents, labels, net.evals - rows0


def image_ok(img_hwc, ref):
    diff = np.abs(img_hwc.astype(np.int32) - ref.astype(np.int32))
    return diff.max() <= 1 and (diff > 0).mean() < 0.005            # test_gpu_precond.py::image_ok


@pytest.mark.parametrize('dtype', [X3, torch.float32])
@pytest.mark.parametrize('name', CASES)
def test_samplers_match_the_reference_runs(ops, gold, man, name, dtype):
    """The reference's own ablation_sampler / edm_sampler run on the CPU (3 rows, seeds 3, 4, 5 through per-row generators, 8 steps).  Inputs
    equal bit for bit; max|x - x64| / max|x64| <= max(3e-6, 4 x the reference's own float32 distance to its float64 run): the standing factor 4
    and the floor of test_gpu_precond.py; the rows through the denoiser equal the reference's (3 x 8 Euler, 3 x 15 Heun); the uint8 image
    within one level on less than 0.5 % of the pixels."""
    case = man['cases'][name]
    net = _net(case['net'], dtype)
    x, latents, labels, rows = _sample(case, net, SEEDS, man['num_steps'])
    assert np.array_equal(latents.numpy(), gold['latents']) and np.array_equal(labels.argmax(1).numpy(), gold['label_idx'])
    x64 = torch.from_numpy(gold[f'{name}_x64'])
    scale = float(x64.abs().max())
    err = float((x.cpu() - x64).abs().max()) / scale
    bound = max(3e-6, 4 * case['ref_f32_vs_f64'])
    e_ref = float((x.cpu() - torch.from_numpy(gold[f'{name}_x'])).abs().max()) / scale
    print(f'{name} {dtype}: err vs float64 {err:.3e} = {err / case["ref_f32_vs_f64"]:.2f} x the reference\'s own {case["ref_f32_vs_f64"]:.3e} '
          f'(bound {bound:.3e}); vs the reference\'s float32 run {e_ref:.3e}; rows {rows}')
    assert err <= bound, (name, err, bound)
    assert rows == case['net_rows'] == 3 * (8 if case['kwargs'].get('solver') == 'euler' else 15)
    img = ops.quantize_u8(x).permute(0, 2, 3, 1).cpu().numpy()
    assert image_ok(img, gold[f'{name}_image'])


@pytest.mark.parametrize('name', ['vp_heun_churn', 'edm_sampler'])
def test_a_row_does_not_depend_on_its_batch(man, gold, name):
    """seed 4 alone and as the middle row of [3, 4, 5]: the same per-row noise, so the two agree within the bound of the case (not bit for bit:
    the launch forms of the convolutions differ with the batch size)"""
    case = man['cases'][name]
    net = _net(case['net'], X3)
    x3, _, _, _ = _sample(case, net, SEEDS, man['num_steps'])
    x1, _, _, rows = _sample(case, net, [4], man['num_steps'])
    scale = float(torch.from_numpy(gold[f'{name}_x64']).abs().max())
    err = float((x1[0] - x3[1]).abs().max()) / scale
    bound = max(3e-6, 4 * case['ref_f32_vs_f64'])
    print(f'{name}: seed 4 alone vs in a batch of 3: {err:.3e} (bound {bound:.3e})')
    assert rows == 15 and err <= bound and float((x1[0] - x3[0]).abs().max()) / scale > 1e-2      # and it IS row 1, not row 0


def test_deterministic_steps_upload_no_noise(man, monkeypatch):
    """without churn every noise coefficient is zero: the draws are still made (the stream stays the reference's) but dts_ode_xhat is given no noise"""
    from diffusion_tts_amd import ops as o
    seen = []
    real = o.ode_xhat
    monkeypatch.setattr(o, 'ode_xhat', lambda x, eps, *a: (seen.append(eps), real(x, eps, *a))[1])
    case = man['cases']['ve_euler']
    draws = []
    from diffusion_tts_amd import bulk, plain
    net = _net('ve', X3)
    rnd, latents, labels = bulk.batch_inputs(SEEDS, net)
    plain.ablation_sampler(net, latents, labels, randn_like=lambda x: (draws.append(1), rnd.randn_like(x))[1], num_steps=man['num_steps'],
                           **case['kwargs'])
    assert len(draws) == man['num_steps'] == len(seen) and all(e is None for e in seen)


def test_generate_images_writes_what_the_sampler_gives(ops, man, tmp_path):
    """5 seeds in batches of at most 2 (tensor_split: 2, 2, 1): five PNGs, each the quantised row of the batched sampler call on its batch"""
    import PIL.Image
    from diffusion_tts_amd import bulk, plain
    case = man['cases']['vp_euler']
    net = _net('vp', X3)
    seeds = [11, 12, 13, 1014, 15]
    rows0 = net.evals
    done = bulk.generate_images(net, seeds, str(tmp_path), max_batch_size=2, num_steps=4, class_idx=7, **case['kwargs'])
    assert sorted(done) == sorted(seeds) and net.evals - rows0 == 5 * 4
    assert sorted(os.listdir(tmp_path)) == sorted(f'{s:06d}.png' for s in seeds)
    for batch in bulk.rank_batches(seeds, 2, 0, 1):
        b = batch.tolist()
        rnd, latents, labels = bulk.batch_inputs(b, net, class_idx=7)
        assert labels.argmax(1).tolist() == [7] * len(b)
        img = ops.quantize_u8(plain.ablation_sampler(net, latents, labels, randn_like=rnd.randn_like, num_steps=4, **case['kwargs'])).cpu()
        for seed, ref in zip(b, img):
            png = np.array(PIL.Image.open(tmp_path / f'{seed:06d}.png'))
            # the file holds the pixels of the sampler call that wrote it; a second call on the same batch (eager launches against the
            # replayed graph) gives the same image within the one level the samplers are held to
            assert png.shape == (16, 16, 3) and np.array_equal(png, done[seed].permute(1, 2, 0).numpy())
            assert image_ok(png, ref.permute(1, 2, 0).numpy())
