"""CPU: the host side of the plain samplers (diffusion_tts_amd/plain.py, bulk.generate_images) -- the schedule and the per-step scalars against
the reference's own values (tests/golden/make_golden_ablation.py), the float64 restatements of the three ODE step kernels
(tests/ablation_reference.py), the refusals, the per-row generators and the batching of the bulk generator."""
import json
import os

import numpy as np
import pytest
import torch

import ablation_reference as ar
import precond_helpers as ph

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KEYS = ('t_hat', 'sigma_hat', 'ratio', 'noise_coef', 'a', 'b', 'h')


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLDEN, 'ablation_golden.npz'))


@pytest.fixture(scope='module')
def man():
    with open(os.path.join(GOLDEN, 'ablation_manifest.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def table():
    return ph.golden()['iddpm_u']


class StubNet:
    """what ode_schedule needs of a network: its range and round_sigma (an iDDPM network's: the nearest entry of its float32 table)"""

    def __init__(self, sigma_min=0.0, sigma_max=float('inf'), table=None):
        self.sigma_min, self.sigma_max = sigma_min, sigma_max
        self.u = None if table is None else torch.from_numpy(np.asarray(table, dtype=np.float32))

    def round_sigma(self, sigma):
        sigma = torch.as_tensor(sigma)
        if self.u is None:
            return sigma
        idx = (sigma.to(torch.float32).reshape(-1, 1) - self.u.reshape(1, -1)).abs().argmin(1)
        return self.u[idx].to(sigma.dtype).reshape(sigma.shape)


def stub_for(case, table):
    return StubNet(case['sigma_min'], case['sigma_max'], table if case['net'] == 'iddpm' else None)


def schedule_kwargs(case):
    kw = dict(case['kwargs'])
    if case['sampler'] == 'edm':                                    # edm_sampler: the ablation sampler's defaults with its own fixed range
        kw.update(sigma_min=0.002, sigma_max=80)
    return kw


def written_out(num_steps, sigma_min, sigma_max, rho):
    """the EDM discretisation as the reference writes it (edm/main.py:78-79, edm/generate.py:38-39)"""
    step_indices = torch.arange(num_steps, dtype=torch.float64)
    return (sigma_max ** (1 / rho) + step_indices / (num_steps - 1) * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho


@pytest.mark.parametrize('num_steps', [2, 4, 18])
def test_edm_sigmas_is_the_written_out_expression_and_each_caller_keeps_its_own_range(num_steps):
    """plain.edm_sigmas bit for bit in float64, for the default range and a clamped one; then the two callers' schedules: equal for a network
    that neither clamps nor rounds, and for the range of the iDDPM ImageNet-64 configuration different in the expected way -- edm_sampler
    (plain.edm_schedule) clamps the range to the network's, generate_image_grid (sampler.grid_schedule) takes it as given"""
    from diffusion_tts_amd import plain, sampler
    from diffusion_tts_amd.config import iddpm_imagenet64
    for lo, hi, rho in ((0.002, 80, 7), (0.0064, 60.5, 7), (0.002, 80, 5)):
        got = plain.edm_sigmas(num_steps, lo, hi, rho)
        assert got.dtype == torch.float64 and torch.equal(got, written_out(num_steps, lo, hi, rho)), (lo, hi, rho)
    free = StubNet()
    grid, plain_ = sampler.grid_schedule(free, num_steps, 0.002, 80, 7), plain.edm_schedule(free, num_steps, 0.002, 80, 7)
    assert torch.equal(grid, plain_) and torch.equal(grid, torch.cat([written_out(num_steps, 0.002, 80, 7), torch.zeros(1, dtype=torch.float64)]))
    cfg = iddpm_imagenet64()
    assert cfg.sigma_min > 0.002 and cfg.sigma_max > 80                               # the low end is cut, the high end is not
    net = StubNet(cfg.sigma_min, cfg.sigma_max)
    grid, plain_ = sampler.grid_schedule(net, num_steps, 0.002, 80, 7), plain.edm_schedule(net, num_steps, 0.002, 80, 7)
    assert torch.equal(grid[:-1], written_out(num_steps, 0.002, 80, 7)) and torch.equal(plain_[:-1], written_out(num_steps, cfg.sigma_min, 80, 7))
    assert float(grid[0]) == float(plain_[0]) and float(grid[num_steps - 1]) < 0.0021 < 0.0064 < float(plain_[num_steps - 1])
    assert float(grid[-1]) == float(plain_[-1]) == 0.0 and not torch.equal(grid, plain_)


SCHED_ARGS = ('sigma_min', 'sigma_max', 'rho', 'discretization', 'schedule', 'scaling', 'epsilon_s', 'C_1', 'C_2', 'M')
STEP_ARGS = ('alpha', 'S_churn', 'S_min', 'S_max', 'S_noise')


def product_scalars(net, num_steps, kw):
    """plain.ode_schedule + plain.ode_step_scalars -> {key: numpy [num_steps]} and t_steps"""
    from diffusion_tts_amd import plain
    sched = plain.ode_schedule(net, num_steps, **{k: v for k, v in kw.items() if k in SCHED_ARGS})
    t_steps = sched[0]
    assert t_steps.dtype == torch.float64 and t_steps.shape == (num_steps + 1,) and float(t_steps[-1]) == 0.0
    rows = [plain.ode_step_scalars(t_steps[i], t_steps[i + 1], sched, net.round_sigma, num_steps, **{k: v for k, v in kw.items() if k in STEP_ARGS})
            for i in range(num_steps)]
    out = {k: np.array([float(r[k]) for r in rows]) for k in KEYS}
    out['t_steps'] = t_steps.numpy()
    return out


def reference_scalars(case, table, num_steps, **mistakes):
    kw = schedule_kwargs(case)
    rs = ar.table_rounding(table) if case['net'] == 'iddpm' else ar.identity
    return ar.schedule_ref(case['sigma_min'], case['sigma_max'], rs, num_steps, **kw, **mistakes)


CASES = ('vp_euler', 've_euler', 'iddpm_heun', 'vp_heun_churn', 've_heun_vpdisc', 'edm_ablation_defaults', 'edm_sampler')


@pytest.mark.parametrize('name', CASES)
def test_schedule_and_step_scalars_match_the_reference(gold, man, table, name):
    """t_steps and, per step, t_hat, sigma(t_hat), ratio, noise_coef, a, b, h of the reference's own run: the four discretisations (vp, ve, iddpm,
    edm) with the schedules and scalings of the golden cases.  The bound is ablation_reference's running error bound (see its docstring:
    one rounding per operation, 4 ulp per library function, first-order propagation, so operation count x conditioning); two hosts'
    evaluations may differ by twice it.  Held by both this build's host code and the restatement the bound belongs to.  The iDDPM network's
    times are entries of its float32 table: equality."""
    case, n = man['cases'][name], man['num_steps']
    ref = reference_scalars(case, table, n)
    got = product_scalars(stub_for(case, table), n, schedule_kwargs(case))
    for key in ('t_steps',) + KEYS:
        g = gold[f'{name}_{key}']
        e_ref, e_got = ar.excess(g, ref[key]), ar.excess(got[key], ref[key])
        rel = float(np.max(ref[key].e / np.maximum(np.abs(ref[key].v), 1e-300)))
        print(f'{name} {key}: golden vs restatement {e_ref:.3f}, this build vs restatement {e_got:.3f} of the allowance '
              f'(largest relative bound {rel:.2e})')
        assert e_ref <= 1 and e_got <= 1, (name, key, e_ref, e_got)
        # the bound is a float64 one, not a licence: at most 1e-8 of the value, except where the expression cancels -- a = sigma'/sigma + s'/s
        # under VP scaling is 1 / (1 + sigma^2) of either term (2e4 at the VP range's upper end), and the noise coefficient may vanish
        assert rel < (1e-5 if key == 'a' else 1e-8) or key == 'noise_coef', (name, key, rel)
    churned = gold[f'{name}_noise_coef'] > 1e-3
    assert churned.sum() == (5 if 'S_churn' in case['kwargs'] else 0)


def test_planted_schedule_mistakes_exceed_the_bound(gold, man, table):
    """epsilon_s 1e-3 -> 1.1e-3 (VP discretisation), round -> floor in the iDDPM index, and the iDDPM recursion without clip(min=C_1) -- that
    one on a range that reaches u[0], the only entry the clip touches (u[0] = 2.03e4: sigma_max = 1e5 on a network without a range of its own;
    the sampler's default range ends at 81, where the clip cannot show)"""
    n = man['num_steps']
    vp = man['cases']['vp_euler']
    wrong = ar.schedule_ref(vp['sigma_min'], vp['sigma_max'], ar.identity, n, **dict(vp['kwargs'], epsilon_s=1.1e-3))
    idd = man['cases']['iddpm_heun']
    floor = reference_scalars(idd, table, n, floor_index=True)
    for what, ref, name in (('epsilon_s', wrong, 'vp_euler'), ('floor', floor, 'iddpm_heun')):
        ex = ar.excess(gold[f'{name}_t_steps'], ref['t_steps'])
        print(f'{what}: {ex:.3e} x the allowance')
        assert ex > 1
    wide = dict(discretization='iddpm', sigma_max=1e5)
    got = product_scalars(StubNet(), n, wide)
    good = ar.schedule_ref(0.0, float('inf'), ar.identity, n, **wide)
    bad = ar.schedule_ref(0.0, float('inf'), ar.identity, n, **wide, drop_clip=True)
    assert got['t_steps'][0] > 1e4                                                 # u[0] is in range
    ex_good, ex_bad = ar.excess(got['t_steps'], good['t_steps']), ar.excess(got['t_steps'], bad['t_steps'])
    print(f'clip(min=C_1): with it {ex_good:.3f}, dropped {ex_bad:.3e} x the allowance')
    assert ex_good <= 1 < ex_bad


# ---- the kernel expressions ------------------------------------------------------------------------------------------------------------
SCALARS = dict(ratio=0.93, coef=0.41, s=0.37, a=-1.7, b=0.37, step=-0.6, h=-0.8, alpha=0.75)


def test_kernel_restatements_hold_their_bounds_and_exclude_the_mistakes():
    """numpy models of the three kernels (each product and sum rounded on its own) against the float64 torch references within 8 e64 x the sum
    of the magnitudes of the terms; x_in equal to (stored x) / s.  The planted mistakes fall outside: a multiplication by 1 / s (only the
    equality sees it: it is one or two roundings off, inside any 8 e64 bound), w0 / w1 swapped at alpha = 0.75, b without its factor s.
    The reciprocal is planted at s = 0.37, where it moves a quarter of the elements.  At s = 0.3 it moves NONE, which is arithmetic and not
    luck: fl(1 / 0.3) is within 7.4e-18 of 1 / fl(0.3), and a 53-bit x over 0.3 is x * 10 / 3 to that accuracy, a sixth of an ulp or more
    from every rounding boundary -- so no test can tell the two forms apart at s = 0.3 (the count is printed and asserted to be zero)."""
    k, d = SCALARS, ar.ode_inputs(771, 5)
    w1 = 1 / (2 * k['alpha'])
    w0 = 1 - w1
    for eps in (d['eps'], d['eps'].float(), None):
        coef = 0.0 if eps is None else k['coef']
        xh, xi = ar.ode_xhat_model(d['x'], eps, k['ratio'], coef, k['s'])
        (r_h, b_h), (r_i, b_i) = ar.ode_xhat_ref(d['x'], eps, k['ratio'], coef, k['s'])
        assert ar.worst(xh, r_h, b_h)[0] <= 1 and ar.worst(xi, r_i, b_i)[0] <= 1 and torch.equal(xi, ar.true_div(xh, k['s']))
        _, xi_bad = ar.ode_xhat_model(d['x'], eps, k['ratio'], coef, k['s'], reciprocal=True)
        off = int((xi_bad != ar.true_div(xh, k['s'])).sum())
        print(f'reciprocal-multiply at s = {k["s"]}: {off} of {xi.numel()} elements differ from the division, worst {ar.worst(xi_bad, r_i, b_i)[0]:.2f} of the 8 e64 bound')
        assert off > 0 and ar.worst(xi_bad, r_i, b_i)[0] <= 1                        # inside the 8 e64 bound: why equality is asked
    _, xi3 = ar.ode_xhat_model(d['x'], d['eps'], k['ratio'], k['coef'], 0.3)
    _, xi3_bad = ar.ode_xhat_model(d['x'], d['eps'], k['ratio'], k['coef'], 0.3, reciprocal=True)
    print(f'reciprocal-multiply at s = 0.3: {int((xi3 != xi3_bad).sum())} elements differ')
    assert torch.equal(xi3, xi3_bad)
    dm, xo, xi = ar.ode_slope_model(d['x'], d['D'], k['a'], k['b'], d['base'], k['step'], k['s'])
    (r_d, b_d), (r_o, b_o), (r_i, b_i) = ar.ode_slope_ref(d['x'], d['D'], k['a'], k['b'], d['base'], k['step'], k['s'])
    assert ar.worst(dm, r_d, b_d)[0] <= 1 and ar.worst(xo, r_o, b_o)[0] <= 1 and ar.worst(xi, r_i, b_i)[0] <= 1 and torch.equal(xi, ar.true_div(xo, k['s']))
    dm_bad, xo_bad, _ = ar.ode_slope_model(d['x'], d['D'], k['a'], k['b'], d['base'], k['step'], k['s'], b_without_s=k['s'])
    assert ar.worst(dm_bad, r_d, b_d)[0] > 1e6 and ar.worst(xo_bad, r_o, b_o)[0] > 1e6
    xn = ar.ode_correct_model(d['base'], d['x'], d['D'], d['d'], k['a'], k['b'], k['h'], w0, w1)
    r_n, b_n = ar.ode_correct_ref(d['base'], d['x'], d['D'], d['d'], k['a'], k['b'], k['h'], w0, w1)
    assert ar.worst(xn, r_n, b_n)[0] <= 1
    xn_bad = ar.ode_correct_model(d['base'], d['x'], d['D'], d['d'], k['a'], k['b'], k['h'], w0, w1, swap_weights=True)
    assert ar.worst(xn_bad, r_n, b_n)[0] > 1e6


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(solver='rk4'), dict(discretization='ddim'), dict(schedule='cosine'), dict(scaling='ve'), dict(solver=None)])
def test_ablation_sampler_refuses_what_the_reference_asserts_on(kw):
    from diffusion_tts_amd import plain
    with pytest.raises(ValueError):
        plain.ablation_sampler(StubNet(), torch.zeros(1, 3, 4, 4), **kw)


def test_ode_xhat_refuses_a_missing_or_a_superfluous_noise():
    from diffusion_tts_amd import ops
    x = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.ode_xhat(x, None, 1.0, 0.5)
    with pytest.raises(ValueError):
        ops.ode_xhat(x, torch.zeros(4, dtype=torch.float64), 1.0, 0.0)
    with pytest.raises(ValueError):
        ops.ode_xhat(x, torch.zeros(4, dtype=torch.float16), 1.0, 0.5)


def test_stacked_generator_rows_are_lone_generators():
    """row i of every stacked draw -- latents, label indices, then two steps' noise, in the generator's order -- equals, bit for bit, what a lone
    generator seeded with seed i draws; a first dimension other than the number of seeds is refused"""
    from diffusion_tts_amd.plain import StackedRandomGenerator
    seeds = [3, 4, 5, (1 << 32) + 4]
    rnd = StackedRandomGenerator(seeds)
    lat = rnd.randn([4, 3, 5, 5], device='cuda')                                    # the device is ignored: host draws
    idx = rnd.randint(10, size=[4], device='cuda')
    x = torch.zeros(4, 3, 5, 5, dtype=torch.float64)
    e1, e2 = rnd.randn_like(x), rnd.randn_like(x)
    assert lat.dtype == torch.float32 and e1.dtype == torch.float64 and not lat.is_cuda and idx.shape == (4,)
    for i, seed in enumerate(seeds):
        g = torch.Generator().manual_seed(seed % (1 << 32))
        assert torch.equal(lat[i], torch.randn([3, 5, 5], generator=g))
        assert torch.equal(idx[i], torch.randint(10, size=[], generator=g))
        assert torch.equal(e1[i], torch.randn([3, 5, 5], generator=g, dtype=torch.float64))
        assert torch.equal(e2[i], torch.randn([3, 5, 5], generator=g, dtype=torch.float64))
    assert torch.equal(lat[1], lat[3])                                             # seeds are taken mod 2^32
    for bad in ([3, 3, 5, 5], [5, 3, 5, 5], []):
        with pytest.raises(ValueError):
            rnd.randn(bad)
    with pytest.raises(ValueError):
        rnd.randint(10, size=[2])


# ---- the bulk generator's batching -----------------------------------------------------------------------------------------------------
class StubDenoiser(StubNet):
    img_channels, img_resolution, label_dim = 3, 4, 0

    def __call__(self, x, sigma, class_labels=None):
        raise AssertionError('the stub sampler does not call the network')


@pytest.mark.parametrize('world', [1, 2, 8])
def test_generate_images_generates_every_seed_once(tmp_path, monkeypatch, world):
    """21 seeds in batches of at most 4 over 1, 2 and 8 ranks with a stub sampler (the quantiser replaced by its two-step torch expression: no
    GPU): one sampler call per non-empty batch, every seed in exactly one of them and written once, its image the one its own generator gives"""
    from diffusion_tts_amd import bulk
    monkeypatch.setattr(bulk.ops, 'quantize_u8', lambda x: (x * 127.5 + 128).clip(0, 255).to(torch.uint8))
    seeds = [7, 1000, 1001] + list(range(20, 38))
    calls, seen = [], []

    def sampler(net, latents, labels, randn_like, num_steps=18):
        assert labels is None and num_steps == 5 and randn_like(latents).shape == latents.shape
        calls.append(latents.shape[0])
        return latents.to(torch.float64)
    for rank in range(world):
        done = bulk.generate_images(StubDenoiser(), seeds, str(tmp_path), max_batch_size=4, subdirs=True, rank=rank, world=world,
                                    sampler_fn=sampler, num_steps=5, sigma_min=None)
        seen += list(done)
        for seed, img in done.items():
            lat = torch.randn([3, 4, 4], generator=torch.Generator().manual_seed(seed))
            assert torch.equal(img, (lat.double() * 127.5 + 128).clip(0, 255).to(torch.uint8))
    assert sorted(seen) == sorted(seeds) and max(calls) <= 4 and sum(calls) == len(seeds)
    files = sorted(os.path.relpath(os.path.join(dp, f), tmp_path) for dp, _, fs in os.walk(tmp_path) for f in fs)
    assert files == sorted(f'{s - s % 1000:06d}/{s:06d}.png' for s in seeds)


def test_one_channel_images_are_written_grey(tmp_path, monkeypatch):
    """a 1-channel network's image is an 8-bit grey PNG (the GPU networks end in a 3-channel convolution, so this path has a stub only)"""
    import PIL.Image
    from diffusion_tts_amd import bulk
    monkeypatch.setattr(bulk.ops, 'quantize_u8', lambda x: (x * 127.5 + 128).clip(0, 255).to(torch.uint8))

    class Grey(StubDenoiser):
        img_channels = 1
    done = bulk.generate_images(Grey(), '5,6', str(tmp_path), max_batch_size=2, sampler_fn=lambda net, lat, lab, randn_like: lat.double())
    for seed in (5, 6):
        png = PIL.Image.open(tmp_path / f'{seed:06d}.png')
        assert png.mode == 'L' and np.array_equal(np.array(png), done[seed][0].numpy())


def test_sampler_choice_follows_the_reference():
    from diffusion_tts_amd import bulk, plain
    assert bulk.pick_sampler(dict(num_steps=18, solver=None, scaling=None)) == (plain.edm_sampler, dict(num_steps=18))
    for key in ('solver', 'discretization', 'schedule', 'scaling'):
        fn, kw = bulk.pick_sampler({key: 'x', 'rho': None})
        assert fn is plain.ablation_sampler and kw == {key: 'x'}
