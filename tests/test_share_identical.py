"""No GPU: which sigma steps `generate_image_grid(share_identical=True)` shares, and how many denoiser rows that saves.

`sampler.identical_steps` lists the sigma steps whose noise coefficient -- what `_Loop.churn` hands to ops.heun_xhat -- is exactly 0.0: there
x_hat = x_cur + 0 * eps, so all candidates of an image are one row.  `sampler.shared_rows_saved` is the closed count of the rows an
eps-greedy / zero-order search then does not launch.  The schedule is the EDM one (edm/main.py:78-80)."""
import inspect

import torch

from diffusion_tts_amd import sampler as sm

CLI = dict(S_churn=40, S_min=0.05, S_max=50, S_noise=1.003)                      # main.py's churn settings


def identity(t):
    return torch.as_tensor(t)


def schedule(num_steps=18, sigma_min=0.002, sigma_max=80, rho=7, round_sigma=identity):
    i = torch.arange(num_steps, dtype=torch.float64)
    t = (sigma_max ** (1 / rho) + i / (num_steps - 1) * (sigma_min ** (1 / rho) - sigma_max ** (1 / rho))) ** rho
    return torch.cat([round_sigma(t), torch.zeros_like(t[:1])])


def steps(t, n, round_sigma=identity, **churn):
    c = dict(CLI, **churn)
    return sm.identical_steps(t, n, c['S_churn'], c['S_min'], c['S_max'], c['S_noise'], round_sigma)


def test_cli_settings_share_the_steps_outside_the_churn_window():
    t = schedule()
    assert float(t[1]) > 50 > float(t[2]) and float(t[14]) > 0.05 > float(t[15])    # sigma 80 and 57.6 above S_max; 0.0229, 0.00753, 0.002 below S_min
    assert steps(t, 18) == [0, 1, 15, 16, 17]
    assert steps(schedule(4), 4) == [0, 3]                                          # the settings of the GPU tests: 80 and 0.002


def test_without_churn_every_step_is_shared_and_with_an_open_window_none():
    t = schedule()
    assert steps(t, 18, S_churn=0) == list(range(18))
    assert sm.identical_steps(t, 18, 0, 0, float('inf'), 1, identity) == list(range(18))      # generate_image_grid's defaults
    assert steps(t, 18, S_min=0, S_max=float('inf')) == []
    assert steps(t, 18, S_noise=0) == list(range(18))                                # the coefficient decides: no noise is added at all


def test_the_rule_is_the_coefficient_not_gamma():
    """a round_sigma that moves ONE level off the schedule adds noise there without churn (t_hat > t_cur): that step is not shared.  One that
    moves a level down makes the coefficient NaN, as the step itself would see it: not shared either."""
    t = schedule()

    def moves(level, factor):
        def round_sigma(s):
            s = torch.as_tensor(s)
            return s * factor if float(s) == float(level) else s
        return round_sigma
    assert steps(t, 18, moves(t[16], 1.01)) == [0, 1, 15, 17]
    assert steps(t, 18, moves(t[0], 1.01), S_churn=0) == list(range(1, 18))
    assert steps(t, 18, moves(t[15], 0.99)) == [0, 1, 16, 17]
    # and a round_sigma that takes a churned t_hat BACK to t_cur removes the noise of a step inside the window
    back = {float(t[5] + min(40 / 18, 2 ** 0.5 - 1) * t[5]): t[5]}
    assert steps(t, 18, lambda s: back.get(float(s), torch.as_tensor(s))) == [0, 1, 5, 15, 16, 17]


def test_identical_steps_is_what_the_loop_computes():
    """the loop's own churn() and identical_steps are one function: coefficient 0.0 exactly at the listed steps"""
    class Net:
        round_sigma = staticmethod(identity)
    t = schedule()
    L = sm._Loop(Net(), 'cpu', 18, 40, 0.05, 50, 1.003, None, None)
    zero = [i for i in range(18) if L.churn(t[i])[1] == 0.0]
    assert zero == steps(t, 18) and L.shared == frozenset()
    assert L.churn(t[3]) == sm.churn_of(t[3], 18, 40, 0.05, 50, 1.003, identity) and L.churn(t[3])[1] > 0


def test_saved_rows_of_the_headline_search():
    shared = steps(schedule(), 18)
    assert sm.shared_rows_saved(shared, 18, N=64, K=4, B=1) == 4 * 64 * (2 * 4 + 1) == 2304
    assert 8995 - sm.shared_rows_saved(shared, 18, N=64, K=4) == 6691
    assert sm.shared_rows_saved([0, 3], 4, N=3, K=2, B=4) == 2 * 3 * 4 * (2 + 1)
    assert sm.shared_rows_saved([], 18, N=64, K=4) == 0
    assert sm.shared_rows_saved(range(18), 18, N=64, K=4) == 4 * 64 * 35          # S_churn = 0: only the 35 pivot rows are left


def test_the_keyword_is_keyword_only_and_off_by_default():
    par = inspect.signature(sm.generate_image_grid).parameters['share_identical']
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is False


def test_main_flag():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('dts_main_cli', os.path.join(root, 'main.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = mod.build_parser()
    need = ['--backend', 'edm', '--scorer', 'brightness']
    assert parser.parse_args(need).share_identical is False
    assert parser.parse_args(need + ['--share-identical']).share_identical is True
