"""Pins tests/elementwise_reference.py on the CPU, in two ways.

Honesty: a numpy model that follows each kernel's own order of operations (float32 or float64, the block reductions lane by lane) stays
inside the reference's bound on the very inputs tests/test_gpu_elementwise.py gives the kernels -- so a bound is not something only an
exact computation could meet.  The quantiser's witness sets are counted and torch's own two-step expression is shown to equal the model.

Teeth: each plausible mistake, applied to the model, leaves the bound (or breaks the equality) on at least one element -- so a bound is
not so wide that it would let the mistake through.  Every test prints its counts; run with -s to see them.

No kernel of csrc/elementwise.hip forms a variance, so there is no E[x^2] - m^2 shortcut to exclude here; the shortcut of the same kind
that IS available -- the brightness mean accumulated in float32 instead of float64 -- is excluded at the 512 x 512 image.
"""
import numpy as np
import pytest
import torch

import elementwise_reference as R


def inside(got, ref, bound):
    ratio, _ = R.worst(got, ref, bound)
    return ratio


def outside_count(got, ref, bound):
    err = (got.double() - ref).abs()
    return int((~(err <= bound)).sum())


# ---- quantiser -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_quantiser_witnesses_edges_and_the_fused_mistake(dtype):
    w = R.quantize_witnesses(dtype)
    two = R.quantize_two_step(w)
    levels = len(set(two.tolist()))
    fused = torch.from_numpy(R.quantize_model(w.numpy(), fused=True))
    print(f'quantiser {dtype}: {len(w)} witnesses on {levels} distinct levels; fused differs on {int((fused != two).sum())}, by at most '
          f'{int((fused.int() - two.int()).abs().max())} level')
    assert len(w) >= 100 and levels >= 100
    assert torch.equal(two, torch.from_numpy(R.quantize_model(w.numpy())))                # torch's two-step expression == the model
    assert bool((fused != two).all()) and int((fused.int() - two.int()).abs().max()) == 1  # the fused form is caught on every one
    for x in (R.quantize_edges(dtype), R.quantize_random(dtype)):
        assert not torch.isnan(x).any()
        assert torch.equal(R.quantize_two_step(x), torch.from_numpy(R.quantize_model(x.numpy())))
    e = R.quantize_edges(dtype)
    q = R.quantize_two_step(e)
    assert int(q.min()) == 0 and int(q.max()) == 255 and len(set(q.tolist())) == 256      # every level is reached
    r = R.quantize_random(dtype)
    n_fused = int((torch.from_numpy(R.quantize_model(r[:65536].numpy(), fused=True)) != R.quantize_two_step(r[:65536])).sum())
    print(f'  random values: the fused form differs on {n_fused} of 65536 -- why random inputs alone do not see it')


def test_float32_input_through_the_float64_kernel_is_exact_either_way():
    """quantize_kernel<float> widens first: the float64 product of a float32 value and 127.5 is exact, so fused and two-step agree"""
    x = torch.cat([R.quantize_witnesses(torch.float32), R.quantize_edges(torch.float32)]).double()
    assert np.array_equal(R.quantize_model(x.numpy(), fused=True), R.quantize_model(x.numpy()))


# ---- brightness ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [1, 255, 256, 257, 4096, 512 * 512])
def test_brightness_model_and_mistakes(hw):
    n = 1 if hw == 512 * 512 else 5
    img = R.brightness_images(hw, n)
    ref, bound = R.brightness_ref(img)
    ratio = inside(R.brightness_model(img), ref, bound)
    missed = [outside_count(R.brightness_model(img, drop_partial=p), ref, bound) for p in range(4)]
    print(f'brightness hw={hw}: model err/bound {ratio:.3f}; a dropped wave partial leaves the bound on {missed} of {n} images')
    assert ratio <= 1.0
    assert all(m > 0 for m in (missed if hw >= 256 else missed[:1]))       # (hw < 256: the later waves hold no pixel)
    if hw == 512 * 512:
        f32 = outside_count(R.brightness_model(img, f32_accumulate=True), ref, bound)
        print(f'  float32 accumulation of the mean: outside on {f32} of {n}')
        assert f32 > 0
    for value in (0, 255):
        flat = torch.full((2, 3, 4, hw // 4 if hw % 4 == 0 else hw), value, dtype=torch.uint8)[:, :, :4 if hw % 4 == 0 else 1]
        ref, bound = R.brightness_ref(flat)
        got = R.brightness_model(flat)
        assert inside(got, ref, bound) <= 1.0 and float(got.max()) <= 1.0 and (value or float(got.abs().max()) == 0.0)


# ---- softmax_gather --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1001])
def test_softmax_model_and_mistakes(k):
    x, tgt = R.softmax_cases(k)
    ref, bound = R.softmax_gather_ref(x, tgt)
    ratio = inside(R.softmax_gather_model(x, tgt), ref, bound)
    nomax = outside_count(R.softmax_gather_model(x, tgt, subtract_max=False), ref, bound)
    off = outside_count(R.softmax_gather_model(x, (tgt + 1) % k), ref, bound) if k > 1 else None
    print(f'softmax k={k}: model err/bound {ratio:.3f}; without the max {nomax} of 8 rows outside; target off by one: {off}')
    assert ratio <= 1.0 and bool(torch.isfinite(ref).all())
    assert float(ref[5]) == 1.0                                            # the row whose other logits are -inf
    if k > 1:
        assert float(ref[6]) < 1e-30 and nomax > 0 and off > 0


# ---- cosine_rows -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('one', [True, False])
@pytest.mark.parametrize('d', [1, 63, 64, 65, 512, 768, 1024])
def test_cosine_model_and_mistakes(d, one):
    a, b = R.cosine_cases(d, one)
    ref, bound = R.cosine_rows_ref(a, b)
    ratio = inside(R.cosine_rows_model(a, b), ref, bound)
    assert ratio <= 1.0
    assert abs(float(ref[1]) - 1) < 1e-6 and abs(float(ref[2]) + 1) < 1e-6 and (d == 1 or abs(float(ref[3])) < 1e-6)
    msg = f'cosine d={d} b_rows={1 if one else 8}: model err/bound {ratio:.3f}'
    if not one:                                                            # the mistake: every row against b's row 0
        wrong = outside_count(R.cosine_rows_model(a, b[:1]), ref, bound)
        msg += f'; b row 0 for every row: {wrong} of 8 outside'
        assert wrong > 0
    if d > 64:                                                             # the mistake: the last ragged trip of the d loop dropped
        cut = (d - 1) // 64 * 64
        wrong = outside_count(R.cosine_rows_model(a[:, :cut], b[:, :cut]), ref, bound)
        msg += f'; last trip dropped: {wrong} of 8 outside'
        assert wrong > 0
    print(msg)


# ---- linear ----------------------------------------------------------------------------------------------------------------------------------
LINEAR_K = [1, 3, 4, 63, 64, 65, 102, 256, 260, 1000, 1028]


@pytest.mark.parametrize('k', LINEAR_K)
def test_linear_model_and_mistakes(k):
    worst_ratio, dropped = 0.0, {}
    for m, n in ((1, 1), (7, 3), (8, 4), (9, 5), (17, 37)):
        for act_in, act_out in ((False, False), (True, False), (False, True), (True, True)):
            x, w, bias, prior = R.linear_inputs(m, n, k, act_in or act_out)
            for with_bias, acc in ((True, False), (False, True)):
                kw = dict(bias=bias if with_bias else None, prior=prior if acc else None, act_in=act_in, act_out=act_out)
                ref, bound = R.linear_ref(x, w, **kw)
                for vector in ((False, True) if k % 4 == 0 else (False,)):
                    worst_ratio = max(worst_ratio, inside(R.linear_model(x, w, vector=vector, **kw), ref, bound))
                    per = 256 if vector else 64
                    if k % per and not (act_in or act_out):
                        dropped[vector] = dropped.get(vector, 0) + (outside_count(R.linear_model(x, w, vector=vector, drop_ragged_trip=True, **kw), ref, bound) > 0)
    print(f'linear k={k}: model err/bound {worst_ratio:.3f}; cases in which a dropped ragged trip leaves the bound: {dropped} of 10 each')
    assert worst_ratio <= 1.0
    assert all(v == 10 for v in dropped.values()) and (dropped or k % 256 == 0)


# ---- pos_embedding ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('swap', [False, True])
@pytest.mark.parametrize('half', [1, 32, 96])
def test_pos_embedding_model_and_mistakes(half, swap):
    v, f = torch.tensor(R.POS_VALUES, dtype=torch.float32), R.pos_freqs(half)
    ref, bound = R.pos_embedding_ref(v, f, swap)
    ratio = inside(R.pos_embedding_model(v, f, swap), ref, bound)
    layout = outside_count(R.pos_embedding_model(v, f, not swap), ref, bound)
    f64 = outside_count(R.pos_embedding_model(v, f, swap, f64_product=True), ref, bound)
    print(f'pos_embedding half={half} swap={swap}: model err/bound {ratio:.3f}; other layout: {layout} outside; float64 product: {f64} outside')
    assert ratio <= 1.0 and layout > 0 and (f64 > 0 or half == 1)         # (half = 1: the only frequency is 1, the product is exact)
    assert tuple(ref.shape) == (len(R.POS_VALUES), 2 * half)


# ---- EDM preconditioning ---------------------------------------------------------------------------------------------------------------------
def test_precond_models_and_mistakes():
    worst_ratio, caught = 0.0, 0
    cases = list(R.precond_cases())
    for x, sig, F in cases:
        (xin, bxin), (coef, bcoef) = R.precond_in_ref(x, sig, 0.5)
        mx, mc = R.precond_in_model(x, sig, 0.5)
        D, bD = R.precond_out_ref(x, F, mc)
        worst_ratio = max(worst_ratio, inside(mx, xin, bxin), inside(mc, coef, bcoef), inside(R.precond_out_model(x, F, mc), D, bD))
        if sig.numel() > 1:                                                # the mistake: sigma[0] for every row
            caught += outside_count(R.precond_in_model(x, sig[:1], 0.5)[0], xin, bxin) > 0
        # the mistake: c_skip and c_out swapped
        assert outside_count(R.precond_out_model(x, F, mc[:, [1, 0, 2, 3]]), D, bD) > 0
    many = sum(1 for c in cases if c[1].numel() > 1)
    print(f'precond: {len(cases)} cases, model err/bound {worst_ratio:.3f}; sigma[0] for every row caught in {caught} of {many}')
    assert worst_ratio <= 1.0 and caught == many


# ---- Heun ------------------------------------------------------------------------------------------------------------------------------------
def test_heun_references_and_the_row_map():
    t = R.sigma_schedule()
    worst_ratio, caught, ambiguous = 0.0, 0, 0
    for x, eps, nb, interleave, i in R.heun_cases():
        t_hat, coef = R.churned(float(t[i]))
        t_next = float(t[i + 1])
        ref, bound = R.heun_xhat_ref(x, eps, coef, nb, interleave)
        fma = torch.from_numpy(np.asarray(x[R.row_map(nb, x.shape[0], interleave)].numpy().astype(np.longdouble)
                                          + np.longdouble(coef) * eps.double().numpy().astype(np.longdouble), dtype=np.float64))   # one rounding
        worst_ratio = max(worst_ratio, inside(fma, ref, bound))
        wrong, _ = R.heun_xhat_ref(x, eps, coef, nb, interleave, wrong_map=True)
        if torch.equal(R.row_map(nb, x.shape[0], interleave), R.row_map(nb, x.shape[0], interleave, True)):
            ambiguous += 1                                                 # xb == 1 or xb == nb: the two orders coincide
        else:
            caught += outside_count(wrong, ref, bound) > 0
        D = (ref.float() * 0.3 + 0.1)
        (d, bd), (xn, bxn) = R.heun_euler_ref(ref, D, t_hat, t_next)
        dl = (ref.numpy().astype(np.longdouble) - D.double().numpy()) / np.longdouble(t_hat)
        xl = ref.numpy() + (np.longdouble(t_next) - np.longdouble(t_hat)) * dl
        worst_ratio = max(worst_ratio, inside(torch.from_numpy(dl.astype(np.float64)), d, bd), inside(torch.from_numpy(xl.astype(np.float64)), xn, bxn))
        if i < 17:
            D2 = (xn.float() * 0.3 + 0.1)
            out, bo = R.heun_correct_ref(ref, D2, d, t_hat, t_next, xn)
            ol = ref.numpy() + (np.longdouble(t_next) - np.longdouble(t_hat)) * (0.5 * d.numpy().astype(np.longdouble) + 0.5 * (xn.numpy().astype(np.longdouble) - D2.double().numpy()) / np.longdouble(t_next))
            worst_ratio = max(worst_ratio, inside(torch.from_numpy(ol.astype(np.float64)), out, bo))
            # the mistake: the Euler slope alone (no 0.5 / 0.5 average)
            assert outside_count(xn, out, bo) > 0
    print(f'heun: extended-precision (fused-like) evaluation err/bound {worst_ratio:.3f}; wrong row order caught in {caught} cases, {ambiguous} where both orders coincide')
    assert worst_ratio <= 1.0 and caught >= 6


# ---- candidate_noise ---------------------------------------------------------------------------------------------------------------------------
def test_candidate_noise_model_and_mistakes():
    worst_ratio, caught, n_mode1 = 0.0, 0, 0
    for pivot, g_, mode, scale in R.candidate_cases():
        ref, bound = R.candidate_noise_ref(pivot, g_, mode, scale)
        worst_ratio = max(worst_ratio, inside(R.candidate_noise_model(pivot, g_, mode, scale), ref, bound))
        b = pivot.shape[0]
        keep = (mode == 0).repeat_interleave(b)
        assert torch.equal(ref[keep], g_[keep])
        if int((mode == 1).sum()) and pivot.shape[1] >= 256:               # the mistake: a wave partial missing from the norm
            n_mode1 += 1
            caught += outside_count(R.candidate_noise_model(pivot, g_, mode, scale, drop_partial=3), ref, bound) > 0
    print(f'candidate_noise: model err/bound {worst_ratio:.3f}; norm missing a wave partial caught in {caught} of {n_mode1} cases')
    assert worst_ratio <= 1.0 and caught == n_mode1 > 0


# ---- DDIM, CFG -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', R.STORAGE)
def test_ddim_and_cfg_models_and_mistakes(dtype):
    worst_ratio, caught, cases = 0.0, 0, 0
    for x, e, z, at, ap, st, _ in R.ddim_cases(dtype):
        (prev, bprev), (x0, bx0) = R.ddim_ref(x, e, z, at, ap, st)
        mp, m0 = R.ddim_model(x, e, z, at, ap, st, dtype)
        worst_ratio = max(worst_ratio, inside(mp, prev, R.rounded_bound(prev, bprev, dtype)), inside(m0, x0, R.rounded_bound(x0, bx0, dtype)))
        # the mistake: base formed from alpha_t's coefficient (sp <- sa)
        wp, _ = R.ddim_model(x, e, z, at, at, st, dtype)
        cases += 1
        caught += outside_count(wp, prev, R.rounded_bound(prev, bprev, dtype)) > 0
    for u, c in R.cfg_cases(dtype):
        for gd in R.GUIDANCE:
            ref, bound = R.cfg_ref(u, c, gd)
            got = R.cfg_model(u, c, gd, dtype)
            worst_ratio = max(worst_ratio, inside(got, ref, R.rounded_bound(ref, bound, dtype)))
            if gd == 0.0:
                assert torch.equal(got, u)
            else:                                                          # the mistake: cond and uncond swapped
                assert outside_count(R.cfg_model(c, u, gd, dtype), ref, R.rounded_bound(ref, bound, dtype)) > 0 or gd == 1.0 and u.numel() == 1
    print(f'ddim / cfg {dtype}: model err/bound {worst_ratio:.3f}; wrong alpha for the base caught in {caught} of {cases} cases')
    assert worst_ratio <= 1.0 and caught == cases


# ---- attention-pool tokens ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', R.STORAGE)
def test_attnpool_model_and_mistakes(dtype):
    worst_ratio, caught, cases = 0.0, 0, 0
    for x, pos in R.attnpool_cases(dtype):
        ref, bound = R.attnpool_tokens_ref(x, pos)
        got = R.attnpool_tokens_model(x, pos, dtype)
        worst_ratio = max(worst_ratio, inside(got, ref, R.rounded_bound(ref, bound, dtype)))
        wrong, _ = R.attnpool_tokens_ref(x, pos, cls_shift=1)               # the mistake: pos one token off
        cases += 1
        caught += outside_count(wrong, ref, R.rounded_bound(ref, bound, dtype)) > 0
        # the mistake: the class token's mean taken over hw + 1
        w2 = ref.clone()
        w2[:, 0] = x.double().sum(1) / (x.shape[1] + 1) + pos.double()[:, 0]
        assert outside_count(w2, ref, R.rounded_bound(ref, bound, dtype)) > 0
    print(f'attnpool_tokens {dtype}: model err/bound {worst_ratio:.3f}; pos off by one token caught in {caught} of {cases} cases')
    assert worst_ratio <= 1.0 and caught == cases


# ---- layout ----------------------------------------------------------------------------------------------------------------------------------
def test_layout_references_are_index_arithmetic():
    x = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).view(2, 3, 5, 7)
    y = R.nchw_to_nhwc_ref(x, torch.float32, cpad=8)
    assert tuple(y.shape) == (2, 5, 7, 8) and float(y[1, 4, 6, 2]) == float(x[1, 2, 4, 6]) and not y[..., 3:].any()
    w = torch.arange(4 * 3 * 2 * 2, dtype=torch.float32).view(4, 3, 2, 2)
    p = R.pack_conv_weight_ref(w, torch.float32, torch.tensor([2, 0, 3, 1], dtype=torch.int32))
    assert tuple(p.shape) == (4, 2, 2, 3) and float(p[0, 1, 0, 2]) == float(w[2, 2, 1, 0])
    assert R.WRAP > 2048 * 256 and R.WRAP % 256
