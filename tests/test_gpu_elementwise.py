"""GPU: every kernel of csrc/elementwise.hip that turns a network output into the next sampler state, an 8-bit image or a reward, against an
exact or float64 reference of the same operation computed on the CPU from the SAME rounded inputs (tests/elementwise_reference.py, pinned
by tests/test_elementwise_reference.py).  The bounds below were written from the number formats and the kernels' documented order of
operations before the kernels first ran under them; they are per element, scaled by the sum of the absolute terms that meet in that
element (never by the tensor's maximum), and are not fitted to what the GPU returns.  Every test prints its worst err / bound.

Notation: u = 2^-8 (bfloat16) / 2^-11 (float16) / 0 (float32 storage), e32 = 2^-24, e64 = 2^-53, 1 ulp = 2 e32.  Device-library accuracy:
the ROCm device-library documentation is not installed with the toolchain, so the OpenCL 3.0 full-profile figures are used (as the GEGLU
test does for erfc): expf 3 ulp, logf 3 ulp, sinf / cosf 4 ulp, sqrtf 3 ulp, division 2.5 ulp; __expf(x) = v_exp_f32(x log2 e): 2^-22 +
|x| 2^-23 relative.  A block of B threads reduces L terms within (ceil(L / B) + 9) e relative to sum |terms| (one wave: ceil(L / 64) + 6).

  quantize_u8          EQUAL to torch's two-step (x * 127.5 + 128).clip(0, 255).to(uint8) on the CPU in the arithmetic type: float64 for a
                       float64 input and for a float32 input widened first; float32 for f32_math.  Includes the inputs on which a fused
                       multiply-add truncates to another byte (126 float32, 115 float64 witnesses, one per level).
  u8_to_unit_f32       EQUAL to x.float() / 255 (IEEE float32 division on both sides).
  brightness           (6 e32 + (hw / 256 + 10) e64) m: five float32 roundings of positive terms per pixel, the float64 pixel sum, one
                       rounding of the mean; all-zero image exactly 0; never above 1.
  softmax_gather       p [(6 + |d_t|) + sum_j w_j (6 + |d_j|) + ceil(k / 256) + 9 + 5] e32 + 2^-125, d_j = x_j - max: each exponential
                       carries the rounding of its argument and expf's 3 ulp, the denominator the weighted mean of that and the
                       reduction, the division 2.5 ulp; the floor is the flush of an exponential (or result) below 2^-126.
  cosine_rows          [2 dn + 11 e32 + (ceil(d / 64) + 6) e32] sum |a_i b_i| / (|a| |b|), dn = (ceil(d / 64) + 7) e32 / 2 + 3 ulp per norm.
  linear               (ceil(k / 64) + 11) e32 S + 2 e32 (S + |bias| + |prior|), S = sum |x_i w_i|; act_in adds sum silu_rel(x_i) |silu(x_i)
                       w_i|, act_out multiplies by 1.1 (max |silu'|) and adds silu_rel(v) |silu(v)|; silu_rel(x) = 2^-22 + |x| 2^-23 + 6 e32.
  pos_embedding        4 * 2^-23 absolute: sinf / cosf's 4 ulp of a result <= 1; the argument is the float32 product v f on both sides.
  edm_precond_in       c_skip, c_out, c_in within 16 e32, c_noise within logf's 3 ulp, xin within 18 e32 -- all relative, from f32(sigma).
  edm_precond_out      4 e32 (|c_skip x| + |c_out F|) from the float32 coefficients it is given.
  heun_xhat/euler/correct   8 e64 * the terms of each expression (elementwise_reference.heun_*_ref): a fused multiply-add stays far inside.
  candidate_noise      2 e64 |pivot| + (ceil(chw / 256) + 16) e64 |scale g / norm|; mode-0 rows bit-equal to g; scale 0 gives the pivot.
  ddim_candidates      the float32 chain of elementwise_reference.ddim_ref (coefficients within 8 e32, dirc's cancellation, the 1 / sqrt(a_t)
                       amplification of x - sqrt(1 - a_t) e) + u (|out| + that) for the store.
  cfg_combine          3 e32 (|u| + |g (c - u)|) + the store's u; guidance 0 returns uncond bit for bit.
  attnpool_tokens      token 0: (hw + 4) e32 sum |x| / hw + e32 |tok|, others e32 |tok|, + the store's u;  take_token: EQUAL.
  layout, casts        EQUAL to torch permute / index / .to(dtype), each direction on its own.

test_grid_stride_wrap runs every grid-stride kernel once at 524 288 + 257 elements -- one more than the 2048 x 256 threads a launch is
capped at -- against the same references: the second trip of the loop.

Left out because already held exactly elsewhere: resample_u8 and lut_u8_f32 (tests/test_gpu_clip_preprocess_ops.py), candidate_noise_sd
(tests/test_gpu_sd.py), split2_f16 / split3_f16 (tests/test_gpu_resample.py: every finite float16 value and its float32 neighbours
against the bit models of tests/resample_reference.py).
"""
import pytest
import torch

import elementwise_reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


def name(dtype):
    return str(dtype).split('.')[-1]


def check(what, got, ref, bound):
    """prints and asserts the worst err / bound of one comparison; returns it"""
    ratio, err = R.worst(got.cpu(), ref, bound)
    print(f'{what}: max err {err:.3e}, max err/bound {ratio:.3f}')
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0, what
    return ratio


class Worst:
    """collects err / bound over the cases of one test and prints the maximum once"""

    def __init__(self, what):
        self.what, self.ratio, self.err, self.cases = what, 0.0, 0.0, 0

    def add(self, got, ref, bound, case=''):
        ratio, err = R.worst(got.cpu(), ref, bound)
        self.ratio, self.err, self.cases = max(self.ratio, ratio), max(self.err, err), self.cases + 1
        assert bool(torch.isfinite(got).all()) and ratio <= 1.0, f'{self.what} {case}: err/bound {ratio:.3f} (max err {err:.3e})'

    def report(self):
        print(f'{self.what}: {self.cases} cases, max err {self.err:.3e}, worst err/bound {self.ratio:.3f}')


# ---- quantiser -------------------------------------------------------------------------------------------------------------------------------
def _quantize(ops, x, form):
    """the three forms of dts_quantize_u8 and the CPU expression each must equal"""
    if form == 'f64':
        return ops.quantize_u8(x.to(DEV)).cpu(), R.quantize_two_step(x)
    if form == 'f32_widened':
        return ops.quantize_u8(x.to(DEV)).cpu(), R.quantize_two_step(x.double())
    return ops.quantize_u8(x.to(DEV), f32_math=True).cpu(), R.quantize_two_step(x)


@pytest.mark.parametrize('form', ['f64', 'f32_widened', 'f32_math'])
def test_quantize_u8_equals_the_two_step_expression(ops, form):
    dtype = torch.float64 if form == 'f64' else torch.float32
    for what, x in (('witnesses', R.quantize_witnesses(dtype)), ('edges', R.quantize_edges(dtype)), ('random', R.quantize_random(dtype))):
        got, want = _quantize(ops, x.contiguous(), form)
        diff = int((got != want).sum())
        print(f'quantize_u8 {form} {what}: {diff} of {x.numel()} bytes differ' + (f' (first at x = {x[got != want][0].item()!r})' if diff else ''))
        assert got.dtype == torch.uint8 and diff == 0, (form, what)


# ---- u8 -> unit, brightness ------------------------------------------------------------------------------------------------------------------
def test_u8_to_unit_f32_full_ramp(ops):
    ramp = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(ops.u8_to_unit_f32(ramp.to(DEV)).cpu(), R.u8_to_unit_ref(ramp))
    img = R.brightness_images(257, 5)
    assert torch.equal(ops.u8_to_unit_f32(img.to(DEV)).cpu(), R.u8_to_unit_ref(img))
    print('u8_to_unit_f32: equal on the 0..255 ramp and on [5, 3, 1, 257]')


@pytest.mark.parametrize('hw', [1, 255, 256, 257, 4096, 512 * 512])
@pytest.mark.parametrize('n', [1, 5])
def test_brightness(ops, hw, n):
    if n == 5 and hw == 512 * 512:
        n = 2                                        # (the largest image once more with a second row; 5 of them add nothing)
    img = R.brightness_images(hw, n)
    ref, bound = R.brightness_ref(img)
    got = ops.brightness(img.to(DEV))
    check(f'brightness hw={hw} n={n}', got, ref, bound)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    flat = torch.zeros_like(img)
    assert float(ops.brightness(flat.to(DEV)).abs().max()) == 0.0                       # all-0: exactly 0
    flat.fill_(255)
    ref, bound = R.brightness_ref(flat)
    got = ops.brightness(flat.to(DEV))
    check(f'brightness hw={hw} n={n} all-255', got, ref, bound)
    assert float(got.max()) <= 1.0


# ---- softmax_gather, cosine_rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1001])
def test_softmax_gather(ops, k):
    x, tgt = R.softmax_cases(k)
    assert int(tgt.min()) >= 0 and int(tgt.max()) < k                                  # the kernel does not check: never outside the row
    ref, bound = R.softmax_gather_ref(x, tgt)
    got = ops.softmax_gather(x.to(DEV), tgt.to(DEV))
    check(f'softmax_gather k={k}', got, ref, bound)
    assert float(got[5]) == 1.0                                                        # every other logit -inf


@pytest.mark.parametrize('one', [True, False])
@pytest.mark.parametrize('d', [1, 63, 64, 65, 512, 768, 1024])
def test_cosine_rows(ops, d, one):
    a, b = R.cosine_cases(d, one)
    ref, bound = R.cosine_rows_ref(a, b)
    check(f'cosine_rows d={d} b_rows={1 if one else 8}', ops.cosine_rows(a.to(DEV), b.to(DEV)), ref, bound)


# ---- linear ----------------------------------------------------------------------------------------------------------------------------------
def _linear_raw(ops, x, w, bias, out, act_in, act_out, accumulate):
    """dts_linear on a row-strided view of x (ops.linear takes contiguous tensors only)"""
    m, k = x.shape
    assert x.stride(1) == 1 and x.dtype == torch.float32
    ops._call('dts_linear', x.data_ptr(), x.stride(0), w.data_ptr(), None if bias is None else bias.data_ptr(), out.data_ptr(), out.shape[-1],
              m, k, w.shape[0], int(act_in), int(act_out), int(accumulate))
    return out


@pytest.mark.parametrize('k', [1, 3, 4, 63, 64, 65, 102, 256, 260, 1000, 1028])
def test_linear(ops, k):
    ws, reached = Worst(f'linear k={k}'), set()
    for m, n in ((1, 1), (7, 3), (8, 4), (9, 5), (17, 37)):
        for act_in, act_out in ((False, False), (True, False), (False, True), (True, True)):
            x, w, bias, prior = R.linear_inputs(m, n, k, act_in or act_out)
            xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
            for with_bias, acc in ((True, False), (False, True)):
                ref, bound = R.linear_ref(x, w, bias if with_bias else None, prior if acc else None, act_in, act_out)
                out = prior.to(DEV).clone() if acc else None
                got = ops.linear(xd, wd, bd if with_bias else None, act_in=act_in, act_out=act_out, out=out, accumulate=acc)
                reached.add(R.linear_takes_vector_kernel(xd, wd, k))
                ws.add(got, ref, bound, f'm={m} n={n} act=({act_in},{act_out}) bias={with_bias} acc={acc}')
        # row-strided views of a wider buffer: ldx = k + 4 keeps ldx % 4 == k % 4 (16-byte loads where k allows), ldx = k + 3 never does;
        # and x one float off a 16-byte boundary, which forces the scalar kernel at any k
        x, w, bias, prior = R.linear_inputs(m, n, k, False)
        ref, bound = R.linear_ref(x, w, bias)
        wd, bd = w.to(DEV), bias.to(DEV)
        for ldx in (k + 4, k + 3):
            buf = torch.full((m, ldx), 1e30, device=DEV)                                 # anything read beyond column k would show
            buf[:, :k] = x.to(DEV)
            view = buf[:, :k]
            vector = R.linear_takes_vector_kernel(view, wd, k)
            assert vector == (k % 4 == 0 and ldx % 4 == 0)
            reached.add(vector)
            ws.add(_linear_raw(ops, view, wd, bd, torch.empty(m, n, device=DEV), False, False, False), ref, bound, f'm={m} n={n} ldx={ldx}')
        flat = torch.zeros(m * k + 4, device=DEV)
        flat[1:1 + m * k] = x.to(DEV).reshape(-1)
        off = flat[1:1 + m * k].view(m, k)
        assert off.data_ptr() % 16 == 4 and not R.linear_takes_vector_kernel(off, wd, k)
        reached.add(False)
        ws.add(ops.linear(off, wd, bd), ref, bound, f'm={m} n={n} offset by one float')
    ws.report()
    assert reached == ({True, False} if k % 4 == 0 else {False})                       # both kernels where the dispatch condition allows both


# ---- pos_embedding ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('swap', [False, True])
@pytest.mark.parametrize('half', [1, 32, 96])
def test_pos_embedding(ops, half, swap):
    v, f = torch.tensor(R.POS_VALUES, dtype=torch.float32), R.pos_freqs(half)
    ref, bound = R.pos_embedding_ref(v, f, swap)
    got = ops.pos_embedding(v.to(DEV), f.to(DEV), swap=swap)
    assert tuple(got.shape) == (len(R.POS_VALUES), 2 * half)
    check(f'pos_embedding half={half} swap={swap}', got, ref, bound)
    # layout, on its own: the cos half of v = 0 is 1, its sin half 0
    cos_half = got[0, half:] if swap else got[0, :half]
    sin_half = got[0, :half] if swap else got[0, half:]
    assert bool((cos_half == 1).all()) and bool((sin_half == 0).all())


# ---- EDM preconditioning ---------------------------------------------------------------------------------------------------------------------
def test_edm_precond(ops):
    wi, wc, wo = Worst('edm_precond_in xin'), Worst('edm_precond_in coef'), Worst('edm_precond_out D')
    for x, sig, F in R.precond_cases():
        (xin, bxin), (coef, bcoef) = R.precond_in_ref(x, sig, 0.5)
        gx, gc = ops.edm_precond_in(x.to(DEV), sig.to(DEV), 0.5)
        case = f'sigma={sig.tolist()} shape={tuple(x.shape)}'
        wi.add(gx, xin, bxin, case)
        wc.add(gc, coef, bcoef, case)
        D, bD = R.precond_out_ref(x, F, gc.cpu())
        wo.add(ops.edm_precond_out(x.to(DEV), F.to(DEV), gc), D, bD, case)
    for w in (wi, wc, wo):
        w.report()


# ---- Heun ------------------------------------------------------------------------------------------------------------------------------------
def test_heun_step(ops):
    t = R.sigma_schedule()
    wx, wd, wn, wcr = Worst('heun_xhat'), Worst('heun_euler d_cur'), Worst('heun_euler x_next'), Worst('heun_correct')
    for x, eps, nb, interleave, i in R.heun_cases():
        t_hat, coef = R.churned(float(t[i]))
        t_next = float(t[i + 1])
        case = f'xb={x.shape[0]} nb={nb} interleave={interleave} chw={x.shape[1]} eps={name(eps.dtype)} step={i}'
        ref, bound = R.heun_xhat_ref(x, eps, coef, nb, interleave)
        x_hat = ops.heun_xhat(x.to(DEV), eps.to(DEV), coef, nb, interleave=interleave)
        wx.add(x_hat, ref, bound, case)
        # the row mapping on its own: row r of x_cur is 10 (r + 1) + [0, 0.25), the noise term is below 4 sigma * coef
        src = R.row_map(nb, x.shape[0], interleave)
        assert torch.equal(((x_hat.cpu() - coef * eps.double()) / 10).round().long()[:, 0] - 1, src), case
        xh = x_hat.cpu()                                                            # the next kernels' exact input
        D = (xh.float() * 0.3 + 0.1)
        (d, bd), (xn, bxn) = R.heun_euler_ref(xh, D, t_hat, t_next)
        d_cur, x_next = ops.heun_euler(x_hat, D.to(DEV), t_hat, t_next)
        wd.add(d_cur, d, bd, case)
        wn.add(x_next, xn, bxn, case)
        if i < 17:
            dc, xnc = d_cur.cpu(), x_next.cpu()
            D2 = (xnc.float() * 0.3 + 0.1)
            out, bo = R.heun_correct_ref(xh, D2, dc, t_hat, t_next, xnc)
            wcr.add(ops.heun_correct(x_hat, D2.to(DEV), d_cur, t_hat, t_next, x_next), out, bo, case)
    for w in (wx, wd, wn, wcr):
        w.report()


# ---- candidate_noise -------------------------------------------------------------------------------------------------------------------------
def test_candidate_noise(ops):
    ws = Worst('candidate_noise')
    for pivot, g_, mode, scale in R.candidate_cases():
        ref, bound = R.candidate_noise_ref(pivot, g_, mode, scale)
        got = ops.candidate_noise(pivot.to(DEV), g_.to(DEV), mode.to(DEV), scale.to(DEV))
        ws.add(got, ref, bound, f'b={pivot.shape[0]} chw={pivot.shape[1]} mode={mode.tolist()}')
        b = pivot.shape[0]
        keep = (mode == 0).repeat_interleave(b)
        assert torch.equal(got.cpu()[keep], g_[keep])                                   # mode 0: a copy, bit for bit
        zero = ((mode == 1) & (scale == 0)).repeat_interleave(b)
        assert torch.equal(got.cpu()[zero], pivot[torch.arange(g_.shape[0]) % b][zero])   # scale 0: the pivot itself
    ws.report()


# ---- DDIM candidates, classifier-free guidance -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', R.STORAGE)
def test_ddim_candidates(ops, dtype):
    wp, w0 = Worst(f'ddim_candidates {name(dtype)} prev'), Worst(f'ddim_candidates {name(dtype)} x0')
    for x, e, z, at, ap, st, want_x0 in R.ddim_cases(dtype):
        (prev, bprev), (x0, bx0) = R.ddim_ref(x, e, z, at, ap, st)
        gp, g0 = ops.ddim_candidates(x.to(DEV), e.to(DEV), None if z is None else z.to(DEV), at, ap, st, want_x0=want_x0)
        case = f'a_t={at} a_prev={ap} sigma_t={st:.4f} ncand={1 if z is None else z.shape[0]} count={x.numel()}'
        assert gp.dtype == dtype and tuple(gp.shape) == tuple(prev.shape) and (g0 is None) == (not want_x0)
        wp.add(gp, prev, R.rounded_bound(prev, bprev, dtype), case)
        if want_x0:
            w0.add(g0, x0, R.rounded_bound(x0, bx0, dtype), case)
    wp.report()
    w0.report()


@pytest.mark.parametrize('dtype', R.STORAGE)
def test_cfg_combine(ops, dtype):
    ws = Worst(f'cfg_combine {name(dtype)}')
    for u, c in R.cfg_cases(dtype):
        for gd in R.GUIDANCE:
            ref, bound = R.cfg_ref(u, c, gd)
            got = ops.cfg_combine(u.to(DEV), c.to(DEV), gd)
            ws.add(got, ref, R.rounded_bound(ref, bound, dtype), f'guidance={gd} count={u.numel()}')
            if gd == 0.0:
                assert torch.equal(got.cpu(), u)                                        # bit for bit
    ws.report()


# ---- attention-pool tokens, take_token ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', R.STORAGE)
def test_attnpool_tokens_and_take_token(ops, dtype):
    ws = Worst(f'attnpool_tokens {name(dtype)}')
    for x, pos in R.attnpool_cases(dtype):
        n, hw, c = x.shape
        ref, bound = R.attnpool_tokens_ref(x, pos)
        tok = ops.attnpool_tokens(x.view(n, hw, 1, c).to(DEV), pos.to(DEV))
        assert tok.dtype == dtype and tuple(tok.shape) == (n, hw + 1, c)
        ws.add(tok, ref, R.rounded_bound(ref, bound, dtype), f'n={n} hw={hw} c={c}')
        for token in (0, hw):
            assert torch.equal(ops.take_token(tok, token).cpu(), tok[:, token].float().cpu())
    ws.report()


# ---- layout, packing, casts: equality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', R.STORAGE)
@pytest.mark.parametrize('c', [3, 5, 24])
def test_layout_and_casts(ops, dtype, c):
    g_ = R.gen(101 + c)
    n, h, w = 2, 5, 7
    x = torch.randn(n, c, h, w, generator=g_) * 3
    assert torch.equal(ops.nchw_to_nhwc(x.to(DEV), dtype).cpu(), R.nchw_to_nhwc_ref(x, dtype))
    pad = ops.nchw_to_nhwc_pad(x.to(DEV), dtype, 64).cpu()
    assert torch.equal(pad, R.nchw_to_nhwc_ref(x, dtype, cpad=64)) and not pad[..., c:].any()
    y = (torch.randn(n, h, w, c, generator=g_) * 3).to(dtype)                            # its own NHWC tensor: not a round trip
    assert torch.equal(ops.nhwc_to_nchw(y.to(DEV)).cpu(), y.float().permute(0, 3, 1, 2).contiguous())
    O = 6
    wt = torch.randn(O, c, 3, 3, generator=g_)
    perm = torch.tensor([4, 0, 5, 2, 1, 3], dtype=torch.int32)
    assert torch.equal(ops.pack_conv_weight(wt.to(DEV), dtype).cpu(), R.pack_conv_weight_ref(wt, dtype))
    assert torch.equal(ops.pack_conv_weight(wt.to(DEV), dtype, out_perm=perm.to(DEV)).cpu(), R.pack_conv_weight_ref(wt, dtype, perm))
    assert torch.equal(ops.cast_from_f32(x.to(DEV), dtype).cpu(), x.to(dtype))
    assert torch.equal(ops.cast_to_f32(y.to(DEV)).cpu(), y.float())
    print(f'layout / pack / cast {name(dtype)} c={c}: equal')


# ---- the second trip of every grid-stride loop -----------------------------------------------------------------------------------------------
def _wrap_layout(ops):
    n, c, h, w = R.WRAP_SHAPE
    x = torch.randn(n, c, h, w, generator=R.gen(110))
    dt = torch.bfloat16
    assert torch.equal(ops.nchw_to_nhwc(x.to(DEV), dt).cpu(), R.nchw_to_nhwc_ref(x, dt))
    assert torch.equal(ops.nchw_to_nhwc_pad(x.to(DEV), dt, 8).cpu(), R.nchw_to_nhwc_ref(x, dt, cpad=8))
    y = x.permute(0, 2, 3, 1).contiguous().to(torch.float16)
    assert torch.equal(ops.nhwc_to_nchw(y.to(DEV)).cpu(), y.float().permute(0, 3, 1, 2).contiguous())
    wt = x.view(c * 49, 2141, 1, 1)                                                        # O = 245, I = 2141
    perm = torch.randperm(c * 49, generator=R.gen(111)).to(torch.int32)
    assert torch.equal(ops.pack_conv_weight(wt.to(DEV), dt, out_perm=perm.to(DEV)).cpu(), R.pack_conv_weight_ref(wt, dt, perm))
    flat = x.view(-1)
    assert torch.equal(ops.cast_from_f32(flat.to(DEV), torch.float16).cpu(), flat.to(torch.float16))
    assert torch.equal(ops.cast_to_f32(flat.to(dt).to(DEV)).cpu(), flat.to(dt).float())
    img = torch.randint(0, 256, (R.WRAP,), generator=R.gen(112), dtype=torch.uint8)
    assert torch.equal(ops.u8_to_unit_f32(img.to(DEV)).cpu(), R.u8_to_unit_ref(img))
    tok = torch.randn(245, 3, 2141, generator=R.gen(113)).to(dt)                            # n * c == WRAP
    assert torch.equal(ops.take_token(tok.to(DEV), 2).cpu(), tok[:, 2].float())


def _wrap_precond(ops):
    g_ = R.gen(114)
    x = torch.randn(5, R.WRAP // 5, generator=g_, dtype=torch.float64) * 80
    sig = torch.tensor([80.0, 1.0, 0.3, 0.002, 7.0], dtype=torch.float64)
    F = torch.randn(5, R.WRAP // 5, generator=g_)
    (xin, bxin), (coef, bcoef) = R.precond_in_ref(x, sig, 0.5)
    gx, gc = ops.edm_precond_in(x.to(DEV), sig.to(DEV), 0.5)
    check('wrap edm_precond_in xin', gx, xin, bxin)
    check('wrap edm_precond_in coef', gc, coef, bcoef)
    D, bD = R.precond_out_ref(x, F, gc.cpu())
    check('wrap edm_precond_out', ops.edm_precond_out(x.to(DEV), F.to(DEV), gc), D, bD)


def _wrap_heun(ops):
    g_ = R.gen(115)
    chw = R.WRAP // 5
    x = 10.0 * torch.arange(1, 6, dtype=torch.float64)[:, None] + 0.25 * torch.rand(5, chw, generator=g_, dtype=torch.float64)
    eps = torch.randn(5, chw, generator=g_)
    t = R.sigma_schedule()
    t_hat, coef = R.churned(float(t[8]))
    t_next = float(t[9])
    ref, bound = R.heun_xhat_ref(x, eps, coef, 5, False)
    x_hat = ops.heun_xhat(x.to(DEV), eps.to(DEV), coef, 5)
    check('wrap heun_xhat', x_hat, ref, bound)
    xh = x_hat.cpu()
    D = xh.float() * 0.3 + 0.1
    (d, bd), (xn, bxn) = R.heun_euler_ref(xh, D, t_hat, t_next)
    d_cur, x_next = ops.heun_euler(x_hat, D.to(DEV), t_hat, t_next)
    check('wrap heun_euler d_cur', d_cur, d, bd)
    check('wrap heun_euler x_next', x_next, xn, bxn)
    dc, xnc = d_cur.cpu(), x_next.cpu()
    D2 = xnc.float() * 0.3 + 0.1
    out, bo = R.heun_correct_ref(xh, D2, dc, t_hat, t_next, xnc)
    check('wrap heun_correct', ops.heun_correct(x_hat, D2.to(DEV), d_cur, t_hat, t_next, x_next), out, bo)


def _wrap_sd(ops):
    g_ = R.gen(116)
    dt = torch.float16
    x, e = torch.randn(R.WRAP, generator=g_).to(dt), torch.randn(R.WRAP, generator=g_).to(dt)
    z = torch.randn(2, R.WRAP, generator=g_).to(dt)
    at, ap = 0.3, 0.45
    st = R.ddim_sigma(at, ap, 1.0)
    (prev, bprev), (x0, bx0) = R.ddim_ref(x, e, z, at, ap, st)
    gp, g0 = ops.ddim_candidates(x.to(DEV), e.to(DEV), z.to(DEV), at, ap, st)
    check('wrap ddim_candidates prev', gp, prev, R.rounded_bound(prev, bprev, dt))
    check('wrap ddim_candidates x0', g0, x0, R.rounded_bound(x0, bx0, dt))
    ref, bound = R.cfg_ref(x, e, 7.5)
    check('wrap cfg_combine', ops.cfg_combine(x.to(DEV), e.to(DEV), 7.5), ref, R.rounded_bound(ref, bound, dt))


def _wrap_pos(ops):
    half = 64
    n = -(-R.WRAP // half)                                                                 # 8197 x 64 = 524 608 elements
    v = torch.rand(n, generator=R.gen(117)) * 80
    f = R.pos_freqs(half)
    ref, bound = R.pos_embedding_ref(v, f, False)
    check('wrap pos_embedding', ops.pos_embedding(v.to(DEV), f.to(DEV)), ref, bound)


@pytest.mark.parametrize('group', ['layout', 'precond', 'heun', 'sd', 'pos'])
def test_grid_stride_wrap(ops, group):
    """each grid-stride kernel once at 524 288 + 257 elements (quantize_u8's random set in the quantiser test is the same size)"""
    assert R.WRAP > 2048 * 256
    {'layout': _wrap_layout, 'precond': _wrap_precond, 'heun': _wrap_heun, 'sd': _wrap_sd, 'pos': _wrap_pos}[group](ops)
