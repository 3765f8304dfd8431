"""Self-attention at the head dims of SD-1.x, 40 / 80 / 160, stored unpadded (csrc/attention.hip: attention16_kernel with a head dim in
memory, DM, below its on-chip K width).  The layout is dts_attention's at the TRUE head dim: qkv [n, t, 3 * heads * d], out [n, t, heads * d];
three heads here, so that head offsets of 80 h, 160 h and 320 h bytes all occur.

  form        kernel                                                              reached by
  40          attention16_kernel<T, 64, 1, 64, true, false, false, false, 40>     no knob (a small grid), att_qt=1
  40/QT2      attention16_kernel<T, 64, 2, 64, true, false, false, false, 40>     att_qt=2 (and the launcher's own rule at a 528-block grid)
  40/QT1+DB   attention16_kernel<T, 64, 1, 64, true, true, false, false, 40>      att_qt=1 att_db=1, t > 64
  40/QT2+DB   attention16_kernel<T, 64, 2, 64, true, true, false, false, 40>      att_qt=2 att_db=1, t > 64
  80          attention16_kernel<T, 96, 1, 96, true, false, false, false, 80>     head dim
  160         attention16_kernel<T, 160, 1>                                       head dim (a multiple of 32: no tail)

Every case is held to two things:
  * the float64 reference of tests/attention_reference.py at the true head dim and scale 1 / sqrt(d): max err / bound16 <= 1, the bound
    derived there from the number formats before any kernel ran;
  * the padded route, bit for bit: the same values zero-padded per head to 64 / 128 / 256, through the kernel of that head dim under the
    same knobs.  A zero tail adds exact zeros to the f32 scores, the value tiles that hold a channel < d accumulate over the same keys in
    the same order, and the softmax is the shared body -- so the outputs are equal, not merely close, and the padded channels are zero.
Then: nothing is written outside the output and nothing foreign is read (a chunk loaded past d would be the next head's; a store past d
would land in it), launches repeat bit for bit in either block order, and the entry points that do not take these dims still say so."""
import contextlib
import functools
import math

import pytest
import torch

from attention_reference import KINDS, ONE_T, TWO_T, att_ref64, bound16, inputs

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DTN = {torch.bfloat16: 'bf16', torch.float16: 'f16', torch.float32: 'f32'}
N, HEADS = 2, 3
PADDED = {40: 64, 80: 128, 160: 256}
DB_T = tuple(t for t in ONE_T if t > 64)          # double buffering needs a second key tile

# form -> (head dim, knobs, sequence lengths)
FORMS = {
    '40': (40, {}, ONE_T),
    '40/QT2': (40, dict(att_qt=2), TWO_T),
    '40/QT1+DB': (40, dict(att_qt=1, att_db=1), DB_T),
    '40/QT2+DB': (40, dict(att_qt=2, att_db=1), TWO_T),
    '80': (80, {}, ONE_T),
    '160': (160, {}, ONE_T),
}
CASES = [(f, dt) for f in FORMS for dt in (torch.bfloat16, torch.float16)]
case_id = lambda v: v if isinstance(v, str) else DTN[v]


@pytest.fixture(scope='module')
def ops():
    from diffusion_tts_amd import ops as o
    return o


@contextlib.contextmanager
def knobs(**kw):
    from diffusion_tts_amd import _lib
    try:
        for name, value in kw.items():
            _lib.set_tuning(name, value)
        yield
    finally:
        for name in ('att_qt', 'att_db', 'att_xcd'):
            _lib.set_tuning(name, -1)


@functools.lru_cache(maxsize=None)
def case16(kind, t, d, dtype, n=N, heads=HEADS):
    """(input, float64 reference, bound16) at the true head dim: computed once, shared by every test, never modified"""
    x = inputs(kind, n, t, heads, d, dtype)
    ref = att_ref64(x, heads, 1.0 / math.sqrt(d))
    return x, ref.o, bound16(ref, dtype)[0]


def pad_heads(x, heads, d, dp, blocks):
    """[n, t, blocks * heads * d] -> [n, t, blocks * heads * dp]: every head's d channels followed by dp - d zeros"""
    n, t, _ = x.shape
    out = torch.zeros((n, t, blocks, heads, dp), dtype=x.dtype, device=x.device)
    out[..., :d] = x.view(n, t, blocks, heads, d)
    return out.view(n, t, blocks * heads * dp)


def padded_route(ops, x, heads, d):
    """the same values through the kernel of the padded head dim (scale of the true one): [n, t, heads, dp]"""
    dp = PADDED[d]
    n, t, _ = x.shape
    return ops.attention(pad_heads(x, heads, d, dp, 3), heads, 1.0 / math.sqrt(d)).view(n, t, heads, dp)


def check(ops, x, ref_o, bound, heads, d):
    """(err / bound, bit-identical to the padded route and its padded channels zero) of one launch under the caller's knobs"""
    n, t, _ = x.shape
    xd = x.to(DEV)
    got = ops.attention(xd, heads, 1.0 / math.sqrt(d))
    assert got.dtype == x.dtype and tuple(got.shape) == (n, t, heads * d)
    pad = padded_route(ops, xd, heads, d)
    same = torch.equal(got.view(n, t, heads, d), pad[..., :d]) and not bool(pad[..., d:].any())
    r = float(((got.double().cpu() - ref_o).abs() / bound).max()) if bool(torch.isfinite(got).all()) else math.inf
    return r, same, got


@pytest.mark.parametrize('form,dtype', CASES, ids=case_id)
def test_every_form_against_float64_and_the_padded_route(ops, form, dtype):
    """every class x every sequence length of the form: err / bound16 <= 1 (printed), and equal to the padded route bit for bit"""
    d, kn, ts = FORMS[form]
    bad = []
    with knobs(**kn):
        for t in ts:
            ratios = []
            for kind in KINDS:
                x, ref_o, bound = case16(kind, t, d, dtype)
                r, same, _ = check(ops, x, ref_o, bound, HEADS, d)
                ratios.append(f'{kind} {r:.3f}' + ('' if same else ' (differs from the padded route)'))
                if not (r <= 1.0 and same):
                    bad.append((t, kind, r, same))
            print(f'attention native {form} {DTN[dtype]} n={N} heads={HEADS} t={t}: err/bound (limit 1) ' + ', '.join(ratios))
    assert not bad, bad


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=case_id)
def test_launcher_takes_two_query_tiles_on_a_large_grid(ops, dtype):
    """no knob: t >= 256 and ceil(t / 128) * n * heads = 3 * 22 * 8 = 528 >= 512 blocks is the launcher's own rule for the two-query-tile
    form, at head dim 40 as at 64; a block of the ragged tail holds a single query"""
    n, t, heads, d = 22, 257, 8, 40
    for kind in ('randn', 'all_negative'):
        x, ref_o, bound = case16(kind, t, d, dtype, n, heads)
        r, same_pad, got = check(ops, x, ref_o, bound, heads, d)
        with knobs(att_qt=2):
            same = torch.equal(got, ops.attention(x.to(DEV), heads, 1.0 / math.sqrt(d)))
        with knobs(att_qt=1):
            r1, same_pad1, got1 = check(ops, x, ref_o, bound, heads, d)
        print(f'attention native 40/QT2 by the launcher\'s rule {DTN[dtype]} n={n} heads={heads} t={t} {kind}: err/bound {r:.3f}, bit-identical to '
              f'att_qt=2: {same}, to the padded route: {same_pad}; att_qt=1: err/bound {r1:.3f}, padded route: {same_pad1}')
        assert r <= 1.0 and same and same_pad and r1 <= 1.0 and same_pad1


GUARD = 3          # token rows in front of and behind the tensors


def guarded(ops, x, heads, d, poison=None):
    """one launch with input and output in the middle of NaN-filled allocations (out= is the caller's view).  poison = (sample, head):
    every q / k / v channel of the OTHER heads and the whole OTHER sample become NaN.  Returns the output after checking that every element
    of it was written (or is NaN only where NaN went in) and that the bands around it still hold NaN."""
    n, t, c3 = x.shape
    c = c3 // 3
    ibuf = torch.full(((n * t + 2 * GUARD) * c3,), math.nan, dtype=x.dtype, device=DEV)
    iview = ibuf[GUARD * c3:(GUARD + n * t) * c3].view(n, t, c3)
    iview.copy_(x)
    if poison is not None:
        s, h = poison
        keep = torch.zeros(3, heads, d, dtype=torch.bool, device=DEV)
        keep[:, h] = True
        iview[:, :, ~keep.view(c3)] = math.nan
        iview[1 - s] = math.nan
    obuf = torch.full(((n * t + 2 * GUARD) * c,), math.nan, dtype=x.dtype, device=DEV)
    oview = obuf[GUARD * c:(GUARD + n * t) * c].view(n, t, c)
    ret = ops.attention(iview, heads, 1.0 / math.sqrt(d), out=oview)
    torch.cuda.synchronize()
    assert ret.data_ptr() == oview.data_ptr()
    assert bool(torch.isnan(obuf[:GUARD * c]).all()) and bool(torch.isnan(obuf[(GUARD + n * t) * c:]).all()), 'wrote outside the output'
    return oview.clone()


@pytest.mark.parametrize('form,dtype', [(f, dt) for f, dt in CASES if 'DB' not in f], ids=case_id)
@pytest.mark.parametrize('t', [17, 65, 129])
def test_nothing_outside_nothing_foreign(ops, form, dtype, t):
    """Clean run: every output element is written (no NaN left of the fill) and the guard bands keep their NaN.  Then, per (sample, head):
    with NaN in every channel of the other two heads and in the whole other sample, that head's output is the clean run's bit for bit --
    a 16-byte chunk loaded past d (the next head's q, k or v) or a store past d (into the next head's output) would show here."""
    d, kn, _ = FORMS[form]
    x = inputs('randn', N, t, HEADS, d, dtype).to(DEV)
    with knobs(**kn):
        clean = guarded(ops, x, HEADS, d)
        assert bool(torch.isfinite(clean).all()), 'an output element was not written'
        _, ref_o, bound = case16('randn', t, d, dtype)
        assert float(((clean.double().cpu() - ref_o).abs() / bound).max()) <= 1.0
        for s in range(N):
            for h in range(HEADS):
                got = guarded(ops, x, HEADS, d, poison=(s, h))
                assert torch.equal(got[s, :, h * d:(h + 1) * d], clean[s, :, h * d:(h + 1) * d]), (s, h)


@pytest.mark.parametrize('form,dtype', CASES, ids=case_id)
def test_repeat_launches_and_block_orders_are_bit_identical(ops, form, dtype):
    d, kn, _ = FORMS[form]
    t = 300 if 'QT2' in form else 200           # four key tiles, the last ragged; QT2: 3 x 6 = 18 blocks (at 8 or fewer both orders coincide)
    x, ref_o, bound = case16('rising', t, d, dtype)
    xd = x.to(DEV)
    with knobs(**kn):
        outs = [ops.attention(xd, HEADS, 1.0 / math.sqrt(d)).clone() for _ in range(3)]
    with knobs(att_xcd=0, **kn):
        plain = ops.attention(xd, HEADS, 1.0 / math.sqrt(d))
    assert float(((outs[0].double().cpu() - ref_o).abs() / bound).max()) <= 1.0
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and torch.equal(outs[0], plain)


def test_refusals_stay_loud(ops):
    z = lambda *shape, dtype=torch.float16: torch.zeros(*shape, dtype=dtype, device=DEV)
    for d in (40, 80, 160):
        with pytest.raises(RuntimeError, match=f'head dim {d}'):
            ops.attention(z(1, 64, 3 * 2 * d, dtype=torch.float32), 2, 0.1)
    with pytest.raises(RuntimeError, match='head dim 40'):
        ops.attention(z(1, 128, 3 * 2 * 40, dtype=torch.float32), 2, 0.1, x3=True)
    with pytest.raises(RuntimeError, match='head dim 40'):
        ops._call('dts_attention_x3', z(1, 128, 6 * 2 * 40).data_ptr(), z(1, 128, 2 * 40, dtype=torch.float32).data_ptr(), 0, 1, 128, 2, 40, 0.1)
    with pytest.raises(RuntimeError, match='head dim 40'):
        ops.attention_masked(z(1, 64, 3 * 2 * 40), 2, 0.1)
    with pytest.raises(RuntimeError, match='head dim 40'):
        ops.attention_x3_masked(z(1, 64, 3 * 2 * 40, dtype=torch.float32), 2, 0.1)
    with pytest.raises(RuntimeError, match='head dim 48'):
        ops.attention(z(1, 64, 3 * 2 * 48), 2, 0.1)
    with pytest.raises(RuntimeError, match='head dim 32'):
        ops.attention(z(1, 64, 3 * 2 * 32), 2, 0.1)
    # out= is checked like cross_attention's
    with pytest.raises(ValueError, match='attention: out'):
        ops.attention(z(1, 64, 3 * 2 * 40), 2, 0.1, out=z(1, 64, 2 * 64))
    with pytest.raises(ValueError, match='attention: out'):
        ops.attention(z(1, 64, 3 * 2 * 40), 2, 0.1, out=z(1, 64, 2 * 40, dtype=torch.bfloat16))
