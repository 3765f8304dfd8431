"""Pins tests/attention_reference.py on the CPU, without any kernel: att_ref64 against torch's float64 softmax; the inputs are FAIR
(the kernels' documented arithmetic, emulated in torch with either float16 subnormal convention, stays inside bound16 at every element of
every class, type and shape the GPU tests launch); the float16 flush allowance is not what carries the bound outside `sharp`; and the
net has TEETH (three deliberately wrong emulations each leave the bound on a named class, in both 16-bit types)."""
import ast
import functools
import math
import os

import pytest
import torch

from attention_reference import KINDS, att_ref64, bound16, emulate16, inputs, shapes, split_qkv, tokens_of

DTYPES = [torch.bfloat16, torch.float16]
DTN = {torch.bfloat16: 'bf16', torch.float16: 'f16'}


@functools.lru_cache(maxsize=None)
def case(kind, shape, dtype):
    n, t, heads, d = shape
    x = inputs(kind, n, t, heads, d, dtype)
    ref = att_ref64(x, heads, 1.0 / math.sqrt(d))
    return x, ref, bound16(ref, dtype)


def worst(got, ref, bound):
    return float(((got.double() - ref.o).abs() / bound).max())


def test_att_ref64_is_float64_softmax_attention():
    n, t, heads, d = 2, 37, 3, 64
    x = inputs('randn', n, t, heads, d, torch.float32)
    q, k, v = split_qkv(x.double(), heads)
    want = tokens_of(torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1) @ v)
    ref = att_ref64(x, heads, 0.125)
    assert float((ref.o - want).abs().max()) < 1e-14
    assert bool((ref.A >= ref.o.abs()).all()) and float((ref.w.sum(-1) - 1).abs().max()) < 1e-14 and float(ref.p.amax(-1).min()) == 1.0


@pytest.mark.parametrize('dtype', DTYPES, ids=DTN.get)
@pytest.mark.parametrize('kind', KINDS)
def test_inputs_are_fair_and_the_flush_term_hides_nothing(kind, dtype):
    """emulate16 <= 1.0 of bound16 everywhere, with float16 subnormals kept and flushed (a condition on the INPUTS and the bound, checked
    without the kernel); and outside `sharp` the flush allowance is below 10 % of the bound at every element."""
    over_all = 0.0
    for shape in shapes():
        n, t, heads, d = shape
        x, ref, (bound, flush) = case(kind, shape, dtype)
        assert x.dtype == dtype and tuple(x.shape) == (n, t, 3 * heads * d) and bool(torch.isfinite(x).all())
        r = [worst(emulate16(x, heads, 1.0 / math.sqrt(d), dtype, fl), ref, bound) for fl in (False, True)]
        share = float((flush / bound).max())
        over_all = max(over_all, *r)
        print(f'{kind} {DTN[dtype]} n={n} t={t} heads={heads} d={d}: emulation err/bound {r[0]:.3f} (subnormals kept) {r[1]:.3f} (flushed), flush share {share:.3f}, |row max| log2e {ref.mb:.0f}')
        assert max(r) <= 1.0, (shape, r)
        if kind != 'sharp':
            assert share < 0.10, (shape, share)
    print(f'{kind} {DTN[dtype]}: worst emulation err/bound over {len(shapes())} shapes {over_all:.3f}')


def test_classes_are_what_they_claim():
    """all_negative: a counted zero key would take nearly all the mass; rising: the maximum rises in every key tile, for every row; falling:
    it never moves after the first tile"""
    n, t, heads, d = 2, 200, 2, 64
    for kind in ('all_negative', 'rising', 'falling'):
        q, k, _ = split_qkv(inputs(kind, n, t, heads, d, torch.float16).double(), heads)
        s = q @ k.transpose(-1, -2) / math.sqrt(d)
        tile_max = torch.stack([s[..., k0:k0 + 64].amax(-1) for k0 in range(0, t, 64)], -1)        # [n, h, q, tiles]
        if kind == 'all_negative':
            assert float(s.max()) < -12.0 and float((1.0 / (1.0 + torch.exp(s).sum(-1))).min()) > 0.99
        elif kind == 'rising':
            assert bool((tile_max[..., 1:] > tile_max[..., :-1]).all())
        else:
            assert bool((tile_max[..., 1:] < tile_max[..., :1]).all())


# (mutation, the class that must catch it, shape): ragged sequences; the skipped rescale sits on a middle tile of four
TEETH = [('pad', 'all_negative', (2, 65, 2, 64)), ('pad', 'all_negative', (2, 200, 2, 128)), ('pad', 'all_negative', (2, 300, 2, 64)),
         (('skip', 2), 'rising', (2, 200, 2, 64)), (('skip', 1), 'rising', (2, 129, 2, 128)), (('skip', 2), 'rising', (2, 200, 1, 512)),
         ('heads', 'randn', (2, 65, 2, 64)), ('heads', 'flat', (2, 17, 2, 256)), ('heads', 'falling', (2, 200, 2, 64))]


@pytest.mark.parametrize('dtype', DTYPES, ids=DTN.get)
@pytest.mark.parametrize('mutation,kind,shape', TEETH, ids=lambda v: v if isinstance(v, str) else '-'.join(map(str, v)))
def test_the_net_has_teeth(mutation, kind, shape, dtype):
    """(a) one zero key and value counted past the end of a ragged sequence, (b) the rescale of O and l skipped on one tile whose maximum
    rose, (c) the value rows of heads 0 and 1 swapped: each must leave the bound, whichever way float16 subnormals go"""
    n, t, heads, d = shape
    x, ref, (bound, _) = case(kind, shape, dtype)
    for fl in (False, True):
        good = worst(emulate16(x, heads, 1.0 / math.sqrt(d), dtype, fl), ref, bound)
        bad = worst(emulate16(x, heads, 1.0 / math.sqrt(d), dtype, fl, mutation=mutation), ref, bound)
        print(f'{mutation} on {kind} {DTN[dtype]} {shape} flush={fl}: err/bound {bad:.1f} (unmutated {good:.3f})')
        assert good <= 1.0 < bad


def test_reference_shares_no_code_with_what_it_measures():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'attention_reference.py')) as f:
        tree = ast.parse(f.read())
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods.update(a.name.split('.')[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            mods.add((node.module or '').split('.')[0])
    assert mods == {'math', 'types', 'torch'}, mods
