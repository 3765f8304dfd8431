"""GPU: dts_attention_masked (csrc/attention.hip, attention16_kernel<T, 64, 1, 64, true, false, false, true>) against the float64 masked reference of
tests/masked_attention_reference.py, per element within attention_reference.bound16 as it stands (its input conditions stay asserted
inside it), on every input class of attention_reference.KINDS, in both 16-bit types, n = 2, heads = 2, d = 64.

  t          what it exercises
  1          a single key
  15, 17     below / across one MFMA tile of 16
  64         exactly one key tile
  65         query 64 sees one key of the second tile; for queries 0-63 that tile is wholly masked (skipped); a query block whose only
             live tile beyond the first is the diagonal one
  77         the workload (CLIP's text length)
  129, 200   later query blocks: full earlier tiles plus the diagonal tile
Mask forms: causal; causal + key_len = [t, max(1, t // 3)]; key_len alone; neither (also held to the UNMASKED att_ref64).
`all_negative` is the class with teeth: every valid logit is -16, so ONE disallowed key counted at logit 0 would take e^16 times a valid
key's weight.  Then exact properties: rows depend on nothing they may not see (bit-identical outputs when the hidden keys and values are
overwritten with +-60000), determinism, sample permutation, and the refusals.
Measured on the MI355X (worst err / bound over every t and mask form, limit 1): bfloat16 sharp 0.51, other classes 0.33 - 0.46; float16
sharp 0.46, other classes 0.35 - 0.41 -- the figures of the unmasked 64/QT1 form (tests/test_gpu_attention.py)."""
import functools

import pytest
import torch

from attention_reference import KINDS, att_ref64, bound16, inputs
from masked_attention_reference import MASK_FORMS, att_ref64_masked, key_len_of

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N, HEADS, D = 2, 2, 64
SCALE = D ** -0.5
TS = (1, 15, 17, 64, 65, 77, 129, 200)
DTYPES = [torch.bfloat16, torch.float16]
DTN = {torch.bfloat16: 'bf16', torch.float16: 'f16'}


@functools.lru_cache(maxsize=None)
def case(kind, t, dtype):
    return inputs(kind, N, t, HEADS, D, dtype)


def run(qkv, causal, key_len):
    from diffusion_tts_amd import ops
    kl = None if key_len is None else torch.tensor(key_len, dtype=torch.int32).to(DEV)
    return ops.attention_masked(qkv.to(DEV).contiguous(), HEADS, SCALE, causal=causal, key_len=kl)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: DTN[d])
@pytest.mark.parametrize('t', TS)
@pytest.mark.parametrize('kind', KINDS)
def test_masked_attention_within_the_bound(kind, t, dtype):
    qkv = case(kind, t, dtype)
    for form in MASK_FORMS:
        causal, key_len = 'causal' in form, key_len_of(form, t)
        got = run(qkv, causal, key_len)
        torch.cuda.synchronize()
        assert got.dtype == dtype and tuple(got.shape) == (N, t, HEADS * D)
        got = got.double().cpu()
        assert bool(torch.isfinite(got).all()), form
        refs = [att_ref64_masked(qkv, HEADS, SCALE, causal, key_len)]
        if form == 'neither':
            refs.append(att_ref64(qkv, HEADS, SCALE))                  # plain attention, by the reference the unmasked kernels are held to
        for ref in refs:
            bound, _ = bound16(ref, dtype)
            ratio = float(((got - ref.o).abs() / bound.clamp_min(1e-300)).max())
            print(f'attention_masked {DTN[dtype]} {kind} t={t} {form}: max err / bound {ratio:.3f}')
            assert bool(((got - ref.o).abs() <= bound).all()), (form, ratio)


def loud(x, rows):
    """x with k and v of `rows` (a bool [n, t]) overwritten by +-60000: finite, so a weight of exactly 0 keeps them out"""
    c = HEADS * D
    x = x.clone()
    sign = torch.where(torch.arange(2 * c) % 2 == 0, 60000.0, -60000.0).to(x.dtype)
    x[..., c:] = torch.where(rows[..., None], sign.expand(*x.shape[:2], 2 * c), x[..., c:])
    return x


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: DTN[d])
def test_rows_depend_on_nothing_they_may_not_see(dtype):
    t = 200
    qkv = case('randn', t, dtype)
    tok = torch.arange(t)[None, :].expand(N, t)
    # causal: queries < 100 never see keys >= 100
    a = run(qkv, True, None)
    b = run(loud(qkv, tok >= 100), True, None)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    assert torch.equal(a[:, :100], b[:, :100])
    assert not torch.equal(a[:, 100:], b[:, 100:])                     # (the rows that do see them move: the overwrite reached the kernel)
    # key_len, not causal: no query sees a key at or past its sample's length
    kl = [100, 37]
    a = run(qkv, False, kl)
    b = run(loud(qkv, tok >= torch.tensor(kl)[:, None]), False, kl)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    assert torch.equal(a, b)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: DTN[d])
def test_deterministic_and_samples_permute(dtype):
    t = 129
    qkv = case('rising', t, dtype)
    for causal, kl in ((True, None), (True, [t, 43]), (False, [t, 43])):
        a = run(qkv, causal, kl)
        assert torch.equal(a, run(qkv, causal, kl))
        b = run(qkv[[1, 0]], causal, None if kl is None else kl[::-1])
        assert torch.equal(b[0], a[1]) and torch.equal(b[1], a[0])


def test_refusals_name_the_value():
    from diffusion_tts_amd import ops
    x = torch.zeros(2, 17, 3 * 2 * 128, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match=r'\(-3\).*head dim 128'):
        ops.attention_masked(x, 2, 0.1)
    x = torch.zeros(2, 17, 3 * 2 * 64, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match=r'\(-3\).*dtype 0 \(DTS_F32\)'):
        ops.attention_masked(x, 2, 0.1)
    x = x.half()
    with pytest.raises(ValueError, match='key_len'):
        ops.attention_masked(x, 2, 0.1, key_len=torch.ones(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match='key_len'):
        ops.attention_masked(x, 2, 0.1, key_len=torch.ones(2, dtype=torch.int64, device=DEV))
