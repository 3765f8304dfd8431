"""Masked self-attention in float64, written from the definition: attention_reference.att_ref64 with the disallowed keys at score -inf.
Torch on the CPU only; nothing here imports diffusion_tts_amd (tests/test_gpu_masked_attention.py holds dts_attention_masked to it, with
attention_reference.bound16 as it stands -- that bound's derivation does not care why a key has zero weight)."""
import types

import torch

from attention_reference import LOG2E, split_qkv, tokens_of

MASK_FORMS = ('causal', 'causal+key_len', 'key_len', 'neither')


def key_len_of(form, t):
    """the per-sample key lengths of a mask form for two samples (None: no key_len): the full length and a third of it"""
    return [t, max(1, t // 3)] if 'key_len' in form else None


def allowed_keys(n, t, causal, key_len):
    """bool [n, 1, t, t]: query i of sample b may attend key j iff (not causal or j <= i) and (key_len is None or j < key_len[b])"""
    ok = torch.ones(n, 1, t, t, dtype=torch.bool)
    if causal:
        ok &= torch.ones(t, t, dtype=torch.bool).tril()
    if key_len is not None:
        kl = torch.as_tensor(key_len, dtype=torch.int64)
        assert tuple(kl.shape) == (n,) and bool(((kl >= 1) & (kl <= t)).all())
        ok &= (torch.arange(t)[None, :] < kl[:, None])[:, None, None, :]
    return ok


def att_ref64_masked(qkv, heads, scale, causal, key_len):
    """att_ref64's namespace (o, A, w, p, vabs, mb, t) for the masked softmax; p = w = 0 on disallowed keys.  Every row keeps key 0, so
    every row maximum is finite."""
    n, t = qkv.shape[:2]
    q, k, v = split_qkv(qkv.double(), heads)
    s = torch.einsum('nhqd,nhkd->nhqk', q, k) * scale
    s = s.masked_fill(~allowed_keys(n, t, causal, key_len), -float('inf'))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    w = p / p.sum(-1, keepdim=True)
    o = torch.einsum('nhqk,nhkd->nhqd', w, v)
    A = torch.einsum('nhqk,nhkd->nhqd', w, v.abs())
    return types.SimpleNamespace(o=tokens_of(o), A=tokens_of(A), w=w, p=p, vabs=v.abs(), mb=float(m.abs().max()) * LOG2E, t=t)
