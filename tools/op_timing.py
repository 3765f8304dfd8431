"""Device-event timing shared by the bench tools (clip_bench.py, clip_text_bench.py, sd_unet_bench.py).  op_shares works by replacing
attributes of the `ops` module for one forward, so it sees only kernels that the package calls as `ops.<name>(...)`."""
import torch
from diffusion_tts_amd import ops


def timed_forward(fn):
    """(milliseconds between device events around fn(), its result)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def op_shares(family, run):
    """One run() -- a forward -- with a device-event pair around every ops.* call named in `family` ({ops attribute: family name}).
    -> ({family: share of the forward's stream time}, the share inside any ops.* call, the number of ops.* calls)"""
    spans, saved = [], {}
    for name, fam in family.items():
        fn = saved[name] = getattr(ops, name)

        def timed(*a, _fn=fn, _fam=fam, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = _fn(*a, **kw)
            e1.record()
            spans.append((_fam, e0, e1))
            return r
        setattr(ops, name, timed)
    try:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)
    fam_ms = {}
    for fam, a, b in spans:
        fam_ms[fam] = fam_ms.get(fam, 0.0) + a.elapsed_time(b)
    total = e0.elapsed_time(e1)
    inside = sum(fam_ms.values())
    fam_ms['other (torch glue, launch gaps)'] = max(0.0, total - inside)
    return {k: round(v / total, 4) for k, v in sorted(fam_ms.items(), key=lambda kv: -kv[1])}, round(inside / total, 4), len(spans)
