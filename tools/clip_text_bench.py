#!/usr/bin/env python3
"""First measurement of the CLIP text tower on the HIP kernels (diffusion_tts_amd/clip_text.py) against the module the SD backend loads by
default: one random-init text encoder of SD-1.5's shape (12 layers, hidden 768, 12 heads, intermediate 3072, vocabulary 49408), 2 rows x 77
tokens -- the prompt and the negative prompt of one search -- in float16.  GPU only.

Two paths ALTERNATE in the same process on the same ids: `CLIPTextModel` of transformers in float16 on the GPU, and CLIPTextTower in
float16.  Each gets `--warmup` forwards, then `--iters` timed ones (device events around each forward); the figure is the median.  Appends
ONE JSON line to profiles/clip_text_bench.jsonl (and prints it): ms per forward of both paths, their ratio, the ops.* calls of a HIP
forward and the share of its stream time inside them (a device-event pair around every ops.* call of one extra forward, as
tools/clip_bench.py), the time of dts_attention_masked and dts_text_tokens alone at this shape, and the largest difference of the two
paths' outputs.  No pass/fail threshold and no claim: the tower runs once per prompt, it is not a hot path.

--hip-only N: N forwards of the HIP tower and nothing else, for a kernel trace (`rocprofv3 --kernel-trace --stats -- python
tools/clip_text_bench.py --hip-only 5`)."""
import argparse
import json
import os
import statistics
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from diffusion_tts_amd import ops
from diffusion_tts_amd.clip_text import CLIPTextTower
from op_timing import op_shares, timed_forward

FAMILY = {'conv2d': 'conv (1x1: projections, MLP)', 'attention_masked': 'attention_masked', 'layer_norm': 'layer_norm', 'gelu': 'gelu',
          'text_tokens': 'text_tokens (incl. the host check and the upload of the ids)', 'cast_to_f32': 'projection (cast, linear)',
          'linear': 'projection (cast, linear)'}


def sd15_text(layers):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        from transformers import CLIPTextConfig, CLIPTextModel
        tc = CLIPTextConfig(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=layers, num_attention_heads=12,
                            max_position_embeddings=77, projection_dim=768, bos_token_id=49406, eos_token_id=49407, pad_token_id=49407)
        torch.manual_seed(0)
        return CLIPTextModel(tc).eval()


def kernel_us(fn, reps=200):
    """microseconds per call of one kernel launched `reps` times back to back (device events around the batch): launch-bound at this size"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / reps, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=2)
    ap.add_argument('--layers', type=int, default=12)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--hip-only', type=int, default=0, help='run only this many forwards of the HIP tower (for a kernel trace)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clip_text_bench.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('clip_text_bench: needs a GPU (no CPU fallback, nothing is measured without one)')
    model = sd15_text(a.layers)
    tower = CLIPTextTower.from_text_model(model, dtype=torch.float16, device='cuda')
    ids = torch.randint(0, 49406, (a.rows, 77), generator=torch.Generator().manual_seed(0))
    ids[:, 0] = 49406
    for b in range(a.rows):                         # the prompt rows end at different lengths, padded with the end token as the tokenizer does
        ids[b, 9 + 31 * b % 68:] = 49407
    if a.hip_only:
        for _ in range(a.hip_only):
            out = tower(ids)
        torch.cuda.synchronize()
        print(json.dumps({'hip_only_forwards': a.hip_only, 'output_finite': bool(torch.isfinite(out[0]).all())}))
        return
    model = model.to('cuda', torch.float16)
    ids_dev = ids.to('cuda')

    def run_tf():
        with torch.no_grad():
            return model(input_ids=ids_dev)[0]

    def run_hip():
        return tower(ids)[0]                        # host ids, as the tokenizer hands them over: the id check and the upload are inside

    for _ in range(a.warmup):
        run_tf()
        run_hip()
    torch.cuda.synchronize()
    t_tf, t_hip = [], []
    for _ in range(a.iters):                        # alternate: both paths see the same clocks and the same neighbours
        ms, o_tf = timed_forward(run_tf)
        t_tf.append(ms)
        ms, o_hip = timed_forward(run_hip)
        t_hip.append(ms)
    ms_tf, ms_hip = statistics.median(t_tf), statistics.median(t_hip)
    shares, inside, calls = op_shares(FAMILY, lambda: tower(ids))
    qkv = torch.randn(a.rows, 77, 3 * 768, generator=torch.Generator().manual_seed(1)).to('cuda', torch.float16)
    us_att = kernel_us(lambda: ops.attention_masked(qkv, 12, 0.125, causal=True))
    us_att_plain = kernel_us(lambda: ops.attention(qkv, 12, 0.125))
    ids32 = ids.to(torch.int32).to('cuda')
    out_tok = torch.empty((a.rows, 77, 768), dtype=torch.float16, device='cuda')
    us_tok = kernel_us(lambda: ops._call('dts_text_tokens', ids32.data_ptr(), tower.tok.data_ptr(), tower.pos.data_ptr(), out_tok.data_ptr(),
                                         ops.dt_code(torch.float16), a.rows, 77, 768, tower.vocab))
    res = {'what': 'CLIP text tower forward, SD-1.5 text encoder shape, random-init weights, float16', 'rows': a.rows, 'layers': a.layers,
           'tokens': 77, 'hidden': 768, 'heads': 12, 'iters': a.iters, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0),
           'transformers_f16': {'ms_per_forward': round(ms_tf, 3), 'ms_min': round(min(t_tf), 3), 'ms_max': round(max(t_tf), 3)},
           'hip_f16': {'ms_per_forward': round(ms_hip, 3), 'ms_min': round(min(t_hip), 3), 'ms_max': round(max(t_hip), 3),
                       'time_share_by_op_family': shares, 'share_inside_ops_calls': inside, 'op_calls_per_forward': calls},
           'transformers_ms_over_hip_ms': round(ms_tf / ms_hip, 3),
           'us_per_launch_back_to_back': {'dts_attention_masked (causal)': us_att, 'dts_attention (unmasked, same shape)': us_att_plain,
                                          'dts_text_tokens': us_tok},
           'max_abs_difference_of_outputs': float((o_hip.float() - o_tf.float()).abs().max()), 'max_abs_output': float(o_hip.float().abs().max()),
           'output_finite': bool(torch.isfinite(o_hip).all())}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
