#!/usr/bin/env python3
"""First measurement of the CLIP image tower on the HIP kernels (diffusion_tts_amd/clip_vision.py) against the path the SD search loop runs
today: one random-init CLIP at ViT-L/14's full shape (hidden 1024, 16 heads, intermediate 4096, 24 layers, 224 / 14 -> 257 tokens, projection
768), 32 rows of [3, 224, 224] pixel_values.  GPU only.

Two paths ALTERNATE in the same process on the same input: `CLIPModel.get_image_features` of transformers in float16 on the GPU, and
CLIPVisionTower in float16.  Each gets `--warmup` forwards, then `--iters` timed ones (device events around each forward); the figure is
the median.  Appends ONE JSON line to profiles/clip_tower_bench.jsonl (and prints it): ms per forward of both paths, their ratio, the
algorithmic FLOPs of a forward counted from the layer shapes, the share of the HIP forward's stream time per op family (a device-event pair
around every ops.* call of one extra forward, as tools/sd_unet_bench.py: "other" is stream time outside any ops.* call -- torch glue and
host launch gaps) and the largest difference of the two paths' outputs.  No pass/fail threshold.

--dtype f16x3: the split-precision (parity-grade) tower alternates with transformers' FLOAT32 `get_image_features` instead -- the module the
parity-grade scorer runs today -- and the line says so (keys transformers_f32 / hip_f16x3).  No speed-up is promised there: the split mode
does three 16-bit matrix products where the float32 matrix instruction runs at 1/16 of the 16-bit rate.

--hip-only N: N forwards of the HIP tower and nothing else, for a kernel trace (`rocprofv3 --kernel-trace --stats -- python tools/clip_bench.py
--hip-only 5`)."""
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
from diffusion_tts_amd.clip_vision import CLIPVisionTower, CLIPVisionTowerX3
from op_timing import op_shares, timed_forward

PEAK_16BIT_DENSE = 2.5e15          # MI355X dense f16 / bf16 matrix peak, FLOP/s
FAMILY = {'conv2d': 'conv (1x1: projections, MLP, patch embedding)', 'attention': 'attention', 'layer_norm': 'layer_norm', 'gelu': 'gelu',
          'patchify': 'embedding (patchify, tokens)', 'vit_tokens': 'embedding (patchify, tokens)', 'vit_head': 'head (vit_head, linear)',
          'linear': 'head (vit_head, linear)',
          # the split-precision mode's ops (the towers call one set or the other)
          'layer_norm_x3': 'layer_norm', 'gelu_x3': 'gelu', 'patchify_x3': 'embedding (patchify, tokens)',
          'vit_tokens_f32': 'embedding (patchify, tokens)', 'vit_head_f32': 'head (vit_head, linear)'}
MODES = {'f16': (torch.float16, torch.float16, 'float16'), 'bf16': (torch.bfloat16, torch.bfloat16, 'bfloat16'),
         'f16x3': (ops.F16X3, torch.float32, 'split precision (f16x3) against float32')}       # tower dtype, transformers dtype, label


def vit_l14(layers):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        from transformers import CLIPConfig, CLIPModel, CLIPTextConfig, CLIPVisionConfig
        tc = CLIPTextConfig(vocab_size=1000, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                            projection_dim=768, bos_token_id=998, eos_token_id=999, pad_token_id=999)      # the text tower is not measured
        vc = CLIPVisionConfig(hidden_size=1024, intermediate_size=4096, num_hidden_layers=layers, num_attention_heads=16, image_size=224,
                              patch_size=14, projection_dim=768)
        torch.manual_seed(0)
        return CLIPModel(CLIPConfig(text_config=tc.to_dict(), vision_config=vc.to_dict(), projection_dim=768)).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=32)
    ap.add_argument('--layers', type=int, default=24)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dtype', default='f16', choices=sorted(MODES), help='the tower\'s mode; transformers runs in the same 16-bit type, or in float32 beside f16x3')
    ap.add_argument('--hip-only', type=int, default=0, help='run only this many forwards of the HIP tower (for a kernel trace)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clip_tower_bench.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('clip_bench: needs a GPU (no CPU fallback, nothing is measured without one)')
    model = vit_l14(a.layers)
    tower_dtype, tf_dtype, label = MODES[a.dtype]
    tf_key, hip_key = 'transformers_' + ops.dtype_name(tf_dtype), 'hip_' + a.dtype
    tower = (CLIPVisionTowerX3 if tower_dtype == ops.F16X3 else CLIPVisionTower).from_clip_model(model, dtype=tower_dtype, device='cuda')
    pix = torch.randn(a.rows, 3, 224, 224, generator=torch.Generator().manual_seed(0)).to('cuda')
    if a.hip_only:
        for _ in range(a.hip_only):
            out = tower(pix)
        torch.cuda.synchronize()
        print(json.dumps({'hip_only_forwards': a.hip_only, 'output_finite': bool(torch.isfinite(out).all())}))
        return
    model = model.to('cuda', tf_dtype)
    pix16 = pix.to(tf_dtype)

    def run_tf():
        with torch.no_grad():
            o = model.get_image_features(pixel_values=pix16)
        return o if isinstance(o, torch.Tensor) else o.pooler_output

    def run_hip():
        return tower(pix)

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
    shares, inside, calls = op_shares(FAMILY, lambda: tower(pix))
    flops = tower.flops(a.rows)
    res = {'what': 'CLIP image tower forward, ViT-L/14 shape, random-init weights, ' + label, 'rows': a.rows, 'layers': a.layers, 'tokens': tower.tokens,
           'pixel_values': [3, 224, 224], 'iters': a.iters, 'warmup': a.warmup, 'device': torch.cuda.get_device_name(0),
           'algorithmic_flops_per_forward': flops,
           tf_key: {'ms_per_forward': round(ms_tf, 3), 'ms_min': round(min(t_tf), 3), 'ms_max': round(max(t_tf), 3),
                                'tflops_algorithmic': round(flops / ms_tf / 1e9, 1)},
           hip_key: {'ms_per_forward': round(ms_hip, 3), 'ms_min': round(min(t_hip), 3), 'ms_max': round(max(t_hip), 3),
                       'tflops_algorithmic': round(flops / ms_hip / 1e9, 1),
                       'fraction_of_dense_16bit_peak_end_to_end': round(flops / (ms_hip * 1e-3) / PEAK_16BIT_DENSE, 4),
                       'time_share_by_op_family': shares, 'share_inside_ops_calls': inside, 'op_calls_per_forward': calls},
           'transformers_ms_over_hip_ms': round(ms_tf / ms_hip, 3),
           'max_abs_difference_of_outputs': float((o_hip - o_tf.float()).abs().max()), 'max_abs_output': float(o_hip.abs().max()),
           'output_finite': bool(torch.isfinite(o_hip).all())}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
