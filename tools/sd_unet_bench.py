#!/usr/bin/env python3
"""Measurement of the SD-1.5 U-Net on the HIP kernels (diffusion_tts_amd/sd_unet.py): one forward over the 2N = 32 rows of BASELINE
config 4 ([32,4,64,64] latents, two distinct [77,768] contexts), random-init weights of SD-1.5's shape, float16 and bfloat16.  GPU only.

Prints ONE JSON line: per dtype ms per forward (median of the timed forwards, device events around each forward, after warm-up), rows/s,
the algorithmic FLOPs of a forward counted from the layer shapes (true head dims and the strided form of the three downsample
convolutions: what the model asks for, not what the zero-padded heads / space-to-depth form execute), the whole-forward rate as a fraction of
the dense 16-bit matrix peak (an END-TO-END figure, not any kernel's share of peak), and the share of the forward's time per op
family from one extra, instrumented forward: a device-event pair is recorded around every ops.* call of the module, nothing synchronises
until the end, so each span is the stream time between the two records (the op's kernels plus whatever gap precedes the closing record) and
"other" is the forward's total minus the summed spans, i.e. stream time outside any ops.* call (torch glue kernels such as unique / slicing,
and host launch gaps when the stream runs dry; taken with graph replay off, a replayed forward makes no ops.* call).

The forward is captured once per shape and replayed (SDUNet._graphs), so each dtype is timed four ways in ONE process on the same inputs,
alternating forward by forward: eager launches (`_graphs.enabled = False`) and graph replay, each through the stock call surface (32
encoder_hidden_states rows, grouped on the device, one 4-byte readback) and through `context_rows=` (the two distinct contexts and a row
map, no host synchronisation).  `ms_per_forward` stays what it was before replay existed -- eager launches, stock surface -- so records
of different commits compare.  `grouping` times ops.group_rows plus the readback of its count against torch.unique(dim=0,
return_inverse=True), which waits for the size of its own result, on the same [32, 59136] 16-bit rows (host clock around work that ends in a
synchronise).
--replay-only N: nothing but N replayed context_rows forwards after the warm-up, for a kernel trace of its own (--replay-head-dims picks
the mode of that model).  No pass/fail threshold.
--head-dims padded,native: instead of the above, per dtype one model of each listed SDUNet head_dims mode in ONE process on the same inputs;
replayed context_rows forwards alternate between the modes, forward by forward, device events around each; reports the median, minimum
and maximum of --iters forwards per mode after the warm-up, the ratio of the medians against the first listed mode, and rel. max
|difference| of the outputs.  The padded mode is the default path, so it is what native is measured against in the same minute.
--downsample s2d,strided: the same table for the SDUNet downsample modes (head_dims padded), plus `downsample_layers`: the three Downsample2D
launches alone at --rows rows ([rows, 64 / 32 / 16, .., 320 / 640 / 1280] inputs), both routes alternating, a device-event pair around each
route's launches (the space-to-depth pass counts with its convolution), median / min / max of --iters in microseconds."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault('DTS_GRAPHS_STRICT', '1')      # a refused capture is an error here: eager figures must not appear under the replay name
import torch
from diffusion_tts_amd import init as dinit
from diffusion_tts_amd import ops
from diffusion_tts_amd.sd_unet import SDUNet
from op_timing import op_shares

PEAK_16BIT_DENSE = 2.5e15          # MI355X dense f16 / bf16 matrix peak, FLOP/s


def forward_flops(boc=(320, 640, 1280, 1280), heads=8, ctx_dim=768, ctx_len=77, lpb=2, res=64, distinct_contexts=2):
    """multiply-adds x 2 of one row's forward (+ the context projections of the distinct contexts, spread over the batch by the caller)"""
    per_row, per_ctx = 0, 0
    temb = 4 * boc[0]

    def conv(cin, cout, k, hw):
        return 2 * cin * cout * k * k * hw

    def resnet(cin, cout, hw):
        f = conv(cin, cout, 3, hw) + conv(cout, cout, 3, hw) + 2 * temb * cout
        return f + (conv(cin, cout, 1, hw) if cin != cout else 0)

    def transformer(c, hw):
        nonlocal per_ctx
        per_ctx += 2 * 2 * ctx_dim * c * ctx_len                                     # to_k, to_v of the text tokens
        f = 2 * conv(c, c, 1, hw)                                                    # proj_in, proj_out
        f += 4 * conv(c, c, 1, hw) + 2 * 2 * hw * hw * c                             # attn1: q, k, v, out + Q.K^T, P.V
        f += 2 * conv(c, c, 1, hw) + 2 * 2 * hw * ctx_len * c                        # attn2: q, out + Q.K^T, P.V over the tokens
        return f + conv(c, 8 * c, 1, hw) + conv(4 * c, c, 1, hw)                     # GEGLU feed-forward

    hw = res * res
    per_row += conv(4, boc[0], 3, hw) + 2 * boc[0] * temb + 2 * temb * temb
    skips, prev = [boc[0]], boc[0]
    for i, c in enumerate(boc):
        last = i == len(boc) - 1
        for _ in range(lpb):
            per_row += resnet(prev, c, hw) + (0 if last else transformer(c, hw))
            prev = c
            skips.append(c)
        if not last:
            hw //= 4
            per_row += conv(c, c, 3, hw)
            skips.append(c)
    per_row += 2 * resnet(prev, prev, hw) + transformer(prev, hw)
    for i, c in enumerate(boc[::-1]):
        for _ in range(lpb + 1):
            per_row += resnet(prev + skips.pop(), c, hw) + (0 if i == 0 else transformer(c, hw))
            prev = c
        if i != len(boc) - 1:
            hw *= 4
            per_row += conv(c, c, 3, hw)
    per_row += conv(boc[0], 4, 3, hw)
    return per_row, per_ctx * distinct_contexts


FAMILY = {'conv2d': 'conv', 'group_norm': 'group_norm', 'attention': 'self_attention', 'cross_attention': 'cross_attention',
          'layer_norm': 'layer_norm', 'geglu': 'geglu', 'linear': 'time_embedding', 'pos_embedding': 'time_embedding',
          'cast_from_f32': 'time_embedding', 'space_to_depth2': 'layout', 'nchw_to_nhwc_pad': 'layout'}


def grouping(ehs, reps=20):
    """us per call, host clock, each ending in the readback the U-Net's host part waits for: ops.group_rows + its count, against
    torch.unique over the int16 view (what SDUNet ran before), which waits for the size of its own result"""
    n = ehs.shape[0]
    bits = ehs.reshape(n, -1).view(torch.int16)

    def ours():
        slot, reps_, count = ops.group_rows(ehs)
        return int(count)

    def unique():
        uniq, inverse = torch.unique(bits, dim=0, return_inverse=True)      # synchronises by itself: the size of its result is data
        return uniq.shape[0]
    out = {'rows': n, 'row_bytes': bits.shape[1] * 2}
    for name, f in (('group_rows_plus_readback_us', ours), ('torch_unique_plus_readback_us', unique)):
        for _ in range(3):
            f()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e6)
        out[name] = {'median': round(statistics.median(ts), 1), 'min': round(min(ts), 1), 'max': round(max(ts), 1)}
    out['groups'] = ours()
    return out


def downsample_layers(a, dt, boc=(320, 640, 1280), res=64):
    """the three Downsample2D launches alone, both routes on the same input and weight, alternating launch by launch"""
    g = torch.Generator().manual_seed(1)
    out = {}
    for i, c in enumerate(boc):
        hw = res >> i
        x = torch.randn(a.rows, hw, hw, c, generator=g).to('cuda', dt)
        w = (torch.randn(c, c, 3, 3, generator=g) / (3.0 * c ** 0.5)).to('cuda')
        b = torch.randn(c, generator=g).to('cuda')
        w1, w4 = ops.pack_conv_weight(w, dt), ops.pack_conv_weight(ops.stride2_conv_weight(w), dt)
        routes = {'s2d': lambda: ops.conv2d(ops.space_to_depth2(x, dt), w4, b, gn_stats=True),
                  'strided': lambda: ops.conv2d(x, w1, b, stride=2, gn_stats=True)}
        plans = {'s2d': ops.conv_plan(ops.space_to_depth2(x, dt), w4, b, gn_stats=True), 'strided': ops.conv_plan(x, w1, b, stride=2, gn_stats=True)}
        times = {r: [] for r in routes}
        for it in range(max(a.warmup, 3) + a.iters):
            for r, f in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                y = f()
                e1.record()
                torch.cuda.synchronize()
                if it >= max(a.warmup, 3):
                    times[r].append(e0.elapsed_time(e1) * 1e3)
        ys = {r: f() for r, f in routes.items()}
        out[f'{hw}x{hw}x{c}'] = {r: {'us_median': round(statistics.median(v), 1), 'us_min': round(min(v), 1), 'us_max': round(max(v), 1),
                                     'plan': {k: plans[r][k] for k in ('kernel', 'tile', 'waves', 'stages', 'splits', 'ks_per_split', 'nblk')}}
                                 for r, v in times.items()}
        out[f'{hw}x{hw}x{c}']['median_ratio_strided_to_s2d'] = round(statistics.median(times['strided']) / statistics.median(times['s2d']), 4)
        out[f'{hw}x{hw}x{c}']['rel_max_diff'] = float((ys['strided'].float() - ys['s2d'].float()).abs().max() / ys['s2d'].float().abs().max())
    return out


def head_dims_table(a, res, sd, x32, c2, key='head_dims'):
    """--head-dims / --downsample: the listed modes of that SDUNet keyword against each other, alternating forward by forward through graph
    replay with context_rows="""
    modes = getattr(a, key).split(',')
    res['what'] += f'; {key} modes alternating, graph replay, context_rows='
    res[key] = modes
    for name in a.dtypes.split(','):
        dt = {'f16': torch.float16, 'bf16': torch.bfloat16}[name]
        x = x32.to('cuda', dt)
        t = torch.tensor(501, device='cuda')
        ctx = c2.to('cuda', dt).contiguous()
        rmap = torch.tensor([0] * (a.rows // 2) + [1] * (a.rows - a.rows // 2), dtype=torch.int32).to('cuda')
        unets = {m: SDUNet(sd, device='cuda', dtype=dt, **{key: m}) for m in modes}
        run = lambda u: u(x, t, encoder_hidden_states=ctx, context_rows=rmap)[0]
        for _ in range(max(a.warmup, 3)):
            outs = {m: run(u) for m, u in unets.items()}
        torch.cuda.synchronize()
        for m, u in unets.items():
            assert u._graphs.captures == 1 and u._graphs.replays > 0, (m, u._graphs.path_report())
        times = {m: [] for m in modes}
        for _ in range(a.iters):
            for m, u in unets.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                outs[m] = run(u)
                e1.record()
                torch.cuda.synchronize()
                times[m].append(e0.elapsed_time(e1))
        stat = lambda v: {'ms_median': round(statistics.median(v), 3), 'ms_min': round(min(v), 3), 'ms_max': round(max(v), 3)}
        base = outs[modes[0]].float()
        res['dtypes'][name] = {'replay_context_rows': {m: stat(v) for m, v in times.items()},
                               'median_ratio_to_' + modes[0]: {m: round(statistics.median(times[m]) / statistics.median(times[modes[0]]), 4) for m in modes},
                               'rel_max_diff_to_' + modes[0]: {m: float((outs[m].float() - base).abs().max() / base.abs().max()) for m in modes},
                               'attention_channels': {m: sorted({A.hp for A in u._tfm}) for m, u in unets.items()},
                               'output_finite': all(bool(torch.isfinite(o).all()) for o in outs.values())}
        if key == 'downsample':
            res['dtypes'][name]['downsampler_cin'] = {m: [d[0].shape[3] for _, d in u.down[:3]] for m, u in unets.items()}
            res['dtypes'][name]['downsample_layers'] = downsample_layers(a, dt)
        del unets
        torch.cuda.empty_cache()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=32)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dtypes', default='f16,bf16')
    ap.add_argument('--replay-only', type=int, default=0, help='only this many replayed context_rows forwards after the warm-up (for a kernel trace)')
    ap.add_argument('--head-dims', default='', help="e.g. padded,native: time these SDUNet head_dims modes against each other (see the module docstring)")
    ap.add_argument('--downsample', default='', help="e.g. s2d,strided: time these SDUNet downsample modes against each other, and the three downsample launches alone")
    ap.add_argument('--replay-head-dims', default='padded', choices=['padded', 'native'], help='the head_dims mode of the --replay-only model')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('sd_unet_bench: needs a GPU (no CPU fallback, nothing is measured without one)')
    per_row, ctx = forward_flops()
    flops = a.rows * per_row + ctx
    sd = dinit.sd_unet_state_dict(seed=0)
    g = torch.Generator().manual_seed(0)
    res = {'what': 'SDUNet forward, SD-1.5 configuration, random-init weights', 'rows': a.rows, 'latent': [4, 64, 64], 'context': [77, 768],
           'distinct_contexts': 2, 'algorithmic_flops_per_forward': flops, 'algorithmic_flops_per_row': per_row,
           'peak_flops_16bit_dense': PEAK_16BIT_DENSE, 'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'warmup': a.warmup, 'dtypes': {}}
    x32 = torch.randn(a.rows, 4, 64, 64, generator=g)
    c2 = torch.randn(2, 77, 768, generator=g)
    if a.head_dims:
        return head_dims_table(a, res, sd, x32, c2)
    if a.downsample:
        return head_dims_table(a, res, sd, x32, c2, key='downsample')
    for name in a.dtypes.split(','):
        dt = {'f16': torch.float16, 'bf16': torch.bfloat16}[name]
        unet = SDUNet(sd, device='cuda', dtype=dt, head_dims=a.replay_head_dims if a.replay_only else 'padded')
        x = x32.to('cuda', dt)
        ehs = torch.cat([c2[:1].expand(a.rows // 2, -1, -1), c2[1:].expand(a.rows - a.rows // 2, -1, -1)]).to('cuda', dt).contiguous()
        t = torch.tensor(501, device='cuda')
        ctx = c2.to('cuda', dt).contiguous()
        rmap = torch.tensor([0] * (a.rows // 2) + [1] * (a.rows - a.rows // 2), dtype=torch.int32).to('cuda')
        forms = {'stock': lambda: unet(x, t, encoder_hidden_states=ehs)[0],
                 'context_rows': lambda: unet(x, t, encoder_hidden_states=ctx, context_rows=rmap)[0]}
        for _ in range(max(a.warmup, 3)):                  # both forms have the same shapes, hence one graph: captured on the third call
            for f in forms.values():
                out = f()
        torch.cuda.synchronize()
        assert unet._graphs.captures == 1 and unet._graphs.replays > 0, unet._graphs.path_report()
        if a.replay_only:
            for _ in range(a.replay_only):
                out = forms['context_rows']()
            torch.cuda.synchronize()
            res['dtypes'][name] = {'replay_only_forwards': a.replay_only, 'path': unet._graphs.path_report()}
            del unet
            torch.cuda.empty_cache()
            continue
        times = {(mode, form): [] for mode in ('eager', 'replay') for form in forms}
        outs = {}
        for _ in range(a.iters):
            for mode in ('eager', 'replay'):
                unet._graphs.enabled = mode == 'replay'
                for form, f in forms.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = f()
                    e1.record()
                    torch.cuda.synchronize()
                    times[mode, form].append(e0.elapsed_time(e1))
                    outs[mode, form] = out
        same = all(torch.equal(o, outs['eager', 'stock']) for o in outs.values())
        unet._graphs.enabled = False                       # the per-op spans need the ops.* calls of an eager forward
        shares, _, launches = op_shares(FAMILY, lambda: unet(x, t, encoder_hidden_states=ehs))
        unet._graphs.enabled = True
        ms = statistics.median(times['eager', 'stock'])
        stat = lambda v: {'ms_median': round(statistics.median(v), 3), 'ms_min': round(min(v), 3), 'ms_max': round(max(v), 3)}
        res['dtypes'][name] = {'ms_per_forward': round(ms, 3), 'ms_min': round(min(times['eager', 'stock']), 3), 'ms_max': round(max(times['eager', 'stock']), 3),
                               'rows_per_s': round(a.rows / ms * 1e3, 1), 'tflops_algorithmic': round(flops / ms / 1e9, 1),
                               'fraction_of_dense_16bit_peak_end_to_end': round(flops / (ms * 1e-3) / PEAK_16BIT_DENSE, 4),
                               'eager': {form: stat(times['eager', form]) for form in forms},
                               'replay': {form: stat(times['replay', form]) for form in forms},
                               'replay_rows_per_s_context_rows': round(a.rows / statistics.median(times['replay', 'context_rows']) * 1e3, 1),
                               'all_four_outputs_bit_identical': bool(same), 'path': unet._graphs.path_report(), 'grouping': grouping(ehs),
                               'time_share_by_op_family': shares, 'op_calls_per_forward': launches, 'output_finite': bool(torch.isfinite(out).all())}
        del unet
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
