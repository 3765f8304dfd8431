"""Thin tensor-level wrappers over the C ABI (include/dts.h).  PyTorch supplies device memory and the
current HIP stream; every computation happens in libdts_hip.so.  Inputs must live on the GPU: there is
no CPU path here (the CPU restatement lives in oracle/ and is test infrastructure only).

Activation tensors are NHWC: shape [n, h, w, c], contiguous, dtype float32 / bfloat16 / float16.
"""
import ctypes as C
import math
import os

import torch

from . import _lib as L

_DT = {torch.float32: L.DTS_F32, torch.bfloat16: L.DTS_BF16, torch.float16: L.DTS_F16}

# The split-precision compute mode (dts.h DTS_F16X3), the DEFAULT of every surface that takes a compute dtype: activations are float32
# tensors and every kernel but the convolutions (and the d = 64 attention) is the float32 (parity-mode) one; the convolutions -- 99.9 % of
# the FLOPs -- run on the 16-bit matrix cores over the f16 split image of their input (per 32 channels: hi | lo * 2^11) against weights
# packed per 32 input channels as hi | lo, three MFMAs per staged K step (hi.hi, lo.hi, hi.lo), f32 accumulate: ~2^-22 products instead
# of f16's 2^-11, at a third of the f16 rate instead of the f32 matrix instruction's sixteenth.
F16X3 = 'f16x3'


def act_dtype(dtype):
    """storage type of the activations of a network computing in `dtype`"""
    return torch.float32 if dtype == F16X3 else dtype


def dtype_name(dtype):
    return dtype if isinstance(dtype, str) else {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}[dtype]


class X3Weight:
    """A conv weight packed for the split-precision mode: `packed` [O][kh][kw][2*I] float16 = per 32 input channels hi(32) | lo(32) of
    w * 2^k (k chosen per layer so that 2^13 < max|w| * 2^k <= 2^14: the lo parts of all weights that matter are normal f16 numbers;
    the matrix cores flush subnormal inputs), `acc_scale` = 2^-k.  The kernels scale the hi fragment by 2^-11 in registers where it meets
    the activations' lo * 2^11 half.  `phases` (pack_conv_weight(.., up_phases=True), else None): the same 3x3 layer under a nearest 2x
    upsample as four 2x2 weights [4][O][2][2][2*I] in the same form, with their own `phase_acc_scale` (dts.h: dts_conv_args.up == 2)."""

    def __init__(self, packed, acc_scale, shape):
        self.packed, self.acc_scale, self.shape = packed, float(acc_scale), tuple(shape)
        self.device, self.dtype = packed.device, F16X3
        self.phases, self.phase_acc_scale = None, 0.0

    def numel(self):
        return self.packed.numel()


class SplitQKV:
    """The qkv projection's result in the split-precision attention's operand form: `data` float16 [n,t,6*C] = hi(3C) | lo(3C) of the
    values * 2^6 (dts_split2_f16's image, written by conv2d(..., out_split2=True)); `shape` is the logical [n, h, w, 3*C]."""

    def __init__(self, data, shape):
        self.data, self.shape = data, tuple(shape)
        self.device, self.dtype = data.device, torch.float32

    def view(self, n, t, c3):
        return SplitQKV(self.data.view(n, t, 2 * c3), (n, t, c3))

    def numel(self):                     # logical elements; each is an f16 pair = 4 bytes, like the f32 value it stands for
        return self.data.numel() // 2

    def element_size(self):
        return 4


class SplitAct:
    """An activation already in the split-precision operand form: `data` float16 [n,h,w,2*C], per 32 channels hi(32) | lo * 2^11 (32)
    (dts_split3_f16 / dts_gn_apply_x3 / dts_attention_x3); `shape` is the logical NHWC shape.  Only convolutions with an X3Weight read it."""

    def __init__(self, data, c):
        self.data, self.shape = data, tuple(data.shape[:3]) + (c,)
        self.device, self.dtype = data.device, torch.float32

    def numel(self):
        return self.data.numel() // 2

    def planes(self):
        """(hi, lo * 2^11) as two float16 tensors of the logical shape (tests / debugging)"""
        return split_planes(self.data, self.shape[-1])


def split_planes(data, c):
    """the two halves of a split-precision operand image `data` [..., 2*c] as tensors [..., c]: (hi, lo * 2^11)"""
    v = data.reshape(*data.shape[:-1], c // 32, 2, 32)
    return v[..., 0, :].reshape(*data.shape[:-1], c), v[..., 1, :].reshape(*data.shape[:-1], c)


def dt_code(dtype):
    try:
        return _DT[dtype]
    except KeyError:
        raise ValueError(f'unsupported activation dtype {dtype}')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t, name='tensor', dtype=None):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f'{name} must be a GPU tensor (the HIP path has no CPU fallback)')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f'{name}: expected {dtype}, got {t.dtype}')
    return t.data_ptr()


def _rows(t, name, dtype):
    """(pointer, leading dimension) of a 2-D row-major view whose rows may be strided (a column slice)."""
    if t is None:
        return None, 0
    if not t.is_cuda:
        raise RuntimeError(f'{name} must be a GPU tensor (the HIP path has no CPU fallback)')
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype != dtype:
        raise ValueError(f'{name}: expected a 2-D {dtype} view with unit inner stride')
    return t.data_ptr(), t.stride(0)


def _call(name, *args):
    lib = L.load()
    L.check(getattr(lib, name)(*args, _stream()), name)


# ---- layout / packing ---------------------------------------------------------------------------
def nchw_to_nhwc(x, dtype):
    n, c, h, w = x.shape
    out = torch.empty((n, h, w, c), dtype=dtype, device=x.device)
    _call('dts_nchw_to_nhwc', _ptr(x, 'x', torch.float32), _ptr(out), dt_code(dtype), n, c, h, w)
    return out


def nchw_to_nhwc_pad(x, dtype, cpad):
    """f32 NCHW [n,c,h,w] -> NHWC [n,h,w,cpad] in `dtype`, channels c.. zero."""
    n, c, h, w = x.shape
    out = torch.empty((n, h, w, cpad), dtype=dtype, device=x.device)
    _call('dts_nchw_to_nhwc_pad', _ptr(x, 'x', torch.float32), _ptr(out), dt_code(dtype), n, c, h, w, cpad)
    return out


def nhwc_to_nchw(x):
    n, h, w, c = x.shape
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    _call('dts_nhwc_to_nchw', _ptr(x), dt_code(x.dtype), _ptr(out), n, c, h, w)
    return out


def _x3_split_pack(w_ohwi):
    """float32 [O][kh][kw][I] -> (packed float16 [O][kh][kw][2*I] = per 32 input channels hi(32) | lo(32) of w * 2^k, 2^-k): exact scaling by
    the power of two that puts max|w| in (2^13, 2^14], two roundings"""
    O, kh, kw, I = w_ohwi.shape
    amax = float(w_ohwi.abs().max())
    k = 0 if amax == 0.0 else max(-24, min(24, int(math.floor(math.log2(16384.0 / amax)))))
    ws = (w_ohwi * (2.0 ** k)).contiguous()                                # exact (power of two)
    hi = ws.to(torch.float16)
    lo = (ws - hi.to(torch.float32)).to(torch.float16)
    packed = torch.stack([hi.view(O, kh, kw, I // 32, 32), lo.view(O, kh, kw, I // 32, 32)], dim=-2)      # [.., I/32, 2, 32]: hi(32) | lo(32)
    return packed.reshape(O, kh, kw, 2 * I).contiguous(), 2.0 ** -k


# rows of a 3x3 kernel that fall on the two low-resolution rows an output row of parity py sees under a nearest 2x upsample:
# UP_PHASE_ROWS[py][ty][kh], tap ty at the low-resolution offset ty - 1 + py (py = 0: {w0, w1 + w2}; py = 1: {w0 + w1, w2}); columns alike
UP_PHASE_ROWS = (((1, 0, 0), (0, 1, 1)), ((1, 1, 0), (0, 0, 1)))


def up_phase_weights(w):
    """OIHW 3x3 weight -> [4][O][2][2][I] in w's dtype: conv2d(nearest_up2(x), w, padding=1) as four 2x2 convolutions over x, one per output
    phase 2*py + px; the tap sums are formed in float64 and rounded once."""
    R = torch.tensor(UP_PHASE_ROWS, dtype=torch.float64, device=w.device)            # [p][t][k]
    ph = torch.einsum('ayh,bxw,oihw->aboyxi', R, R, w.to(torch.float64))              # [py][px][O][ty][tx][I]
    O, I = w.shape[:2]
    return ph.reshape(4, O, 2, 2, I).to(w.dtype)


def pack_conv_weight(w, dtype, out_perm=None, up_phases=False):
    """OIHW float32 (device) -> [O][kh][kw][I] in `dtype`; out_perm: int32 device tensor of source rows.
    up_phases (F16X3, 3x3): the X3Weight also carries `phases` [4][O][2][2][2*I] (the four 2x2 weights of up_phase_weights(), split and
    interleaved like `packed`, scaled by their own power of two: `phase_acc_scale`) for conv2d(..., up=True)."""
    if w.dim() == 3:                      # conv1d weight [O, I, 1]
        w = w.unsqueeze(-1)
    w = w.contiguous()
    O, I, kh, kw = w.shape
    if up_phases and (dtype != F16X3 or (kh, kw) != (3, 3)):
        raise ValueError('pack_conv_weight: up_phases is the split-precision mode\'s, for 3x3 weights')
    if dtype == F16X3:                    # load-time preparation in float32 on the device: exact scaling, two roundings
        wp = w if out_perm is None else w[out_perm.long()]
        if I % 32:
            raise ValueError(f'pack_conv_weight(F16X3): {I} input channels are not a multiple of 32 (one K step of the split image)')
        packed, acc_scale = _x3_split_pack(wp.permute(0, 2, 3, 1))         # [O][kh][kw][I]
        xw = X3Weight(packed, acc_scale, (O, kh, kw, I))
        if up_phases:
            pp, xw.phase_acc_scale = _x3_split_pack(up_phase_weights(wp).reshape(4 * O, 2, 2, I))
            xw.phases = pp.reshape(4, O, 2, 2, 2 * I)
        return xw
    out = torch.empty((O, kh, kw, I), dtype=dtype, device=w.device)
    _call('dts_pack_conv_weight', _ptr(w, 'w', torch.float32), _ptr(out), dt_code(dtype), O, I, kh, kw,
          _ptr(out_perm, 'perm', torch.int32))
    return out


# ---- convolution --------------------------------------------------------------------------------
_CONV_WS = {}
CONV_WS_BYTES = 96 << 20        # split-K scratch per device (covers 8 splits of the 8x8 / 16x16 ADM levels at N=64)


def _conv_workspace(device):
    key = (device.type, device.index)
    ws = _CONV_WS.get(key)
    if ws is None:
        ws = _CONV_WS[key] = torch.empty(CONV_WS_BYTES, dtype=torch.uint8, device=device)
    return ws


def _conv_args(x1, w, x2, up, stride=1):
    n, hin, win, c1 = x1.shape
    a = L.ConvArgs()
    a.c1, a.c2 = c1, 0 if x2 is None else x2.shape[-1]
    a.n, a.hin, a.win, a.cout, a.ksize = n, hin, win, w.shape[0], w.shape[1]
    a.up, a.dtype = _up_field(up, stride), dt_code(x1.dtype)
    return a


def _up_field(up, stride):
    """dts_conv_args.up of conv2d(up=, stride=): 0 / 1, or -1 for stride 2 (which takes no upsample)"""
    if stride not in (1, 2):
        raise ValueError(f'conv2d: stride {stride!r} (1 or 2)')
    if stride == 2 and up:
        raise ValueError('conv2d: stride=2 takes no up=True')
    return -1 if stride == 2 else int(up)


def conv_kernel(x1, w, x2=None, up=False, residual=None, gn_coef=None, gn_stats=False, stride=1):
    """Which kernel ops.conv2d launches for these arguments: 0 = 4-wave implicit GEMM (its phase and stride-2 forms included), 6 / 4 = ping-pong
    kernel with 192- / 128-cout blocks (dts_conv_kernel; measurement aid for bench.py)."""
    a = _conv_args(x1, w, x2, up, stride)
    if isinstance(w, X3Weight):           # the launch sees one 16-bit source of 2*(c1+c2) channels
        a.c1, a.c2, a.dtype = 2 * (a.c1 + a.c2), 0, L.DTS_F16X3
    a.residual = _ptr(residual)
    a.gn_coef = _ptr(gn_coef, 'gn_coef', torch.float32)
    if up and x2 is None and getattr(w, 'phases', None) is not None:
        # as conv2d routes it (pointers are never dereferenced by the queries: presence is all that counts)
        a.workspace, a.workspace_bytes = 16, CONV_WS_BYTES
        if gn_stats and (4 * a.hin * a.win) % 64 == 0:
            a.stats_out = 16
        _route_phases(a, w, None)
    return int(L.load().dts_conv_kernel(C.byref(a)))


def _route_phases(a, w, phases):
    """conv2d(.., up=True) with a weight that carries phase-packed tensors: the dts_conv_args become the phase form's (up = 2, the four 2x2
    weights and their power of two) where dts_conv_takes_phases says yes (phases=None), always (True: the library refuses what it cannot
    run) or never (False); returns whether they did."""
    if phases is False or getattr(w, 'phases', None) is None or a.up != 1:
        return False
    keep = (a.up, a.w, a.acc_scale)
    a.up, a.w, a.acc_scale = 2, (w.phases.data_ptr() if w.phases.is_cuda else None), w.phase_acc_scale
    if phases is None and not L.load().dts_conv_takes_phases(C.byref(a)):
        a.up, a.w, a.acc_scale = keep
        return False
    return True


def conv_takes_phases(x1, w, bias=None, **kw):
    """True if conv2d(same arguments, up=True) runs the phase form: the 3x3 convolution over the nearest-2x upsampled input as four 2x2
    convolutions over the input itself (dts_conv_takes_phases; `w` packed with up_phases=True)."""
    kw.pop('up', None)
    a, *_keep = _conv2d_args(x1, w, bias, up=True, **kw)
    return a.up == 2


def conv_fuses_gn(x1, w, *, x2=None, up=False):
    """True if conv2d(x1, w, ..., gn_coef=...) applies the GroupNorm of its input inside the kernel for this shape / dtype
    (the ping-pong / halo kernel: 3x3, cout % 192 == 0, 16-bit, square power-of-two images >= 16, no fused upsample)."""
    return bool(L.load().dts_conv_fuses_gn(C.byref(_conv_args(x1, w, x2, up))))


def _skip_fields(a, skip, n, ho, wo, cout):
    """dts_conv_args.skip_*: skip = (SplitAct of the block input, X3Weight of the 1x1 layer, up)"""
    src, sw, sup = skip
    if not isinstance(src, SplitAct) or not isinstance(sw, X3Weight):
        raise ValueError('conv2d: skip = (SplitAct, X3Weight, up)')
    sh = (n, ho // 2, wo // 2) if sup else (n, ho, wo)
    if tuple(src.shape[:3]) != sh or tuple(sw.shape) != (cout, 1, 1, src.shape[3]):
        raise ValueError(f'conv2d: skip source {tuple(src.shape)} / weight {tuple(sw.shape)} do not match an output of {(n, ho, wo, cout)} (up={bool(sup)})')
    a.skip_c, a.skip_x, a.skip_w = src.data.shape[-1], _ptr(src.data, 'skip_x', torch.float16), _ptr(sw.packed, 'skip_w', torch.float16)
    a.skip_acc_scale, a.skip_up = sw.acc_scale, int(bool(sup))


def conv_folds_skip(x1, w, skip):
    """True if conv2d(x1, w, bias, skip=skip) accumulates the block's 1x1 skip convolution inside this 3x3 launch (dts_conv_folds_skip:
    split-precision mode, ping-pong kernel, a grid that needs no K split); skip = (SplitAct of the block input, its X3Weight, up)."""
    if not isinstance(w, X3Weight) or skip is None or not isinstance(skip[0], SplitAct):
        return False
    a = _conv_args(x1, w, None, False)
    a.c1, a.c2, a.dtype = 2 * a.c1, 0, L.DTS_F16X3
    _skip_fields(a, skip, a.n, a.hin, a.win, a.cout)
    return bool(L.load().dts_conv_folds_skip(C.byref(a)))


def _conv2d_args(x1, w, bias=None, *, x2=None, bias_nc=None, residual=None, up=False, out_scale=1.0, out=None, gn_stats=False,
                 timing_events=None, gn_coef=None, gn_silu=True, out_split2=False, skip=None, phases=None, stride=1):
    """the dts_conv_args of conv2d(...) (and of conv_plan(...): one builder, so the two cannot differ): (args, out, statistics buffer or None,
    out_split2, tensors the arguments point into)"""
    n, hin, win, c1 = x1.shape
    c2 = 0 if x2 is None else x2.shape[-1]
    cout, kh, kw, cin = w.shape
    if cin != c1 + c2 or kh != kw:
        raise ValueError(f'conv2d: weight {tuple(w.shape)} does not match inputs ({c1}+{c2})')
    up_field = _up_field(up, stride)
    x3 = isinstance(w, X3Weight)
    if stride == 2:         # the 16-bit 3x3 form alone (dts.h: dts_conv_args.up == -1); refused here, before the library is called
        for given, what in ((gn_coef is not None, 'gn_coef'), (skip is not None, 'skip'), (out_split2, 'out_split2'), (x3, 'a split-precision weight'),
                            (x1.dtype == torch.float32, 'float32 activations'), (kh != 3, f'a {kh}x{kh} weight')):
            if given:
                raise ValueError(f'conv2d: stride=2 takes no {what}')
    ho, wo = ((hin + 1) // 2, (win + 1) // 2) if stride == 2 else (2 * hin, 2 * win) if up else (hin, win)
    if x3 and (x1.dtype != torch.float32 or gn_coef is not None):
        raise ValueError('conv2d: a split-precision weight takes float32 activations (and no fused input GroupNorm)')
    if isinstance(x1, SplitAct) and (not x3 or x2 is not None):
        raise ValueError('conv2d: a split activation feeds a split-precision weight, alone')
    out_split2 = bool(out_split2) and x3 and not gn_stats       # (split-precision mode only: the qkv projection feeding attention(x3=True))
    if out_split2:
        out = torch.empty((n, ho, wo, 2 * cout), dtype=torch.float16, device=x1.device)
    elif out is None:
        out = torch.empty((n, ho, wo, cout), dtype=x1.dtype, device=x1.device)
    a, xs = L.ConvArgs(), None
    a.out_split2 = int(out_split2)
    dt_in = x1.dtype
    if x3:      # the conv reads the f16 split image (per 32 channels hi | lo) of concat(x1, x2); epilogue operands and output stay float32
        xs = x1.data if isinstance(x1, SplitAct) else split3_f16(x1, x2)
        a.x1, a.c1, a.x2, a.c2 = _ptr(xs, 'x1', torch.float16), 2 * (c1 + c2), None, 0
        a.w, a.acc_scale = _ptr(w.packed, 'w', torch.float16), w.acc_scale
    else:
        a.x1, a.c1 = _ptr(x1, 'x1'), c1
        a.x2, a.c2 = _ptr(x2, 'x2', x1.dtype), c2
        a.w = _ptr(w, 'w', x1.dtype)
    a.bias = _ptr(bias, 'bias', torch.float32)
    a.bias_nc, a.ld_bias_nc = _rows(bias_nc, 'bias_nc', x1.dtype)
    a.residual = _ptr(residual, 'residual', x1.dtype)
    if residual is not None and tuple(residual.shape) != (n, ho, wo, cout):
        raise ValueError(f'conv2d: residual shape {tuple(residual.shape)} != {(n, ho, wo, cout)}')
    a.out = _ptr(out, 'out', torch.float16 if out_split2 else x1.dtype)
    a.n, a.hin, a.win, a.cout, a.ksize = n, hin, win, cout, kh
    a.up, a.out_scale, a.dtype = up_field, float(out_scale), (L.DTS_F16X3 if x3 else dt_code(x1.dtype))
    ws = _conv_workspace(x1.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    st = None
    if gn_stats and (ho * wo) % 64 == 0:
        st = torch.empty(((n * ho * wo) // 64, cout, 2), dtype=torch.float32, device=x1.device)
        a.stats_out = st.data_ptr()
    if timing_events is not None:
        a.ev_start, a.ev_stop = timing_events
    if skip is not None:
        if not x3 or residual is not None or up:
            raise ValueError('conv2d: skip= is the split-precision mode\'s, without residual / upsample')
        _skip_fields(a, skip, n, ho, wo, cout)
    if gn_coef is not None:       # GroupNorm (+SiLU) of the input applied on the staged tile: only where conv_fuses_gn() says so
        if tuple(gn_coef.shape) != (n, c1 + c2, 2):
            raise ValueError(f'conv2d: gn_coef shape {tuple(gn_coef.shape)} != {(n, c1 + c2, 2)}')
        a.gn_coef, a.gn_silu = _ptr(gn_coef, 'gn_coef', torch.float32), int(gn_silu)
    if x3 and up:
        _route_phases(a, w, phases)
    return a, out, st, out_split2, (xs, ws)


def conv_plan(*args, **kw):
    """The launch plan of conv2d(same arguments) as a dict of dts_conv_plan_info's fields (kernel, tile, waves, stages, pf, gn, sk, dbg, splits,
    ks_per_split, n_ct, n_pt, nblk, threads, lds_bytes, stats_in_kernel, stats_in_reduce, stats_written, epi_rows, fuses_gn, folds_skip,
    refused, phases): what the launcher derives, nothing is launched.  Test and measurement aid."""
    a, *_keep = _conv2d_args(*args, **kw)
    info = L.ConvPlanInfo()
    _call('dts_conv_plan', C.byref(a), C.byref(info))
    return {f: int(getattr(info, f)) for f, _ in L.ConvPlanInfo._fields_}


def conv2d(x1, w, bias=None, *, x2=None, bias_nc=None, residual=None, up=False, out_scale=1.0, out=None, gn_stats=False,
           timing_events=None, gn_coef=None, gn_silu=True, out_split2=False, skip=None, phases=None, stride=1):
    """stride=2 (float16 / bfloat16, 3x3 weights): zero padding 1 and stride 2, an SD Downsample2D; the output (and a residual) is
    [n, (hin+1)//2, (win+1)//2, cout], odd sizes included, `w` the ordinary pack_conv_weight of the [C, C, 3, 3] tensor.  Not with up=True,
    gn_coef, skip, out_split2, an X3Weight or float32 activations (ValueError).
    phases (up=True with a weight packed with up_phases=True): None = the phase form where conv_takes_phases() says so, False = never,
    True = always (the library refuses what it cannot run).
    skip=(SplitAct, X3Weight, up): the block's 1x1 skip convolution of that operand accumulated by this launch (only where conv_folds_skip()
    says so; `bias` is then the sum of the two layers' biases and there is no `residual`).
    timing_events=(start, stop): raw hipEvent_t handles attached to the conv kernel's own dispatch (measurement only).
    gn_stats=True: the epilogue also emits the GroupNorm moments of the output (per 64-pixel strip and channel); they
    ride on the returned tensor as `out._gn_stats` (None when the launch could not produce them) and are consumed by
    group_norm(), which then skips its own pass over the tensor."""
    a, out, st, out_split2, _keep = _conv2d_args(x1, w, bias, x2=x2, bias_nc=bias_nc, residual=residual, up=up, out_scale=out_scale, out=out,
                                                 gn_stats=gn_stats, timing_events=timing_events, gn_coef=gn_coef, gn_silu=gn_silu,
                                                 out_split2=out_split2, skip=skip, phases=phases, stride=stride)
    _call('dts_conv2d', C.byref(a))
    if out_split2:
        return SplitQKV(out, (out.shape[0], out.shape[1], out.shape[2], out.shape[3] // 2))
    out._gn_stats = st if (st is not None and a.stats_written) else None
    return out


def split3_f16(x1, x2=None):
    """float32 NHWC [n,h,w,c1] (+ [n,h,w,c2]) -> float16 [n,h,w,2*(c1+c2)]: per 32 channels of the channel concat hi(32) | lo * 2^11 (32)
    (dts_split3_f16; the historical name: round 4's image had three planes)."""
    n, h, w, c1 = x1.shape
    c2 = 0 if x2 is None else x2.shape[-1]
    out = torch.empty((n, h, w, 2 * (c1 + c2)), dtype=torch.float16, device=x1.device)
    _call('dts_split3_f16', _ptr(x1, 'x1', torch.float32), c1, _ptr(x2, 'x2', torch.float32), c2, _ptr(out), n * h * w)
    return out


def split2_f16(x):
    """float32 [..., c] -> float16 [..., 2*c]: hi(c) | lo(c) of x * 2^6 per row (dts_split2_f16: the operand image of dts_attention_x3, what
    conv2d(..., out_split2=True) writes from its epilogue)"""
    c = x.shape[-1]
    out = torch.empty(tuple(x.shape[:-1]) + (2 * c,), dtype=torch.float16, device=x.device)
    _call('dts_split2_f16', _ptr(x, 'x', torch.float32), c, _ptr(out), x.numel() // c)
    return out


def _out(who, out, shape, dtype, device):
    """the output tensor of an op: a fresh one, or the caller's `out` -- a contiguous GPU tensor (_ptr checks that where it is passed on) of
    exactly this shape and type on the inputs' device -- which is then what the op returns"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not torch.is_tensor(out) or tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device:
        raise ValueError(f'{who}: out {tuple(out.shape)} {out.dtype} on {out.device} != {tuple(shape)} {dtype} on {device}'
                         if torch.is_tensor(out) else f'{who}: out is a {type(out).__name__}')
    return out


def conv_in3(x, w, bias, cout, dtype, out=None):
    """x f32 NCHW [n,3,h,w]; w f32 OIHW [cout,3,3,3] -> NHWC [n,h,w,cout] (written into `out` where given)."""
    n, c, h, wd = x.shape
    assert c == 3
    out = _out('conv_in3', out, (n, h, wd, cout), dtype, x.device)
    _call('dts_conv_in3', _ptr(x, 'x', torch.float32), _ptr(w, 'w', torch.float32), _ptr(bias, 'bias', torch.float32),
          _ptr(out, 'out', dtype), dt_code(dtype), n, h, wd, cout)
    return out


def conv_out3(x, w_ohwi, bias, out=None):
    """x NHWC [n,h,w,c]; w f32 [3,3,3,c] (O,kh,kw,I) -> f32 NCHW [n,3,h,w] (written into `out` where given)."""
    n, h, wd, c = x.shape
    out = _out('conv_out3', out, (n, 3, h, wd), torch.float32, x.device)
    _call('dts_conv_out3', _ptr(x), dt_code(x.dtype), _ptr(w_ohwi, 'w', torch.float32), _ptr(bias, 'bias', torch.float32),
          _ptr(out, 'out', torch.float32), n, h, wd, c)
    return out


# ---- group norm ---------------------------------------------------------------------------------
def gn_coef(x1, groups, eps, gamma, beta, *, x2=None, scale_shift=None):
    n, h, w, c1 = x1.shape
    c2 = 0 if x2 is None else x2.shape[-1]
    C_ = c1 + c2
    lib = L.load()
    ws = torch.empty((lib.dts_gn_ws_floats(n, groups),), dtype=torch.float32, device=x1.device)
    coef = torch.empty((n, C_, 2), dtype=torch.float32, device=x1.device)
    ss_ptr, ss_ld = _rows(scale_shift, 'scale_shift', x1.dtype)
    _call('dts_gn_coef', _ptr(x1, 'x1'), c1, _ptr(x2, 'x2', x1.dtype), c2, dt_code(x1.dtype), n, h * w, groups, float(eps),
          _ptr(gamma, 'gamma', torch.float32), _ptr(beta, 'beta', torch.float32), ss_ptr, ss_ld, _ptr(coef), _ptr(ws))
    return coef


def gn_apply(x1, coef, *, x2=None, silu=True, pool=False, split_out=False, raw_split=False):
    """split_out (float32 inputs only): the result leaves as the f16 split image a split-precision convolution reads (SplitAct).
    raw_split (with split_out): returns (normalised image, image of the un-normalised [2x2-averaged if pool] input) from the one pass."""
    n, h, w, c1 = x1.shape
    c2 = 0 if x2 is None else x2.shape[-1]
    ho, wo = (h // 2, w // 2) if pool else (h, w)
    if split_out:
        out = torch.empty((n, ho, wo, 2 * (c1 + c2)), dtype=torch.float16, device=x1.device)
        raw = torch.empty_like(out) if raw_split else None
        _call('dts_gn_apply_x3', _ptr(x1, 'x1', torch.float32), c1, _ptr(x2, 'x2', torch.float32), c2, _ptr(coef, 'coef', torch.float32),
              _ptr(out), _ptr(raw), n, h, w, int(silu), int(pool))
        return (SplitAct(out, c1 + c2), SplitAct(raw, c1 + c2)) if raw_split else SplitAct(out, c1 + c2)
    out = torch.empty((n, ho, wo, c1 + c2), dtype=x1.dtype, device=x1.device)
    _call('dts_gn_apply', _ptr(x1, 'x1'), c1, _ptr(x2, 'x2', x1.dtype), c2, dt_code(x1.dtype),
          _ptr(coef, 'coef', torch.float32), _ptr(out), n, h, w, int(silu), int(pool))
    return out


GN_FUSED_MAX_HW = 64        # 8x8 levels take the single-launch kernel (measured: tools/gn_bench.py; larger levels are bandwidth-bound)


def _coef_from_strips(x1, x2, groups, eps, gamma, beta, scale_shift):
    """coef [n, C, 2] from the strip statistics the producing convolutions attached to x1 (and x2), or None."""
    n, h, w, c1 = x1.shape
    c2 = 0 if x2 is None else x2.shape[-1]
    st1 = getattr(x1, '_gn_stats', None)
    st2 = None if x2 is None else getattr(x2, '_gn_stats', None)
    if st1 is None or (x2 is not None and st2 is None) or (h * w) % 64 != 0:
        return None
    coef = torch.empty((n, c1 + c2, 2), dtype=torch.float32, device=x1.device)
    ss_ptr, ss_ld = _rows(scale_shift, 'scale_shift', x1.dtype)
    _call('dts_gn_coef_strips', _ptr(st1, 'st1', torch.float32), c1, _ptr(st2, 'st2', torch.float32), c2, dt_code(x1.dtype), n,
          h * w, groups, float(eps), _ptr(gamma, 'gamma', torch.float32), _ptr(beta, 'beta', torch.float32), ss_ptr, ss_ld,
          _ptr(coef))
    return coef


def gn_coefficients(x1, groups, eps, gamma, beta, *, x2=None, scale_shift=None):
    """The GroupNorm of concat(x1, x2) as per-(sample, channel) coefficients (a, b): norm(x)*gamma+beta [*(1+scale)+shift] == x*a+b.
    Taken from the producers' strip statistics when they are attached, else from a statistics pass over the tensor.  What
    conv2d(..., gn_coef=) consumes when the consuming convolution applies the norm itself (conv_fuses_gn)."""
    coef = _coef_from_strips(x1, x2, groups, eps, gamma, beta, scale_shift)
    return coef if coef is not None else gn_coef(x1, groups, eps, gamma, beta, x2=x2, scale_shift=scale_shift)


def group_norm(x1, groups, eps, gamma, beta, *, x2=None, scale_shift=None, silu=True, pool=False, path=None, split_out=False, raw_split=False):
    """GroupNorm [+ (1+scale), shift] [+ SiLU] [+ 2x2 average pool].  path: None = auto, 'fused' | 'split' (tests).
    split_out: float32 in, SplitAct out (the operand form of a split-precision convolution); raw_split (with split_out): a pair, see gn_apply."""
    n, h, w, c1 = x1.shape
    c2 = 0 if x2 is None else x2.shape[-1]
    cg = (c1 + c2) // groups
    fused_ok = (not pool) and cg % 2 == 0 and cg <= 64
    if path in (None, 'strips'):
        coef = _coef_from_strips(x1, x2, groups, eps, gamma, beta, scale_shift)
        if coef is not None:
            return gn_apply(x1, coef, x2=x2, silu=silu, pool=pool, split_out=split_out, raw_split=raw_split)
    if path == 'strips':
        raise ValueError('strip statistics are not attached to the input(s)')
    if path is None:
        path = 'fused' if (fused_ok and h * w <= GN_FUSED_MAX_HW and not split_out) else 'split'
    if path == 'fused':
        if not fused_ok:
            raise ValueError('fused GroupNorm needs pool=False and an even number (<= 64) of channels per group')
        out = torch.empty((n, h, w, c1 + c2), dtype=x1.dtype, device=x1.device)
        ss_ptr, ss_ld = _rows(scale_shift, 'scale_shift', x1.dtype)
        _call('dts_gn_fused', _ptr(x1, 'x1'), c1, _ptr(x2, 'x2', x1.dtype), c2, dt_code(x1.dtype), n, h * w, groups, float(eps),
              _ptr(gamma, 'gamma', torch.float32), _ptr(beta, 'beta', torch.float32), ss_ptr, ss_ld, _ptr(out), int(silu))
        return out
    return gn_apply(x1, gn_coef(x1, groups, eps, gamma, beta, x2=x2, scale_shift=scale_shift), x2=x2, silu=silu, pool=pool,
                    split_out=split_out, raw_split=raw_split)


def resample2x(x, up):
    n, h, w, c = x.shape
    ho, wo = (2 * h, 2 * w) if up else (h // 2, w // 2)
    out = torch.empty((n, ho, wo, c), dtype=x.dtype, device=x.device)
    _call('dts_resample2x', _ptr(x), _ptr(out), dt_code(x.dtype), n, h, w, c, int(up))
    return out


FIR_TAPS = (1, 3, 3, 1)       # the NCSN++ resampling filter (SongUNet resample_filter=[1,3,3,1]); per axis, before normalisation


def resample_fir(x, up, split_out=False):
    """2x down / up sampling with the [1,3,3,1] filter (dts_resample_fir): conv2d(x, F, stride 2, padding 1) / conv_transpose2d(x, 4F, stride 2,
    padding 1) per channel, F = outer(k, k) / 64.  split_out (float32 input): the result leaves as a split-precision convolution's operand (SplitAct)."""
    n, h, w, c = x.shape
    ho, wo = (2 * h, 2 * w) if up else (h // 2, w // 2)
    if split_out:
        out = torch.empty((n, ho, wo, 2 * c), dtype=torch.float16, device=x.device)
        _call('dts_resample_fir', _ptr(x, 'x', torch.float32), _ptr(out), L.DTS_F32, n, h, w, c, int(up), 1)
        return SplitAct(out, c)
    out = torch.empty((n, ho, wo, c), dtype=x.dtype, device=x.device)
    _call('dts_resample_fir', _ptr(x), _ptr(out), dt_code(x.dtype), n, h, w, c, int(up), 0)
    return out


def conv_cin_granule(dtype):
    """input channels of dts_conv2d come in multiples of this, per compute mode (one K step)"""
    return 32 if dtype in (F16X3, torch.float32) else 64


def space_to_depth2(x, dtype, nchw=False, cpad=None):
    """[n, h, w, c] activations (or, nchw=True, the float32 [n, c, h, w] image) -> [n, h/2, w/2, cpad]: channel (ry*2 + rx)*c + ci of output
    pixel (i, j) is input pixel (2i+ry, 2j+rx), channel ci; channels beyond 4c are zero (cpad defaults to 4c rounded up to the convolution's
    granularity in compute mode `dtype`).  In the split-precision mode the result is a SplitAct.  The operand of a fused_down_weight()."""
    if nchw:
        n, c, h, w = x.shape
    else:
        n, h, w, c = x.shape
    g = conv_cin_granule(dtype)
    cpad = -(-4 * c // g) * g if cpad is None else cpad
    x3, adt = dtype == F16X3, act_dtype(dtype)
    if x.dtype != (torch.float32 if nchw else adt):
        raise ValueError(f'space_to_depth2: input dtype {x.dtype} in compute mode {dtype_name(dtype)}')
    out = torch.empty((n, h // 2, w // 2, 2 * cpad if x3 else cpad), dtype=torch.float16 if x3 else adt, device=x.device)
    _call('dts_space_to_depth2', _ptr(x), int(nchw), _ptr(out), dt_code(adt), n, h, w, c, cpad, int(x3))
    return SplitAct(out, cpad) if x3 else out


def fused_down_weight(w, taps=FIR_TAPS, cpad=None, out_dtype=torch.float32):
    """The weight of Conv2d(kernel=3, down=True, fused_resample=True) (networks.py:78-80: conv2d(x, w, padding=2), then the depthwise filter
    F = outer(k, k) / sum(k)^2 at stride 2 without padding) as ONE 3x3 padding-1 convolution over space_to_depth2(x).

    The two linear steps compose into a 6x6 stride-2 padding-2 convolution, W6[o,c,u,v] = sum_{a,b} F[a,b] w[o,c,u-a,v-b]; with u = 2t + r its
    taps fall on the 2x2 phases r of the pixel blocks t - 1 .. t + 1, i.e. a 3x3 convolution of the 4c channels (ry, rx, c).  Composed in
    float64 from the float32 weight, rounded once to `out_dtype`.  w: [O, C, 3, 3] (any device) -> [O, cpad or 4C, 3, 3] on w's device."""
    O, Cin, kh, kw = w.shape
    if (kh, kw) != (3, 3) or len(taps) != 4:
        raise ValueError('fused_down_weight: a 3x3 weight and a 4-tap filter')
    k = torch.tensor(list(taps), dtype=torch.float64, device=w.device)
    F2 = torch.outer(k, k) / k.sum() ** 2
    w64 = w.detach().to(torch.float64)
    w6 = torch.zeros((O, Cin, 6, 6), dtype=torch.float64, device=w.device)
    for a in range(4):
        for b in range(4):
            w6[:, :, a:a + 3, b:b + 3] += F2[a, b] * w64
    # [O, C, ty, ry, tx, rx] -> [O, ry, rx, C, ty, tx]
    w3 = w6.view(O, Cin, 3, 2, 3, 2).permute(0, 3, 5, 1, 2, 4).reshape(O, 4 * Cin, 3, 3)
    cpad = 4 * Cin if cpad is None else cpad
    out = torch.zeros((O, cpad, 3, 3), dtype=out_dtype, device=w.device)
    out[:, :4 * Cin] = w3.to(out_dtype)
    return out


# ---- attention ----------------------------------------------------------------------------------
def attention(qkv, heads, scale, x3=False, split_out=False, out=None):
    """qkv [n, t, 3*heads*d] (q|k|v blocks) -> [n, t, heads*d] (dts_attention).  Head dims 64 / 128 / 256 in every dtype; 40 / 80 / 160 (the
    SD-1.x heads, stored unpadded) and 512 in float16 / bfloat16.  out (the plain kernel only): written and returned where given.  x3 (split-precision mode, float32 qkv or a SplitQKV, head dim 64): Q.K^T and
    P.V on the 16-bit matrix cores with hi/lo operand pairs (dts_attention_x3) instead of the f32 matrix instruction; same accuracy.
    split_out (with x3): the result leaves as the operand image of the proj convolution (SplitAct [n, t, 1, C])."""
    n, t, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    pre = isinstance(qkv, SplitQKV)
    if out is not None and (pre or x3 or split_out):
        raise ValueError('attention: out= goes with the plain kernel (no x3, no split_out, no SplitQKV)')
    # (short sequences stay on the f32 kernel: at T = 64 the split pass alone costs what that launch does -- tools/att_bench.py --x3)
    if pre or (x3 and d == 64 and t >= 128 and qkv.dtype == torch.float32):
        if pre:
            sp = qkv.data
        else:
            sp = torch.empty((n, t, 2 * c3), dtype=torch.float16, device=qkv.device)
            _call('dts_split2_f16', _ptr(qkv, 'qkv', torch.float32), c3, _ptr(sp), n * t)
        if split_out:
            out = torch.empty((n, t, 2 * c), dtype=torch.float16, device=qkv.device)
            _call('dts_attention_x3', _ptr(sp), _ptr(out), 1, n, t, heads, d, float(scale))
            return SplitAct(out.view(n, t, 1, 2 * c), c)
        out = torch.empty((n, t, c), dtype=torch.float32, device=qkv.device)
        _call('dts_attention_x3', _ptr(sp), _ptr(out), 0, n, t, heads, d, float(scale))
        return out
    out = _out('attention', out, (n, t, c), qkv.dtype, qkv.device)
    _call('dts_attention', _ptr(qkv), _ptr(out, 'out', qkv.dtype), dt_code(qkv.dtype), n, t, heads, d, float(scale))
    return out


def attention_masked(qkv, heads, scale, causal=True, key_len=None):
    """qkv [n, t, 3*heads*64] (q|k|v blocks; float16 / bfloat16) -> [n, t, heads*64] (dts_attention_masked): query i of sample b attends
    key j iff (not causal or j <= i) and (key_len is None or j < key_len[b]).  key_len: int32 [n] on the device with 1 <= key_len[b] <= t --
    the caller vouches for the range, it is not read back here.  causal=False with key_len=None is plain attention."""
    if qkv.dim() != 3 or heads <= 0 or qkv.shape[-1] % (3 * heads):
        raise ValueError(f'attention_masked: qkv {tuple(qkv.shape)} is not [n, t, 3 * {heads} heads * d]')
    n, t, c3 = qkv.shape
    c = c3 // 3
    if key_len is not None and (tuple(key_len.shape) != (n,) or key_len.dtype != torch.int32):
        raise ValueError(f'attention_masked: key_len {tuple(key_len.shape)} {key_len.dtype} is not int32 [{n}]')
    out = torch.empty((n, t, c), dtype=qkv.dtype, device=qkv.device)
    _call('dts_attention_masked', _ptr(qkv, 'qkv'), _ptr(out), dt_code(qkv.dtype), n, t, heads, c // heads, float(scale), int(bool(causal)),
          _ptr(key_len, 'key_len', torch.int32))
    return out


def attention_x3_masked(qkv, heads, scale, causal=True, key_len=None, split_out=False):
    """attention_masked in the split-precision mode (dts_attention_x3_masked; head dim 64, any t >= 1): qkv float32 [n, t, 3*heads*64]
    (split here by dts_split2_f16) or a SplitQKV (what conv2d(..., out_split2=True) wrote) -> float32 [n, t, heads*64], or with split_out the
    operand image of the proj convolution (SplitAct [n, t, 1, C]).  causal / key_len as attention_masked: int32 [n] on the device with
    1 <= key_len[b] <= t, vouched for by the caller.  Unlike attention(x3=True) no sequence length is routed to the float32 kernel."""
    pre = isinstance(qkv, SplitQKV)
    if not pre and not torch.is_tensor(qkv):
        raise ValueError(f'attention_x3_masked: qkv must be a float32 tensor or a SplitQKV, got {type(qkv).__name__}')
    if len(qkv.shape) != 3 or heads <= 0 or qkv.shape[-1] % (3 * heads):
        raise ValueError(f'attention_x3_masked: qkv {tuple(qkv.shape)} is not [n, t, 3 * {heads} heads * d]')
    if not pre and qkv.dtype != torch.float32:
        raise ValueError(f'attention_x3_masked: qkv must be float32 (or a SplitQKV), got {qkv.dtype}: float16 / bfloat16 take attention_masked')
    n, t, c3 = qkv.shape
    c = c3 // 3
    if key_len is not None and (not torch.is_tensor(key_len) or tuple(key_len.shape) != (n,) or key_len.dtype != torch.int32):
        raise ValueError(f'attention_x3_masked: key_len {tuple(key_len.shape) if torch.is_tensor(key_len) else type(key_len).__name__} '
                         f'{getattr(key_len, "dtype", "")} is not int32 [{n}]')
    sp = qkv.data if pre else split2_f16(qkv)
    out = torch.empty((n, t, 2 * c) if split_out else (n, t, c), dtype=torch.float16 if split_out else torch.float32, device=sp.device)
    _call('dts_attention_x3_masked', _ptr(sp, 'qkv', torch.float16), _ptr(out), int(bool(split_out)), n, t, heads, c // heads, float(scale),
          int(bool(causal)), _ptr(key_len, 'key_len', torch.int32))
    return SplitAct(out.view(n, t, 1, 2 * c), c) if split_out else out


def attention_x3_ok(t, d):
    """whether attention(..., x3=True) takes the split-precision kernel for this sequence length / head dim (so that the qkv projection may
    write its operand image directly and the proj convolution may read one)"""
    return d == 64 and t >= 128 and os.environ.get('DTS_X3_FUSE_IMAGES', '1') != '0'     # (0: A/B aid -- f32 tensors + split passes)


def cross_attention(q, kv, heads, scale, kv_rows=None, out=None):
    """q [n, tq, heads*d], kv [m, tk, 2*heads*d] (k | v blocks; 1 <= tk <= 128) -> [n, tq, heads*d] (dts_cross_attention; float16 / bfloat16;
    head dims 40 / 64 / 80 / 128 / 160 / 256, each stored at its own width).
    kv_rows: int32 [n] on the device, sample i attends to kv[kv_rows[i]] (entries in [0, m)); None: m == n, row for row.
    out: written and returned where given."""
    n, tq, c = q.shape
    m, tk, c2 = kv.shape
    if c2 != 2 * c or c % heads or (kv_rows is None and m != n) or (kv_rows is not None and tuple(kv_rows.shape) != (n,)):
        raise ValueError(f'cross_attention: q {tuple(q.shape)}, kv {tuple(kv.shape)}, {heads} heads' + ('' if kv_rows is None else f', kv_rows {tuple(kv_rows.shape)}'))
    out = _out('cross_attention', out, (n, tq, c), q.dtype, q.device)
    _call('dts_cross_attention', _ptr(q, 'q'), _ptr(kv, 'kv', q.dtype), _ptr(kv_rows, 'kv_rows', torch.int32), m, _ptr(out, 'out', q.dtype), dt_code(q.dtype),
          n, tq, tk, heads, c // heads, float(scale))
    return out


GROUP_ROWS_MAX = 1024


def group_rows(x):
    """Groups of bitwise-identical rows of a contiguous device tensor [n, ...], numbered in order of first occurrence (dts_group_rows):
    (slot int32 [n]: the group of row i; reps int32 [n]: the first row of group g for g < count, -1 beyond; count int32 [1]), all on the
    device -- nothing is read back here.  1 <= n <= 1024, bytes per row a multiple of 16."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError('group_rows: a GPU tensor (the HIP path has no CPU fallback)')
    if x.dim() < 1 or not x.is_contiguous():
        raise ValueError('group_rows: a contiguous tensor [n, ...]')
    n = x.shape[0]
    row_bytes = (x.numel() // n) * x.element_size() if n else 0
    if not 1 <= n <= GROUP_ROWS_MAX or row_bytes == 0 or row_bytes % 16:
        raise ValueError(f'group_rows: {n} rows of {row_bytes} bytes (1 .. {GROUP_ROWS_MAX} rows, a multiple of 16 bytes each)')
    ws = torch.empty((n, 4), dtype=torch.int32, device=x.device)
    out = torch.empty((2 * n + 1,), dtype=torch.int32, device=x.device)
    slot, reps, count = out[:n], out[n:2 * n], out[2 * n:]
    _call('dts_group_rows', x.data_ptr(), n, row_bytes, ws.data_ptr(), slot.data_ptr(), reps.data_ptr(), count.data_ptr())
    return slot, reps, count


def _norm_pair(who, gamma, beta, c):
    if tuple(gamma.shape) != (c,) or tuple(beta.shape) != (c,):
        raise ValueError(f'{who}: gamma {tuple(gamma.shape)} / beta {tuple(beta.shape)} for {c} channels')
    return _ptr(gamma, 'gamma', torch.float32), _ptr(beta, 'beta', torch.float32)


def layer_norm(x, gamma, beta, eps=1e-5):
    """LayerNorm over the last dimension of a contiguous float16 / bfloat16 tensor; gamma, beta float32 [c] (dts_layer_norm)."""
    c = x.shape[-1]
    gp, bp = _norm_pair('layer_norm', gamma, beta, c)
    out = torch.empty_like(x)
    _call('dts_layer_norm', _ptr(x, 'x'), _ptr(out), dt_code(x.dtype), x.numel() // c, c, float(eps), gp, bp)
    return out


def geglu(x):
    """x [..., 2*inner] -> x[..., :inner] * gelu(x[..., inner:]) with the exact (erf) GELU (dts_geglu; float16 / bfloat16)."""
    inner = x.shape[-1] // 2
    if x.shape[-1] != 2 * inner:
        raise ValueError(f'geglu: odd last dimension {x.shape[-1]}')
    out = torch.empty(tuple(x.shape[:-1]) + (inner,), dtype=x.dtype, device=x.device)
    _call('dts_geglu', _ptr(x, 'x'), _ptr(out), dt_code(x.dtype), x.numel() // (2 * inner), inner)
    return out


# ---- CLIP vision tower ----------------------------------------------------------------------------
def patch_kpad(patch):
    """columns of a patch row: 3*patch*patch rounded up to conv2d's 64-channel granularity (588 -> 640 at patch 14, 3072 at patch 32)"""
    return (3 * patch * patch + 63) // 64 * 64


def _patch_rows(who, x, patch, kpad, kmul=None):
    """what ops.patchify and ops.patchify_x3 ask of their arguments: -> (n, S, S // patch, kpad).  kmul: the multiple kpad is held to HERE
    (the operand image's 32); the 16-bit form leaves that refusal to the library."""
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
        raise ValueError(f'{who}: x {tuple(x.shape)} is not [n, 3, S, S]')
    n, _, S, _ = x.shape
    if patch <= 0 or S % patch:
        raise ValueError(f'{who}: image size {S} is not a multiple of the patch size {patch}')
    kpad = patch_kpad(patch) if kpad is None else int(kpad)
    if kmul and (kpad % kmul or kpad < 3 * patch * patch):
        raise ValueError(f'{who}: kpad {kpad} (a multiple of {kmul}, at least 3*patch*patch = {3 * patch * patch})')
    return n, S, S // patch, kpad


def patchify(x, patch, dtype, kpad=None, out=None):
    """pixel_values float32 NCHW [n, 3, S, S] -> patch rows [n, (S/patch)^2, kpad] in float16 / bfloat16: column (c*patch + py)*patch + px of
    row gy*(S/patch) + gx is x[n, c, gy*patch + py, gx*patch + px] rounded once, columns from 3*patch*patch on are zero (dts_patchify).
    kpad defaults to patch_kpad(patch)."""
    n, S, g, kpad = _patch_rows('patchify', x, patch, kpad)
    if out is None:
        out = torch.empty((n, g * g, kpad), dtype=dtype, device=x.device)
    elif tuple(out.shape) != (n, g * g, kpad):
        raise ValueError(f'patchify: out {tuple(out.shape)} != {(n, g * g, kpad)}')
    _call('dts_patchify', _ptr(x, 'x', torch.float32), _ptr(out, 'out', dtype), dt_code(dtype), n, S, patch, kpad)
    return out


def _token_tables(who, patches, cls, pos):
    n, tp, c = patches.shape
    if tuple(cls.shape) != (c,) or tuple(pos.shape) != (tp + 1, c):
        raise ValueError(f'{who}: cls {tuple(cls.shape)} / pos {tuple(pos.shape)} for patches {tuple(patches.shape)}')
    return n, tp, c


def vit_tokens(patches, cls, pos):
    """patches [n, t-1, c] float16 / bfloat16, cls float32 [c], pos float32 [t, c] -> tokens [n, t, c]: row 0 = cls + pos[0], row 1 + p =
    patches[:, p] + pos[1 + p], summed in float32 and rounded once (dts_vit_tokens)."""
    n, tp, c = _token_tables('vit_tokens', patches, cls, pos)
    out = torch.empty((n, tp + 1, c), dtype=patches.dtype, device=patches.device)
    _call('dts_vit_tokens', _ptr(patches, 'patches'), _ptr(cls, 'cls', torch.float32), _ptr(pos, 'pos', torch.float32), _ptr(out),
          dt_code(patches.dtype), n, tp + 1, c)
    return out


def _text_ids(who, ids, tok, pos):
    """the host checks of text_tokens / text_tokens_f32 -> (int32 ids on the tables' device, n, t, c, vocab)"""
    if not torch.is_tensor(ids) or ids.dim() != 2 or ids.dtype.is_floating_point or ids.dtype == torch.bool or ids.numel() == 0:
        raise ValueError(f'{who}: ids must be an integer tensor [n, t], got {tuple(ids.shape) if torch.is_tensor(ids) else type(ids).__name__}'
                         + (f' {ids.dtype}' if torch.is_tensor(ids) else ''))
    n, t = ids.shape
    if tok.dim() != 2 or pos.dim() != 2 or pos.shape[1] != tok.shape[1] or pos.shape[0] < t:
        raise ValueError(f'{who}: tok {tuple(tok.shape)} / pos {tuple(pos.shape)} for ids {tuple(ids.shape)}')
    vocab, c = tok.shape
    host = ids.detach().cpu()
    lo, hi = int(host.min()), int(host.max())
    if lo < 0 or hi >= vocab:
        raise ValueError(f'{who}: token id {lo if lo < 0 else hi} is outside [0, {vocab}) (the rows of the token table)')
    return host.to(torch.int32).to(tok.device).contiguous(), n, t, c, vocab


def text_tokens(ids, tok, pos, dtype):
    """ids integer [n, t], tok float32 [vocab, c], pos float32 [>= t, c] (both on the device) -> [n, t, c] in float16 / bfloat16:
    tok[ids] + pos[:t], summed in float32 and rounded once (dts_text_tokens).  The kernel cannot report a bad id, so 0 <= id < vocab is
    checked HERE, on the host, before the upload: a ValueError names the offending value.  The ids come from the tokenizer as a host
    tensor; one that is already on the device is copied back for the check -- one synchronisation, acceptable where this runs (once per
    prompt)."""
    dev_ids, n, t, c, vocab = _text_ids('text_tokens', ids, tok, pos)
    out = torch.empty((n, t, c), dtype=dtype, device=tok.device)
    _call('dts_text_tokens', _ptr(dev_ids, 'ids', torch.int32), _ptr(tok, 'tok', torch.float32), _ptr(pos, 'pos', torch.float32), _ptr(out),
          dt_code(dtype), n, t, c, vocab)
    return out


def text_tokens_f32(ids, tok, pos):
    """text_tokens in float32 (dts_text_tokens_f32: one float32 add, nothing rounded to 16 bits) -> float32 [n, t, c]; the same host check
    of 0 <= id < vocab before the upload; c a multiple of 8."""
    dev_ids, n, t, c, vocab = _text_ids('text_tokens_f32', ids, tok, pos)
    if c <= 0 or c % 8:
        raise ValueError(f'text_tokens_f32: {c} channels (a multiple of 8)')
    out = torch.empty((n, t, c), dtype=torch.float32, device=tok.device)
    _call('dts_text_tokens_f32', _ptr(dev_ids, 'ids', torch.int32), _ptr(tok, 'tok', torch.float32), _ptr(pos, 'pos', torch.float32), _ptr(out),
          n, t, c, vocab)
    return out


GELU_KINDS = {'quick_gelu': 0, 'gelu': 1}


def gelu(x, kind='quick_gelu', out=None):
    """Elementwise over a contiguous float16 / bfloat16 tensor whose element count is a multiple of 8 (dts_gelu).  kind 'quick_gelu':
    x * sigmoid(1.702 x); 'gelu': the exact (erf) GELU.  out may be x itself (in place)."""
    if kind not in GELU_KINDS:
        raise ValueError(f'gelu: kind {kind!r} (one of {sorted(GELU_KINDS)})')
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape:
        raise ValueError(f'gelu: out {tuple(out.shape)} != x {tuple(x.shape)}')
    _call('dts_gelu', _ptr(x, 'x'), _ptr(out, 'out', x.dtype), dt_code(x.dtype), x.numel(), GELU_KINDS[kind])
    return out


def vit_head(tokens, gamma, beta, eps=1e-5):
    """tokens [n, t, c] float16 / bfloat16 -> float32 [n, c] = LayerNorm(tokens[:, 0]) * gamma + beta: the class token only, the other
    tokens are not read (dts_vit_head); gamma, beta float32 [c].  The projection follows as ops.linear."""
    n, t, c = tokens.shape
    gp, bp = _norm_pair('vit_head', gamma, beta, c)
    out = torch.empty((n, c), dtype=torch.float32, device=tokens.device)
    _call('dts_vit_head', _ptr(tokens, 'tokens'), _ptr(out), dt_code(tokens.dtype), n, t, c, float(eps), gp, bp)
    return out


# ---- CLIP vision tower, split-precision mode (F16X3) ------------------------------------------------
# float32 activations; what only a split-precision 1x1 conv2d reads leaves as its operand image (SplitAct: split3_f16's bits).
def _f32_gpu(t, who, name):
    """host-side refusal, by name, before any launch: `t` must be a contiguous float32 GPU tensor"""
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise ValueError(f'{who}: {name} must be a float32 tensor, got {t.dtype if torch.is_tensor(t) else type(t).__name__}')
    return _ptr(t, name, torch.float32)


def layer_norm_x3(x, gamma, beta, eps=1e-5, want_f32=False, want_split=True):
    """LayerNorm over the last dimension of a contiguous float32 tensor [..., c] (dts_layer_norm_x3); gamma, beta float32 [c]; c a multiple of
    32, at most 2048.  Returns the operand image of the normalised rows (SplitAct; a 3-D input [n, t, c] is taken as [n, t, 1, c]), or with
    want_f32 the pair (float32 rows shaped like x, SplitAct), or with want_split=False the float32 rows alone.  The image is the split of the
    float32 rows whether or not those are written."""
    if not (want_f32 or want_split):
        raise ValueError('layer_norm_x3: neither want_f32 nor want_split')
    xp = _f32_gpu(x, 'layer_norm_x3', 'x')
    if x.dim() not in (3, 4):
        raise ValueError(f'layer_norm_x3: x {tuple(x.shape)} is not [n, t, c] or [n, h, w, c]')
    c = x.shape[-1]
    if c <= 0 or c % 32 or c > 2048:
        raise ValueError(f'layer_norm_x3: {c} channels (a multiple of 32, at most 2048)')
    gp, bp = _norm_pair('layer_norm_x3', gamma, beta, c)
    lead = tuple(x.shape[:-1]) if x.dim() == 4 else tuple(x.shape[:2]) + (1,)
    out = torch.empty_like(x) if want_f32 else None
    img = torch.empty(lead + (2 * c,), dtype=torch.float16, device=x.device) if want_split else None
    _call('dts_layer_norm_x3', xp, _ptr(out), _ptr(img), x.numel() // c, c, float(eps), gp, bp)
    if not want_split:
        return out
    return (out, SplitAct(img, c)) if want_f32 else SplitAct(img, c)


def gelu_x3(x, kind='quick_gelu'):
    """act(x) of a contiguous float32 tensor [n, h, w, c] as the operand image of the convolution that follows (SplitAct; dts_gelu_x3); kind as
    ops.gelu; c a multiple of 32."""
    if kind not in GELU_KINDS:
        raise ValueError(f'gelu_x3: kind {kind!r} (one of {sorted(GELU_KINDS)})')
    xp = _f32_gpu(x, 'gelu_x3', 'x')
    if x.dim() != 4:
        raise ValueError(f'gelu_x3: x {tuple(x.shape)} is not [n, h, w, c]')
    c = x.shape[-1]
    if c <= 0 or c % 32:
        raise ValueError(f'gelu_x3: {c} channels (a multiple of 32)')
    img = torch.empty(tuple(x.shape[:-1]) + (2 * c,), dtype=torch.float16, device=x.device)
    _call('dts_gelu_x3', xp, _ptr(img), x.numel() // c, c, GELU_KINDS[kind])
    return SplitAct(img, c)


def patchify_x3(x, patch, kpad=None):
    """pixel_values float32 NCHW [n, 3, S, S] -> the operand image of the unrounded patch rows (SplitAct of logical shape [n, S/patch, S/patch,
    kpad]; dts_patchify_x3): ops.patchify's column order, columns from 3*patch*patch on are zero.  kpad defaults to patch_kpad(patch) and must
    be a multiple of 32 covering 3*patch*patch."""
    xp = _f32_gpu(x, 'patchify_x3', 'x')
    n, S, g, kpad = _patch_rows('patchify_x3', x, patch, kpad, 32)
    img = torch.empty((n, g, g, 2 * kpad), dtype=torch.float16, device=x.device)
    _call('dts_patchify_x3', xp, _ptr(img), n, S, patch, kpad)
    return SplitAct(img, kpad)


def vit_tokens_f32(patches, cls, pos):
    """patches float32 [n, t-1, c], cls float32 [c], pos float32 [t, c] -> float32 tokens [n, t, c]: row 0 = cls + pos[0], row 1 + p =
    patches[:, p] + pos[1 + p] (dts_vit_tokens_f32: one float32 add); c a multiple of 4."""
    pp = _f32_gpu(patches, 'vit_tokens_f32', 'patches')
    if patches.dim() != 3:
        raise ValueError(f'vit_tokens_f32: patches {tuple(patches.shape)} is not [n, t - 1, c]')
    n, tp, c = _token_tables('vit_tokens_f32', patches, cls, pos)
    if tp < 1 or c <= 0 or c % 4:
        raise ValueError(f'vit_tokens_f32: {tp} patches x {c} channels (at least one patch, channels a multiple of 4)')
    out = torch.empty((n, tp + 1, c), dtype=torch.float32, device=patches.device)
    _call('dts_vit_tokens_f32', pp, _ptr(cls, 'cls', torch.float32), _ptr(pos, 'pos', torch.float32), _ptr(out), n, tp + 1, c)
    return out


def vit_head_f32(tokens, gamma, beta, eps=1e-5):
    """tokens float32 [n, t, c] -> float32 [n, c] = LayerNorm(tokens[:, 0]) * gamma + beta (dts_vit_head_f32: the class token only);
    c a multiple of 8, at most 2048.  The projection follows as ops.linear."""
    tp = _f32_gpu(tokens, 'vit_head_f32', 'tokens')
    if tokens.dim() != 3:
        raise ValueError(f'vit_head_f32: tokens {tuple(tokens.shape)} is not [n, t, c]')
    n, t, c = tokens.shape
    if c <= 0 or c % 8 or c > 2048:
        raise ValueError(f'vit_head_f32: {c} channels (a multiple of 8, at most 2048)')
    gp, bp = _norm_pair('vit_head_f32', gamma, beta, c)
    out = torch.empty((n, c), dtype=torch.float32, device=tokens.device)
    _call('dts_vit_head_f32', tp, _ptr(out), n, t, c, float(eps), gp, bp)
    return out


def stride2_conv_weight(w, cpad=None):
    """The weight of Conv2d(kernel 3, stride 2, padding 1) (diffusers Downsample2D) as a 3x3 padding-1 stride-1 convolution over
    space_to_depth2(x): output pixel (i, j) reads input rows 2i - 1, 2i, 2i + 1 = phase 1 of pixel block i - 1 and phases 0, 1 of block i, so
    of the 3 x 3 block taps only those at offsets {-1, 0} are live and each carries the source taps that fall on its phases (the others stay
    zero: 4 x the multiply-adds of the strided form).  w [O, C, 3, 3] -> [O, cpad or 4C, 3, 3], channel (ry*2 + rx)*C + c; a pure rearrangement."""
    O, Cin, kh, kw = w.shape
    if (kh, kw) != (3, 3):
        raise ValueError('stride2_conv_weight: a 3x3 weight')
    cpad = 4 * Cin if cpad is None else cpad
    out = torch.zeros((O, cpad, 3, 3), dtype=w.dtype, device=w.device)
    place = ((0, 1), (1, 0), (1, 1))                 # source tap u -> (block tap t, phase r): 2i + u - 1 = 2(i + t - 1) + r
    for u, (ty, ry) in enumerate(place):
        for v, (tx, rx) in enumerate(place):
            ch = (ry * 2 + rx) * Cin
            out[:, ch:ch + Cin, ty, tx] = w[:, :, u, v]
    return out


# ---- embedding / preconditioning ----------------------------------------------------------------
def linear(x, w, bias=None, *, act_in=False, act_out=False, out=None, accumulate=False):
    m, k = x.shape
    nn_ = w.shape[0]
    if out is None:
        out = torch.empty((m, nn_), dtype=torch.float32, device=x.device)
    _call('dts_linear', _ptr(x, 'x', torch.float32), x.stride(0) if x.dim() == 2 else k, _ptr(w, 'w', torch.float32),
          _ptr(bias, 'bias', torch.float32), _ptr(out, 'out', torch.float32), out.shape[-1], m, k, nn_,
          int(act_in), int(act_out), int(accumulate))
    return out


def pos_embedding(v, freqs, swap=False):
    n, half = v.shape[0], freqs.shape[0]
    out = torch.empty((n, 2 * half), dtype=torch.float32, device=v.device)
    _call('dts_pos_embedding', _ptr(v, 'v', torch.float32), _ptr(freqs, 'freqs', torch.float32), _ptr(out), n, half, int(swap))
    return out


def edm_precond_in(x, sigma, sigma_data):
    """x f64 NCHW, sigma f64 [1] or [n] -> (c_in*x as f32 NCHW, coef f32 [n,4] = c_skip,c_out,c_in,c_noise)."""
    n = x.shape[0]
    chw = x[0].numel()
    xin = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    coef = torch.empty((n, 4), dtype=torch.float32, device=x.device)
    _call('dts_edm_precond_in', _ptr(x, 'x', torch.float64), _ptr(sigma, 'sigma', torch.float64), sigma.numel(),
          float(sigma_data), _ptr(xin), _ptr(coef), n, chw)
    return xin, coef


PRECOND_KINDS = {'vp': 1, 've': 2, 'iddpm': 3}          # dts.h dts_precond_kind


def precond_params(kind, M=1000, beta_d=19.9, beta_min=0.1):
    """The host array dts_precond_in reads: the Python-scalar sub-expressions of the reference's forward (networks.py:504, 517, 610), each
    evaluated in double and rounded to float32 once -- what torch does with a Python scalar that meets a float32 tensor."""
    import ctypes
    if kind == 'vp':
        v = (M - 1, beta_min ** 2, 2 * beta_d, beta_min, beta_d)
    elif kind == 'iddpm':
        v = (M - 1, 0.0, 0.0, 0.0, 1.0)
    else:
        return None
    return (ctypes.c_float * 5)(*[float(t) for t in v])


def precond_in(kind, x, sigma, params=None, table=None):
    """The VP / VE / iDDPM twin of edm_precond_in: x f64 NCHW, sigma f64 [1] or [n] -> (c_in*x f32 NCHW, coef f32 [n,4]).  params:
    precond_params(...); table: the iDDPM `u` buffer, f32 on the device."""
    if kind not in PRECOND_KINDS:
        raise ValueError(f'precond_in: kind {kind!r}, one of {sorted(PRECOND_KINDS)}')
    if (kind != 've' and params is None) or (kind == 'iddpm' and table is None):
        raise ValueError(f'precond_in: kind {kind!r} needs its params' + (' and table' if kind == 'iddpm' else ''))
    n = x.shape[0]
    xin = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    coef = torch.empty((n, 4), dtype=torch.float32, device=x.device)
    _call('dts_precond_in', PRECOND_KINDS[kind], params, _ptr(table, 'table', torch.float32), 0 if table is None else table.numel(),
          _ptr(x, 'x', torch.float64), _ptr(sigma, 'sigma', torch.float64), sigma.numel(), _ptr(xin), _ptr(coef), n, x[0].numel())
    return xin, coef


def edm_precond_out(x, F, coef):
    n = x.shape[0]
    D = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _call('dts_edm_precond_out', _ptr(x, 'x', torch.float64), _ptr(F, 'F', torch.float32), _ptr(coef, 'coef', torch.float32),
          _ptr(D), n, x[0].numel())
    return D


def cast_from_f32(x, dtype):
    if dtype == torch.float32:
        return x
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    _call('dts_cast_from_f32', _ptr(x, 'x', torch.float32), _ptr(out), dt_code(dtype), x.numel())
    return out


def cast_to_f32(x):
    if x.dtype == torch.float32:
        return x
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _call('dts_cast_to_f32', _ptr(x), dt_code(x.dtype), _ptr(out), x.numel())
    return out


# ---- Heun step ----------------------------------------------------------------------------------
def heun_xhat(x_cur, eps, noise_coef, nb, interleave=False):
    """x_hat[i] = x_cur[src(i)] + noise_coef*eps[i]; x_cur has xb rows, broadcast to nb rows
    (Tensor.repeat order unless interleave=True = repeat_interleave order)."""
    xb = x_cur.shape[0]
    chw = x_cur[0].numel()
    if eps.dtype not in (torch.float64, torch.float32):
        raise ValueError('eps must be float64 or float32')
    if eps.shape[0] != nb:
        raise ValueError('eps rows != nb')
    x_hat = torch.empty((nb,) + tuple(x_cur.shape[1:]), dtype=torch.float64, device=x_cur.device)
    _call('dts_heun_xhat', _ptr(x_cur, 'x_cur', torch.float64), xb, int(interleave), _ptr(eps, 'eps'),
          int(eps.dtype == torch.float32), float(noise_coef), _ptr(x_hat), nb, chw)
    return x_hat


def heun_euler(x_hat, D, t_hat, t_next):
    d_cur = torch.empty_like(x_hat)
    x_next = torch.empty_like(x_hat)
    _call('dts_heun_euler', _ptr(x_hat, 'x_hat', torch.float64), _ptr(D, 'D', torch.float32), float(t_hat), float(t_next),
          _ptr(d_cur), _ptr(x_next), x_hat.numel())
    return d_cur, x_next


def heun_correct(x_hat, D2, d_cur, t_hat, t_next, x_next):
    _call('dts_heun_correct', _ptr(x_hat, 'x_hat', torch.float64), _ptr(D2, 'D2', torch.float32),
          _ptr(d_cur, 'd_cur', torch.float64), float(t_hat), float(t_next), _ptr(x_next, 'x_next', torch.float64), x_hat.numel())
    return x_next


def row_scalars(values, n, name, device, nonzero=False):
    """The per-row scalars of a dts_heun_*_rows launch: `values`, a sequence or a tensor of n numbers, as a float64 device tensor [n].  A
    tensor that is already that is passed through unread (the caller checked it on the host before uploading it, once for several launches);
    anything else is a host array, checked here -- with nonzero=True an entry equal to 0 is refused by name, which the kernel's entry point
    cannot do without a host read -- and uploaded."""
    if isinstance(values, torch.Tensor) and values.is_cuda:
        if values.dtype != torch.float64 or tuple(values.shape) != (n,):
            raise ValueError(f'{name}: a device tensor must be float64 [{n}], got {values.dtype} {tuple(values.shape)}')
        return values.contiguous()
    host = torch.as_tensor(values, dtype=torch.float64).reshape(-1)
    if host.numel() != n:
        raise ValueError(f'{name}: need one value per row, got {host.numel()} values for {n} rows')
    if nonzero and bool((host == 0).any()):
        raise ValueError(f'{name} == 0 in row {int((host == 0).nonzero()[0])}')
    return host.to(device).contiguous()


def heun_xhat_rows(x_cur, eps, noise_coef, nb, interleave=False):
    """heun_xhat with a noise coefficient per row: x_hat[i] = x_cur[src(i)] + noise_coef[i]*eps[i].  noise_coef: nb numbers (sequence or
    tensor).  Row i has the bits of heun_xhat launched with noise_coef[i]; a row whose coefficient is 0.0 is its source row."""
    xb = x_cur.shape[0]
    chw = x_cur[0].numel()
    if eps.dtype not in (torch.float64, torch.float32):
        raise ValueError('eps must be float64 or float32')
    if eps.shape[0] != nb:
        raise ValueError('eps rows != nb')
    coef = row_scalars(noise_coef, nb, 'heun_xhat_rows: noise_coef', x_cur.device)
    x_hat = torch.empty((nb,) + tuple(x_cur.shape[1:]), dtype=torch.float64, device=x_cur.device)
    _call('dts_heun_xhat_rows', _ptr(x_cur, 'x_cur', torch.float64), xb, int(interleave), _ptr(eps, 'eps'),
          int(eps.dtype == torch.float32), _ptr(coef), _ptr(x_hat), nb, chw)
    return x_hat


def heun_euler_rows(x_hat, D, t_hat, t_next):
    """heun_euler with t_hat / t_next per row (n numbers each); a host array holding t_hat == 0 is refused before any launch"""
    n, chw = x_hat.shape[0], x_hat[0].numel()
    th = row_scalars(t_hat, n, 'heun_euler_rows: t_hat', x_hat.device, nonzero=True)
    tn = row_scalars(t_next, n, 'heun_euler_rows: t_next', x_hat.device)
    d_cur = torch.empty_like(x_hat)
    x_next = torch.empty_like(x_hat)
    _call('dts_heun_euler_rows', _ptr(x_hat, 'x_hat', torch.float64), _ptr(D, 'D', torch.float32), _ptr(th), _ptr(tn),
          _ptr(d_cur), _ptr(x_next), n, chw)
    return d_cur, x_next


def heun_correct_rows(x_hat, D2, d_cur, t_hat, t_next, x_next):
    """heun_correct with t_hat / t_next per row (in place on x_next); a host array holding t_next == 0 (the last sigma step is Euler only) is
    refused before any launch"""
    n, chw = x_hat.shape[0], x_hat[0].numel()
    th = row_scalars(t_hat, n, 'heun_correct_rows: t_hat', x_hat.device)
    tn = row_scalars(t_next, n, 'heun_correct_rows: t_next', x_hat.device, nonzero=True)
    _call('dts_heun_correct_rows', _ptr(x_hat, 'x_hat', torch.float64), _ptr(D2, 'D2', torch.float32),
          _ptr(d_cur, 'd_cur', torch.float64), _ptr(th), _ptr(tn), _ptr(x_next, 'x_next', torch.float64), n, chw)
    return x_next


# ---- the general ODE step (ablation sampler, edm/generate.py:156-174) ---------------------------
def ode_xhat(x_cur, eps, ratio, noise_coef, s_hat=1.0):
    """x_hat = ratio * x_cur + noise_coef * eps (eps float64 | float32; None exactly when noise_coef == 0: no noise is read).
    Returns (x_hat, x_in): x_in = x_hat / s_hat, the denoiser's input -- x_hat itself when s_hat == 1."""
    if (eps is None) != (float(noise_coef) == 0.0):
        raise ValueError(f'ode_xhat: eps is None exactly when noise_coef == 0 (noise_coef = {float(noise_coef)!r})')
    if eps is not None:
        if eps.dtype not in (torch.float64, torch.float32):
            raise ValueError('eps must be float64 or float32')
        if eps.shape != x_cur.shape:
            raise ValueError(f'eps has shape {tuple(eps.shape)}, x_cur {tuple(x_cur.shape)}')
    x_hat = torch.empty_like(x_cur)
    x_in = torch.empty_like(x_cur) if float(s_hat) != 1.0 else None
    _call('dts_ode_xhat', _ptr(x_cur, 'x_cur', torch.float64), _ptr(eps, 'eps'), int(eps is not None and eps.dtype == torch.float32),
          float(ratio), float(noise_coef), float(s_hat), _ptr(x_hat), _ptr(x_in), x_cur.numel())
    return x_hat, (x_hat if x_in is None else x_in)


def ode_slope(x, D, a, b, step, s_out=1.0, base=None, want_d=True):
    """d = a * x - b * D; x_out = base + step * d (base = x unless given).  Returns (d or None, x_out, x_in): x_in = x_out / s_out, the
    denoiser's next input -- x_out itself when s_out == 1."""
    base = x if base is None else base
    if D.shape != x.shape or base.shape != x.shape:
        raise ValueError(f'ode_slope: x {tuple(x.shape)}, D {tuple(D.shape)}, base {tuple(base.shape)}')
    d = torch.empty_like(x) if want_d else None
    x_out = torch.empty_like(x)
    x_in = torch.empty_like(x) if float(s_out) != 1.0 else None
    _call('dts_ode_slope', _ptr(x, 'x', torch.float64), _ptr(D, 'D', torch.float32), float(a), float(b), _ptr(base, 'base', torch.float64),
          float(step), float(s_out), _ptr(d), _ptr(x_out), _ptr(x_in), x.numel())
    return d, x_out, (x_out if x_in is None else x_in)


def ode_correct(x_hat, x_prime, D2, d_cur, a, b, h, w0, w1):
    """x_next = x_hat + h * (w0 * d_cur + w1 * (a * x_prime - b * D2))"""
    if not (x_prime.shape == D2.shape == d_cur.shape == x_hat.shape):
        raise ValueError('ode_correct: shapes differ')
    x_next = torch.empty_like(x_hat)
    _call('dts_ode_correct', _ptr(x_hat, 'x_hat', torch.float64), _ptr(x_prime, 'x_prime', torch.float64), _ptr(D2, 'D2', torch.float32),
          _ptr(d_cur, 'd_cur', torch.float64), float(a), float(b), float(h), float(w0), float(w1), _ptr(x_next), x_hat.numel())
    return x_next


# ---- scorer plumbing ----------------------------------------------------------------------------
def quantize_u8(x, f32_math=False):
    """(x*127.5+128).clip(0,255) truncated to uint8; f64 arithmetic (EDM loop) unless f32_math (SD loop, f32 input)."""
    if x.dtype not in (torch.float64, torch.float32):
        raise ValueError('quantize_u8: float64/float32 only')
    if f32_math and x.dtype != torch.float32:
        raise ValueError('f32_math needs a float32 input')
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _call('dts_quantize_u8', _ptr(x), 2 if f32_math else int(x.dtype == torch.float32), _ptr(out), x.numel())
    return out


def cfg_combine(uncond, cond, guidance):
    out = torch.empty_like(uncond)
    _call('dts_cfg_combine', _ptr(uncond, 'uncond'), _ptr(cond, 'cond', uncond.dtype), float(guidance), _ptr(out),
          dt_code(uncond.dtype), uncond.numel())
    return out


def brightness(img_u8):
    n, c, h, w = img_u8.shape
    assert c == 3
    out = torch.empty((n,), dtype=torch.float32, device=img_u8.device)
    _call('dts_brightness', _ptr(img_u8, 'img', torch.uint8), _ptr(out), n, h * w)
    return out


def u8_to_unit_f32(img_u8):
    out = torch.empty(img_u8.shape, dtype=torch.float32, device=img_u8.device)
    _call('dts_u8_to_unit_f32', _ptr(img_u8, 'img', torch.uint8), _ptr(out), img_u8.numel())
    return out


def resample_u8(img, out_len, axis, bounds, coefs):
    """One pass of Pillow's 8-bit separable resampling: img uint8 [planes, h, w] -> [planes, h, out_len] (axis 1) or [planes, out_len, w]
    (axis 0); bounds int32 [out_len, 2], coefs int32 [out_len, ksize] (clip_preprocess.resample_tables)."""
    planes, h, w = img.shape
    out = torch.empty((planes, h, out_len) if axis else (planes, out_len, w), dtype=torch.uint8, device=img.device)
    _call('dts_resample_u8', _ptr(img, 'img', torch.uint8), _ptr(out), planes, h, w, out_len, int(axis), _ptr(bounds, 'bounds', torch.int32),
          _ptr(coefs, 'coefs', torch.int32), coefs.shape[1])
    return out


def lut_u8_f32(img, lut):
    """img uint8 [n, c, h, w], lut f32 [c, 256] -> f32 [n, c, h, w]."""
    n, c, h, w = img.shape
    out = torch.empty(img.shape, dtype=torch.float32, device=img.device)
    _call('dts_lut_u8_f32', _ptr(img, 'img', torch.uint8), _ptr(lut, 'lut', torch.float32), _ptr(out), n, c, h * w)
    return out


# ---- JPEG byte length (the compressibility reward) -------------------------------------------------
# ITU T.81 Annex K.1 / K.2: the luminance and chrominance quantisation tables a quality setting scales, natural (row-major) order
_JPEG_BASE_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
_JPEG_BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
_JPEG_QTAB, _JPEG_WS = {}, {}


def _jpeg_quality(quality):
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f'jpeg: quality must be an integer in [1, 100], got quality={quality!r}')
    return quality


def jpeg_quant_tables(quality):
    """(luma, chroma): the two 64-entry quantisation tables (natural order, ints in [1, 255]) a baseline JPEG encoder derives from
    `quality` in [1, 100]: the Annex K tables times 5000/q % below 50, (200 - 2q) % from 50 on, rounded, clamped."""
    q = _jpeg_quality(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(255, max(1, (b * scale + 50) // 100)) for b in base] for base in (_JPEG_BASE_LUMA, _JPEG_BASE_CHROMA))


def jpeg_header_bytes():
    """Bytes of a Pillow-written baseline JPEG file in front of its entropy-coded data: SOI, APP0 (JFIF), two DQT, SOF0, four DHT (the
    standard tables: 12 DC symbols, 162 AC symbols), SOS; every segment = marker (2) + length field (2) + payload."""
    soi, app0, dqt, sof0, sos = 2, 4 + 14, 4 + 1 + 64, 4 + 6 + 3 * 3, 4 + 1 + 3 * 2 + 3
    dht_dc, dht_ac = 4 + 1 + 16 + 12, 4 + 1 + 16 + 162
    return soi + app0 + 2 * dqt + sof0 + 2 * dht_dc + 2 * dht_ac + sos


def jpeg_size(img_u8, quality=80, return_coefficients=False):
    """Byte length of the JPEG file `PIL.Image.save(format='JPEG', quality=quality)` writes for each image -- exact, computed on the GPU
    without writing the file (dts_jpeg_size).  img_u8: uint8 GPU tensor [n, 3, h, w], h and w multiples of 16; anything else raises
    ValueError (no fallback: score such images with the host codec).  Returns int32 [n] on the images' device; with
    return_coefficients also the quantised DCT coefficients, int16 [n, h/16 * w/16 * 6, 64]: zigzag order, blocks in scan order (per
    16x16 MCU: four Y blocks, Cb, Cr)."""
    q = _jpeg_quality(quality)
    if not isinstance(img_u8, torch.Tensor) or img_u8.dtype != torch.uint8:
        raise ValueError(f'jpeg_size: expected a uint8 tensor, got {getattr(img_u8, "dtype", type(img_u8))}')
    if not img_u8.is_cuda:
        raise ValueError(f'jpeg_size: the image tensor is on {img_u8.device}; the HIP codec takes GPU tensors (no CPU fallback)')
    if img_u8.dim() != 4 or img_u8.shape[1] != 3:
        raise ValueError(f'jpeg_size: expected [n, 3, h, w] (3 channels), got shape {tuple(img_u8.shape)}')
    n, _, h, w = img_u8.shape
    if n < 1 or h < 16 or w < 16 or h % 16 or w % 16:
        raise ValueError(f'jpeg_size: shape {tuple(img_u8.shape)}: height and width must be multiples of 16 (whole MCUs) and n >= 1')
    lib = L.load()
    need = lib.dts_jpeg_workspace_bytes(n, h, w)
    if need <= 0:
        raise ValueError(f'jpeg_size: shape {tuple(img_u8.shape)} is beyond what one call takes')
    dev = img_u8.device
    key = (dev.type, dev.index)
    ws = _JPEG_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _JPEG_WS[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    qtab = _JPEG_QTAB.get(key + (q,))
    if qtab is None:
        qtab = _JPEG_QTAB[key + (q,)] = torch.tensor(jpeg_quant_tables(q), dtype=torch.int16).to(dev)     # <= 255: the bits of a uint16 table
    sizes = torch.empty((n,), dtype=torch.int32, device=dev)
    coef = torch.empty((n, (h // 16) * (w // 16) * 6, 64), dtype=torch.int16, device=dev) if return_coefficients else None
    _call('dts_jpeg_size', _ptr(img_u8, 'img', torch.uint8), _ptr(sizes), n, h, w, _ptr(qtab), _ptr(ws), ws.numel(), _ptr(coef))
    return (sizes, coef) if return_coefficients else sizes


def cosine_rows(a, b):
    """a [n,d] f32, b [n,d] or [1,d] f32 -> [n] f32: cosine similarity of the L2-normalised rows (CLIP reward tail)."""
    n, d = a.shape
    out = torch.empty((n,), dtype=torch.float32, device=a.device)
    _call('dts_cosine_rows', _ptr(a, 'a', torch.float32), _ptr(b, 'b', torch.float32), b.shape[0], _ptr(out), n, d)
    return out


def attnpool_tokens(x, pos):
    n, h, w, c = x.shape
    out = torch.empty((n, h * w + 1, c), dtype=x.dtype, device=x.device)
    _call('dts_attnpool_tokens', _ptr(x), _ptr(pos, 'pos', torch.float32), _ptr(out), dt_code(x.dtype), n, h * w, c)
    return out


def take_token(x, token):
    n, t, c = x.shape
    out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    _call('dts_take_token', _ptr(x), dt_code(x.dtype), _ptr(out), n, t, c, int(token))
    return out


def softmax_gather(logits, target):
    n, k = logits.shape
    out = torch.empty((n,), dtype=torch.float32, device=logits.device)
    _call('dts_softmax_gather', _ptr(logits, 'logits', torch.float32), _ptr(target, 'target', torch.int32), _ptr(out), n, k)
    return out


def candidate_noise(pivot, g, mode, scale):
    """pivot [b,...] f64, g [N*b,...] f64 (n-major), mode int32 [N], scale f32 [N] -> candidates [N*b,...] f64."""
    b = pivot.shape[0]
    nb = g.shape[0]
    out = torch.empty_like(g)
    _call('dts_candidate_noise', _ptr(pivot, 'pivot', torch.float64), _ptr(g, 'g', torch.float64),
          _ptr(mode, 'mode', torch.int32), _ptr(scale, 'scale', torch.float32), _ptr(out), nb, b, pivot[0].numel())
    return out


def candidate_noise_rows(pivot, g, mode_rows, scale_rows):
    """candidate_noise with mode / scale per output row: pivot [b,...] f64, g [N*b,...] f64 (n-major), mode_rows int32 [N*b] (or [N, b]),
    scale_rows f32 [N*b] -> candidates [N*b,...] f64; row n*b + s is built from pivot[s].  Bit-equal to candidate_noise where mode / scale
    are constant over the images of every candidate."""
    b = pivot.shape[0]
    nb = g.shape[0]
    if mode_rows.numel() != nb or scale_rows.numel() != nb:
        raise ValueError(f'candidate_noise_rows: mode / scale need one entry per output row ({nb}), got {mode_rows.numel()} / {scale_rows.numel()}')
    out = torch.empty_like(g)
    _call('dts_candidate_noise_rows', _ptr(pivot, 'pivot', torch.float64), _ptr(g, 'g', torch.float64),
          _ptr(mode_rows, 'mode_rows', torch.int32), _ptr(scale_rows, 'scale_rows', torch.float32), _ptr(out), nb, b, pivot[0].numel())
    return out


def candidate_noise_sd(pivot, u, mode, scale):
    """pivot [1,C,H,W], u [N,1,C,H,W] (same dtype), mode int32 [N], scale f32 [N,3] = (rand, lambda, sqrt(numel)) per candidate ->
    candidates [N,1,C,H,W]: the SD backend's eps-greedy / zero-order builder (pipeline_stable_diffusion.py:1371-1379) in the latents' dtype,
    the three tensor-by-scalar products rounded one by one like the reference's."""
    n = u.shape[0]
    if tuple(scale.shape) != (n, 3):
        raise ValueError(f'candidate_noise_sd: scale must be [{n}, 3] (rand, lambda, sqrt(numel)), got {tuple(scale.shape)}')
    out = torch.empty_like(u)
    _call('dts_candidate_noise_sd', _ptr(pivot, 'pivot'), _ptr(u, 'u', pivot.dtype), _ptr(mode, 'mode', torch.int32),
          _ptr(scale, 'scale', torch.float32), _ptr(out), dt_code(pivot.dtype), n, pivot.numel())
    return out


def candidate_noise_sd_rows(pivot, u, mode, scale, out=None):
    """candidate_noise_sd for S searches in lock-step: pivot [S,C,H,W], u [S*N,C,H,W] (same dtype, search-major), mode int32 [S*N],
    scale f32 [S*N,3] -> candidates [S*N,C,H,W] (written into `out` where given); row s*N + n is built from pivot[s] with its own mode and
    scale.  S = 1 is candidate_noise_sd bit for bit."""
    s_, rows = pivot.shape[0], u.shape[0]
    if s_ < 1 or rows % s_ != 0 or tuple(u.shape[1:]) != tuple(pivot.shape[1:]):
        raise ValueError(f'candidate_noise_sd_rows: u {tuple(u.shape)} is not a whole number of rows per pivot of {tuple(pivot.shape)}')
    if mode.numel() != rows or tuple(scale.shape) != (rows, 3):
        raise ValueError(f'candidate_noise_sd_rows: mode must be [{rows}] and scale [{rows}, 3] (rand, lambda, sqrt(numel)), got '
                         f'{tuple(mode.shape)} / {tuple(scale.shape)}')
    out = _out('candidate_noise_sd_rows', out, tuple(u.shape), u.dtype, u.device)
    _call('dts_candidate_noise_sd_rows', _ptr(pivot, 'pivot'), _ptr(u, 'u', pivot.dtype), _ptr(mode, 'mode', torch.int32),
          _ptr(scale, 'scale', torch.float32), _ptr(out, 'out', pivot.dtype), dt_code(pivot.dtype), s_, rows // s_, pivot[0].numel())
    return out


def ddim_candidates_groups(x, e, z, alpha_t, alpha_prev, sigma_t, ncand=None, want_x0=True, out=None, x0_out=None):
    """ddim_candidates for G independent (x, e) pairs in one launch: x, e [G, ...]; z [G, ncand, ...] or None (then ncand = 1 unless given)
    -> (prev [G, ncand, ...], x0 [G, ...] or None), written into `out` / `x0_out` where given.  The scalars are shared by the groups.
    G = 1 is ddim_candidates bit for bit."""
    g = x.shape[0]
    if z is not None:
        if z.dim() != x.dim() + 1 or z.shape[0] != g or tuple(z.shape[2:]) != tuple(x.shape[1:]) or (ncand is not None and z.shape[1] != ncand):
            raise ValueError(f'ddim_candidates_groups: z {tuple(z.shape)} is not [G, ncand, ...] over x {tuple(x.shape)}')
        ncand = z.shape[1]
    ncand = 1 if ncand is None else int(ncand)
    if tuple(e.shape) != tuple(x.shape):
        raise ValueError(f'ddim_candidates_groups: e {tuple(e.shape)} != x {tuple(x.shape)}')
    prev = _out('ddim_candidates_groups', out, (g, ncand) + tuple(x.shape[1:]), x.dtype, x.device)
    x0 = _out('ddim_candidates_groups', x0_out, tuple(x.shape), x.dtype, x.device) if want_x0 else None
    _call('dts_ddim_candidates_groups', _ptr(x), _ptr(e, 'e', x.dtype), _ptr(z, 'z', x.dtype), _ptr(prev, 'out', x.dtype), _ptr(x0, 'x0_out'),
          dt_code(x.dtype), float(alpha_t), float(alpha_prev), float(sigma_t), g, ncand, x[0].numel() if g else 0)
    return prev, x0


def ddim_candidates(x, e, z, alpha_t, alpha_prev, sigma_t, want_x0=True):
    """x, e: [count] tensors (any shape, same dtype); z: [ncand, *x.shape] or None -> (prev [ncand,*], x0)."""
    ncand = 1 if z is None else z.shape[0]
    prev = torch.empty((ncand,) + tuple(x.shape), dtype=x.dtype, device=x.device)
    x0 = torch.empty_like(x) if want_x0 else None
    _call('dts_ddim_candidates', _ptr(x), _ptr(e, 'e', x.dtype), _ptr(z, 'z', x.dtype), _ptr(prev), _ptr(x0), dt_code(x.dtype),
          float(alpha_t), float(alpha_prev), float(sigma_t), ncand, x.numel())
    return prev, x0
