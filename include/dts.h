/* dts.h -- C ABI of libdts_hip.so, the MI355X (gfx950) kernels under the noise-trajectory-search hot path.
 *
 * The reference (rvignav/diffusion-tts) is pure Python on PyTorch: it has NO native code and NO FFI
 * (SURVEY.md, fact 1).  Each entry point below therefore replaces a *sequence of PyTorch ops* at the
 * cited reference call site; the Python host (diffusion_tts_amd/) keeps the reference's own module /
 * function surface on top (INTEGRATION.md shows the binding a maintainer would add).
 *
 * Conventions
 *  - every function returns 0 on success, a negative dts_status otherwise; the message is available
 *    (per thread) from dts_last_error().  Nothing throws across the ABI.
 *  - all pointers are DEVICE pointers owned by the caller (PyTorch allocations); the library never
 *    frees or retains them, never allocates on the launch path, never synchronises.
 *  - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream).
 *  - activations are NHWC ("channels-last"): [n][h][w][c], element type `dtype`
 *    (DTS_F32 parity mode, DTS_BF16 / DTS_F16 throughput modes; accumulation is always f32).
 *  - images/latents at the sampler boundary keep the reference's layout: NCHW, fp64 state
 *    (edm/main.py:99), fp32 denoiser output (networks.py:667), uint8 scorer input (edm/main.py:126).
 */
#ifndef DTS_H_
#define DTS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dts_stream;

enum dts_dtype { DTS_F32 = 0, DTS_BF16 = 1, DTS_F16 = 2,
                 /* dts_conv2d only: SPLIT PRECISION on the 16-bit matrix cores -- the DEFAULT compute mode of the Python surfaces.  Activations
                    and the epilogue operands (bias_nc, residual, out) are f32 tensors; the conv's input is their split image from
                    dts_split3_f16 -- x1 = [n][h][w][2*C] f16, per group of 32 channels 128 bytes = hi(32) | lo * 2^11 (32) with hi = f16(x),
                    lo = x - hi (pass c1 = 2*C, c2 = 0) -- and the packed weight is [cout][taps][2*C] f16, per 32 input channels
                    wh(32) | wl(32) = the hi / lo parts of w * 2^k (acc_scale = 2^-k; the powers of two keep every part a NORMAL f16 number:
                    the matrix cores flush subnormal inputs).  One staged 128-byte K step feeds THREE MFMAs per accumulator tile --
                    wh.hi, (wh * 2^-11).(lo * 2^11), wl.hi -- accumulating, in f32, x_hi*w_hi + x_lo*w_hi + x_hi*w_lo: products exact to
                    ~2^-22 (f16 x f16 carries 22 bits) against 2^-24 of the f32 matrix instruction, which runs at 1/16 of the 16-bit
                    rate.  This is the mode that reproduces the reference's fp32 selections (edm/main.py:842: argmax over rewards that
                    differ by 1e-7) at a third of the 16-bit modes' matrix rate.  (ABI 108 laid the image out as three planes hi | lo | hi
                    against hi | hi * 2^-11 | lo: 1.5 x the bytes, LDS-DMA pieces and fragment reads for the same products.) */
                 DTS_F16X3 = 3 };
enum dts_status { DTS_OK = 0, DTS_ERR_ARG = -1, DTS_ERR_LAUNCH = -2, DTS_ERR_UNSUPPORTED = -3 };

#define DTS_ABI_VERSION 125        /* bumped with every change of a signature or of dts_conv_args (101: ev_start/ev_stop; 102: tuning knobs; 103: dts_cosine_rows; 104: dts_nchw_to_nhwc_pad,
                                     105: dts_conv_args.gn_coef / gn_silu, dts_conv_fuses_gn;
                                     head dim 512 in dts_attention; 106: dts_conv_kernel, 128-cout ping-pong blocks; 107: dts_resample_u8, dts_lut_u8_f32; 108: DTS_F16X3, dts_conv_args.acc_scale, dts_split3_f16, dts_gn_apply_x3, dts_split2_f16, dts_attention_x3;
                                     109: dts_candidate_noise_sd; the DTS_F16X3 operand images are 2*C wide, interleaved per 32 channels; dts_gn_apply_x3 raw_out;
                                     110: dts_candidate_noise_sd takes the three scalars of the reference's product separately (scale [n][3]);
                                     111: dts_conv_args.skip_* (a block's 1x1 skip convolution folded into its second 3x3), dts_conv_folds_skip;
                                     112: dts_resample_fir, dts_space_to_depth2 (the NCSN++ options of SongUNet);
                                     113: dts_cross_attention, dts_layer_norm, dts_geglu (the SD U-Net's transformer blocks);
                                     114: dts_patchify, dts_vit_tokens, dts_gelu, dts_vit_head (the CLIP scorer's vision tower);
                                     115: dts_jpeg_workspace_bytes, dts_jpeg_size (the compressibility scorer's JPEG byte length);
                                     116: dts_group_rows (the SD U-Net's distinct text contexts, grouped on the device);
                                     117: dts_attention_masked, dts_text_tokens (the CLIP text tower: SD's text encoder and the CLIP scorer's text side);
                                     118: dts_layer_norm_x3, dts_gelu_x3, dts_patchify_x3, dts_vit_tokens_f32, dts_vit_head_f32 (the CLIP vision tower in DTS_F16X3);
                                     119: dts_conv_plan (the whole launch plan of a dts_conv2d call, as a query);
                                     120: dts_conv_args.up == 2 (phase-packed weights), dts_conv_takes_phases, dts_conv_plan_info.phases;
                                     121: dts_precond_in (the VP, VE and iDDPM preconditioners);
                                     122: dts_attention_x3_masked, dts_text_tokens_f32 (the CLIP text tower in DTS_F16X3);
                                     123: dts_ode_xhat, dts_ode_slope, dts_ode_correct (the general ODE step of the ablation sampler);
                                     124: dts_candidate_noise_rows (mode / scale per output row: searches of several seeds in lock-step);
                                     125: dts_candidate_noise_sd_rows, dts_ddim_candidates_groups (the SD backend's searches of several seeds in lock-step);
                                     125, domain widened without a signature change: dts_attention (16-bit types) and dts_cross_attention take
                                          head dims 40 / 80 / 160 at their true width (SD-1.x's heads without zero padding); dts_conv_args.up
                                          takes -1 (3x3, stride 2: SD-1.x's downsamplers without space-to-depth; it was read as "upsample" before);
                                     125, entry points added without a change of an existing signature: dts_heun_xhat_rows, dts_heun_euler_rows,
                                          dts_heun_correct_rows (K9 with the step's scalars per row: the MCTS expansions of several seeds' searches,
                                          each at its own sigma step, in one launch); a binding that needs them finds them by name or refuses the library) */
int dts_version(void);            /* == DTS_ABI_VERSION of the build; a binding must refuse any other value */
const char* dts_last_error(void);
/* Tuning knobs (measurement aid; a knob only selects between kernels / block orders / ring depths that give correct results -- the
 * timing-only diagnostic kernels and the A/B experiments that lost (DTS_CONV_VARIANT = 11 .. 91) exist only in builds made with -DDTS_DIAG_KERNELS and are
 * refused by the product library).  knob: index of
 * enum dts_knob in csrc/dts_common.h; value -1 = launcher default.  Used by tools/conv_bench.py and tools/att_bench.py to A/B variants in one process. */
int dts_set_tuning(int knob, int value);
int dts_get_tuning(int knob);

/* ---- layout / packing (weight preparation and test plumbing; not on the per-step path) ------------ */
/* NCHW f32 -> NHWC dtype, and back. */
int dts_nchw_to_nhwc(const float* src, void* dst, int dtype, int n, int c, int h, int w, dts_stream s);
int dts_nhwc_to_nchw(const void* src, int dtype, float* dst, int n, int c, int h, int w, dts_stream s);
/* NCHW f32 -> NHWC dtype with the channel count padded to cpad (zeros): SD latents (4 channels) feeding the MFMA conv (cin % 64 == 0). */
int dts_nchw_to_nhwc_pad(const float* src, void* dst, int dtype, int n, int c, int h, int w, int cpad, dts_stream s);
/* OIHW f32 conv weight (torch layout, networks.py:62 / unet.py conv_nd) -> [O][kh][kw][I] dtype.
 * out_perm (device int32[O], nullable): packed row o is taken from source row out_perm[o]; used to
 * regroup the qkv projection's output channels into q|k|v blocks (networks.py:182, unet.py:365). */
int dts_pack_conv_weight(const float* w_oihw, void* dst, int dtype, int O, int I, int kh, int kw,
                         const int32_t* out_perm, dts_stream s);

/* ---- K1/K2/K3: implicit-GEMM convolution on MFMA (networks.py:68-90 Conv2d.forward) --------------- */
typedef struct dts_conv_args {
  const void* x1; int32_t c1;     /* input, NHWC [n][hin][win][c1] */
  const void* x2; int32_t c2;     /* optional 2nd input concatenated on channels (networks.py:458 torch.cat); c2=0 if none */
  const void* w;                  /* packed weight [cout][ksize*ksize][c1+c2] */
  const float* bias;              /* [cout] or NULL */
  const void* bias_nc;            /* per-sample per-channel addend [n][ld_bias_nc] (dtype) or NULL (networks.py:175 x.add_(params)) */
  int32_t ld_bias_nc;
  const void* residual;           /* NHWC [n][hout][wout][cout] or NULL (networks.py:178,185) */
  void* out;                      /* NHWC [n][hout][wout][cout] */
  int32_t n, hin, win;
  int32_t cout;
  int32_t ksize;                  /* 1 or 3 (pad ksize/2, stride 1) */
  int32_t up;                     /* 1: nearest 2x upsample of the input fused into the gather (networks.py:82-83);
                                     2 (DTS_F16X3, ksize 3 only): the same convolution as four 2x2 convolutions over the low-resolution input, one
                                     per output phase (py, px) = (y & 1, x & 1).  `w` is then the phase-packed weight [4][cout][2][2][c1]: phase
                                     2*py + px, taps (ty, tx) row-major at the low-resolution offsets (ty - 1 + py, tx - 1 + px), each tap the sum
                                     of the 3x3 taps that fall on that input pixel (rows, py = 0: {w0, w1+w2}; py = 1: {w0+w1, w2}; columns
                                     alike), `acc_scale` that tensor's power of two; the output is [n][2*hin][2*win][cout] as for 1, 4/9 of the
                                     multiply-adds.  Only launches for which dts_conv_takes_phases() returns 1 accept it;
                                     -1 (DTS_F16 / DTS_BF16, ksize 3 only): zero padding 1, STRIDE 2 (an SD Downsample2D): the output is
                                     [n][(hin+1)/2][(win+1)/2][cout], output pixel (i, j) reads input rows 2i-1 .. 2i+1 and columns 2j-1 .. 2j+1, taps
                                     outside the image are zero; odd sizes are allowed.  `w` is the ordinary packed 3x3 weight.  x2 / c2, bias,
                                     bias_nc, residual (at the output size), out_scale, stats_out (hout*wout % 64 == 0), workspace (K split) and
                                     the timing events work as for 0; DTS_F32, DTS_F16X3, ksize 1, gn_coef, skip_*, out_split2 and an acc_scale
                                     other than 0 / 1 are refused.  Always conv_igemm_kernel (dts_conv_kernel 0; the three queries below answer
                                     0), with 4 | 8 waves and a 2- | 3-deep ring: DTS_CONV_STAGES=4 runs the 3-deep ring, and dts_conv_plan reports
                                     what runs.  Values below -1 are refused */
  float out_scale;                /* out = (conv + bias + bias_nc + residual) * out_scale  (networks.py:179,186 skip_scale) */
  int32_t dtype;
  void* workspace;                /* optional scratch (16-byte aligned) for split-K partial sums; NULL disables split-K */
  int64_t workspace_bytes;
  float* stats_out;               /* optional [ceil(P/64)][cout][2] f32: per 64-pixel strip (sum, sumsq) of the stored outputs,
                                     the GroupNorm moments of the NEXT layer fused into this epilogue (needs hout*wout % 64 == 0) */
  int32_t stats_written;          /* OUT: 1 whenever stats_out was filled -- by the fused epilogue, or by the reduce pass of a split-K launch;
                                     0: the statistics were not produced (tile variant without 64-pixel wave strips): run dts_gn_coef */
  void* ev_start; void* ev_stop;  /* optional hipEvent_t pair attached to the conv kernel's own dispatch (start / end of that kernel, as a
                                     kernel trace sees it; no barrier packets between launches).  Measurement only: bench.py's roofline leg */
  const float* gn_coef;           /* optional [n][c1+c2][2] f32 (a, b) from dts_gn_coef / dts_gn_coef_strips: the GroupNorm (+ adaptive
                                     scale/shift) of the INPUT, applied as act(x*a + b) while the conv stages its input tile, so the
                                     normalised tensor is never written (networks.py:168,173-175 feeding conv0 / conv1).  Only launches
                                     for which dts_conv_fuses_gn() returns 1 accept it; padding stays zero (the reference pads AFTER the norm) */
  int32_t gn_silu;                /* 1: act = SiLU, 0: identity */
  float acc_scale;                /* DTS_F16X3 only (0 = 1): out = (conv * acc_scale + bias + bias_nc + residual) * out_scale; undoes the power of
                                     two the packed split-precision weights carry */
  int32_t out_split2;             /* DTS_F16X3 only: 1 = `out` is f16 [n][hout][wout][2*cout] = hi(cout) | lo(cout) of the result * 2^6 per pixel, saturating (the
                                     image dts_split2_f16 would make of it: the qkv projection feeding dts_attention_x3) instead of f32 [..][cout] */
  /* DTS_F16X3 only: the UNetBlock's 1x1 skip convolution (networks.py:164,177: x = conv1(..) + skip(orig)) accumulated by the SAME launch, as a
     second K loop over the block input behind the 3x3 taps: out = ((conv + skip_conv) + bias) * out_scale with `bias` = the two layers' biases
     added by the caller and no `residual`.  Only launches for which dts_conv_folds_skip() returns 1 accept it. */
  int32_t skip_c;                 /* f16 elements per pixel of skip_x (= 2 x the skip conv's input channels), a multiple of 64; 0 = no fold */
  const void* skip_x;             /* split image of the block input, f16 [n][hout >> skip_up][wout >> skip_up][skip_c] */
  const void* skip_w;             /* the 1x1 layer's packed split-precision weight [cout][skip_c] */
  float skip_acc_scale;           /* that weight's power of two (0 = 1), like acc_scale */
  int32_t skip_up;                /* 1: skip_x is at half the output resolution (the nearest-2x upsample of networks.py:82-83 fused into the gather) */
} dts_conv_args;
/* 1 if dts_conv2d would apply a->gn_coef inside the conv for this shape / dtype (3x3, cout % 192 == 0, 16-bit, square power-of-two
 * images >= 16, whole 256-pixel tiles, no fused upsample), else 0: the caller then runs dts_gn_apply first. */
int dts_conv_fuses_gn(const dts_conv_args* a);
/* 1 if dts_conv2d accepts a->skip_* for this launch (DTS_F16X3, 3x3 on the ping-pong kernel with a grid that needs no K split, no residual /
 * out_split2 / upsample of x1), else 0: the caller then runs the 1x1 layer as its own launch and passes its output as `residual`. */
int dts_conv_folds_skip(const dts_conv_args* a);
/* 1 if dts_conv2d accepts a->up == 2 for this launch (DTS_F16X3, 3x3, cout a multiple of 128 or 192, no x2 / gn_coef / skip_* / out_split2,
 * a grid that neither wants nor is forced to a K split, hin*win % 64 == 0 when stats_out is given, DTS_CONV_UP_PHASES not 0), else 0: the
 * caller then passes the 3x3 weight with up = 1.  A residual is allowed. */
int dts_conv_takes_phases(const dts_conv_args* a);
/* which kernel dts_conv2d takes for these arguments (shape, dtype, residual / gn_coef presence; tuning knobs included): 0 = the 4-wave
 * implicit-GEMM kernel, 6 / 4 = the 8-wave ping-pong / halo kernel with 192- / 128-cout blocks, -1 = invalid arguments.  Measurement aid:
 * bench.py attributes its per-launch times and algorithmic bytes to the kernel name a trace will show. */
int dts_conv_kernel(const dts_conv_args* a);
/* The whole launch plan of dts_conv2d for these arguments, as the launcher itself derives it (host only: no GPU needed; the three queries
 * above return fields of the same plan).  Reads the shape, the dtype, the tuning knobs and which of residual / gn_coef / skip_* /
 * stats_out / out_split2 / workspace (+ workspace_bytes) are present; pointers are never dereferenced.  Returns DTS_ERR_ARG where
 * dts_conv_kernel answers -1, else DTS_OK; `refused` = 1: dts_conv2d refuses the call (dts_last_error says why) and the fields after
 * the first refusing rule are not filled.  Measurement and test aid. */
typedef struct dts_conv_plan_info {
  int32_t kernel;                         /* as dts_conv_kernel: 0 / 6 / 4, -1 = invalid arguments */
  int32_t tile, waves, stages, pf;        /* conv_igemm_kernel: cout tile 64 | 128 | 192, waves 4 | 8, LDS ring depth 2 | 3 | 4, fragment prefetch; 0 otherwise */
  int32_t gn, sk, dbg;                    /* conv_pp_kernel: fused GroupNorm apply, folded skip convolution, diagnostic form (0 in the product library) */
  int32_t splits, ks_per_split;           /* K split (grid.y; > 1: f32 partial slabs + the reduce pass) and K steps per split */
  int32_t n_ct, n_pt, nblk;               /* cout tiles, pixel tiles, grid.x = n_ct * n_pt (phases = 1: tiles of low-resolution pixels, grid.x = 4 * n_ct * n_pt) */
  int32_t threads, lds_bytes;             /* block size, dynamic LDS */
  int32_t stats_in_kernel, stats_in_reduce, stats_written;      /* who writes stats_out; stats_written as dts_conv2d will report it */
  int32_t epi_rows;                       /* f32 outputs: 1 / 2 = a row-layout epilogue, 0 = the accumulator-layout one */
  int32_t fuses_gn, folds_skip;           /* as dts_conv_fuses_gn / dts_conv_folds_skip */
  int32_t refused;
  int32_t phases;                         /* 1: the phase form of conv_igemm_kernel (up == 2), else 0 */
} dts_conv_plan_info;
int dts_conv_plan(const dts_conv_args* a, dts_conv_plan_info* out);
int dts_conv2d(dts_conv_args* a, dts_stream s);      /* writes a->stats_written; no state is kept between calls (thread-safe) */

/* first / last convolutions of the U-Nets (3 image channels; direct, not MFMA) */
/* x f32 NCHW [n][3][h][w] -> out NHWC [n][h][w][cout]; w f32 OIHW [cout][3][3][3] */
int dts_conv_in3(const float* x, const float* w, const float* bias, void* out, int dtype,
                 int n, int h, int w_, int cout, dts_stream s);
/* x NHWC [n][h][w][c] -> out f32 NCHW [n][3][h][w]; w f32 [3][3][3][c] (O,kh,kw,I) */
int dts_conv_out3(const void* x, int dtype, const float* w, const float* bias, float* out,
                  int n, int h, int w_, int c, dts_stream s);

/* ---- K4/K5: GroupNorm (+ adaptive scale/shift, SiLU, 2x2 avg-pool) (networks.py:104-106,168-175) -- */
/* number of floats of workspace dts_gn_coef needs */
int64_t dts_gn_ws_floats(int n, int groups);
/* coef[n][C][2] = (a, b) such that groupnorm(x)*gamma+beta [*(1+scale)+shift] == x*a + b.
 * x = concat(x1, x2) on channels; scale_shift (dtype, [n][ld_ss], scale = [0,C), shift = [C,2C)) may be NULL. */
int dts_gn_coef(const void* x1, int c1, const void* x2, int c2, int dtype, int n, int hw, int groups, float eps,
                const float* gamma, const float* beta, const void* scale_shift, int ld_ss,
                float* coef, float* ws, dts_stream s);
/* same coefficients from strip statistics emitted by dts_conv2d (stats_out) for each source: st1 [n*hw/64][c1][2],
 * st2 [n*hw/64][c2][2] (NULL when c2 == 0); no pass over x at all. */
int dts_gn_coef_strips(const float* st1, int c1, const float* st2, int c2, int dtype, int n, int hw, int groups, float eps,
                       const float* gamma, const float* beta, const void* scale_shift, int ld_ss, float* coef, dts_stream s);
/* out = act(x*a + b); pool=1 averages 2x2 pixel blocks after the activation (resample filter [1,1],
 * networks.py:84-85; unet.py:213-215 avg_pool) and writes [n][h/2][w/2][C]. */
int dts_gn_apply(const void* x1, int c1, const void* x2, int c2, int dtype, const float* coef,
                 void* out, int n, int h, int w, int silu, int pool, dts_stream s);
/* the same pass in the split-precision mode (DTS_F16X3): x / coef as above in f32, out = the f16 split image [n][h'][w'][2*C] (per 32
 * channels hi | lo * 2^11, the arithmetic and layout of dts_split3_f16) that dts_conv2d(dtype = DTS_F16X3) reads -- the f32 normalised
 * tensor is never written.  C a multiple of 32.  raw_out (optional, same shape as out): the split image of the UN-normalised input rows
 * (2x2-averaged like dts_resample2x when pool = 1) is written by the same pass -- the operand of the block's 1x1 skip convolution
 * (networks.py:177), bit-identical to dts_split3_f16 of the (resampled) input. */
int dts_gn_apply_x3(const float* x1, int c1, const float* x2, int c2, const float* coef, void* out, void* raw_out, int n, int h, int w, int silu,
                    int pool, dts_stream s);
/* single-launch variant for low-resolution levels (hw <= ~256): statistics + apply in one kernel, one block per
 * (group, sample); same result as dts_gn_coef + dts_gn_apply(pool=0).  Channels per group must be even and <= 64. */
int dts_gn_fused(const void* x1, int c1, const void* x2, int c2, int dtype, int n, int hw, int groups, float eps,
                 const float* gamma, const float* beta, const void* scale_shift, int ld_ss, void* out, int silu, dts_stream s);
/* 2x resampling of an NHWC tensor for the skip path: mode 0 = 2x2 average (down), 1 = nearest (up). */
int dts_resample2x(const void* x, void* out, int dtype, int n, int h, int w, int c, int mode, dts_stream s);
/* The same resampling with the NCSN++ filter, resample_filter = [1,3,3,1] (networks.py:64-65,82-85), F = outer(k,k) / 64:
 *   up = 0: out [n][h/2][w/2][c] = conv2d(x, F, stride 2, padding 1) per channel;
 *   up = 1: out [n][2h][2w][c] = conv_transpose2d(x, 4F, stride 2, padding 1) per channel (per axis: 3/4 of the nearer source pixel, 1/4 of
 *           the farther one); pixels outside the image count as zero.
 * c a multiple of the 16-byte vector (4 f32 / 8 16-bit elements).  split_out = 1 (dtype DTS_F32, c % 32 == 0): `out` is the f16 split
 * operand image [..][2*c] of the result (dts_split3_f16's arithmetic and layout), what dts_conv2d(dtype = DTS_F16X3) reads. */
int dts_resample_fir(const void* x, void* out, int dtype, int n, int h, int w, int c, int up, int split_out, dts_stream s);
/* out [n][h/2][w/2][cpad], out[..][i][j][(ry*2 + rx)*c + ci] = x[..][2i+ry][2j+rx][ci], channels 4c .. cpad-1 zero.  x is NHWC in `dtype`, or
 * (x_nchw_f32 = 1) the f32 NCHW image at the U-Net's input.  With it the residual encoder's fused-resample convolution (networks.py:78-80,
 * 290-292: 3x3 with padding 2, then F at stride 2 without padding) is ONE dts_conv2d: the two steps compose into a 6x6 stride-2 padding-2
 * convolution, which over this rearrangement is a 3x3 padding-1 convolution of 4c channels (ops.fused_down_weight builds its weight).
 * cpad >= 4c, a multiple of dts_conv2d's channel granularity; split_out as in dts_resample_fir (cpad % 32 == 0). */
int dts_space_to_depth2(const void* x, int x_nchw_f32, void* out, int dtype, int n, int h, int w, int c, int cpad, int split_out, dts_stream s);

/* ---- K6: fused self-attention (networks.py:113-118,181-185; unet.py:355-372,388-407) -------------- */
/* qkv NHWC-flattened [n][t][3*heads*d] laid out q[heads][d] | k[heads][d] | v[heads][d];
 * out [n][t][heads*d]; softmax(q.k * scale) in f32; any t >= 1.  Head dims per dtype:
 *   DTS_F32            d in {64, 128, 256};
 *   DTS_BF16 / DTS_F16 d in {64, 128, 256}, 512 (the SD VAE's mid block) and 40, 80, 160 (the heads of SD-1.x's U-Net).
 * 40 / 80 / 160 are laid out like every other d: at the TRUE head dim, nothing padded in memory (a head's row is 80 / 160 / 320 bytes, whole
 * 16-byte chunks).  The zero-tail rule: on chip the K dimension of Q.K^T is d rounded up to 32 (64 / 96 / 160) and the 16-byte chunks at or
 * beyond d/8 of a Q fragment, K row or V row are zeros that are never loaded; P.V covers d rounded up to 16 channels and only channels < d are
 * stored.  A zero tail adds exact zeros to the f32 scores, so the result has the bits of the same call on values zero-padded per head to
 * 64 / 128 / 256 (with the scale of the true d).  Every other d returns an error that names it. */
int dts_attention(const void* qkv, void* out, int dtype, int n, int t, int heads, int d, float scale, dts_stream s);
/* the same attention in the split-precision mode (DTS_F16X3; d = 64): qkv_split = dts_split2_f16 of the f32 qkv tensor, f16 [n][t][6*heads*d] =
 * hi(3C) | lo(3C) per token (also what dts_conv2d writes with out_split2); out f32 [n][t][heads*d], or with out_split3 = 1 the f16 operand
 * image [n][t][2*heads*d] (per 32 channels hi | lo * 2^11: dts_split3_f16's arithmetic and layout) the proj convolution reads.  Q.K^T and P.V on the 16-bit matrix cores with hi/lo operand pairs (the lo*lo term,
 * 2^-22, dropped), softmax in f32: the f32 kernel's accuracy without the f32 matrix instruction's 1/16 rate. */
int dts_attention_x3(const void* qkv_split, void* out, int out_split3, int n, int t, int heads, int d, float scale, dts_stream s);
/* Masked self-attention (CLIP's text transformer); layout as dts_attention.  Query i of sample b attends key j iff
 * (!causal || j <= i) && (key_len == NULL || j < key_len[b]).  key_len: device int32 [n], nullable; the caller vouches for
 * 1 <= key_len[b] <= t (the kernel clamps it for memory safety only), so every query has key 0 and no row is empty.  causal = 0 with
 * key_len = NULL is plain attention.  DTS_BF16 / DTS_F16 with d = 64 (every CLIP text width: 512/8, 768/12, 1024/16, 1280/20); DTS_F32 and
 * other head dims return DTS_ERR_UNSUPPORTED; any t >= 1; scale > 0.  The arithmetic is dts_attention's in the 16-bit types (f32 scores, f32
 * softmax with exp2, P rounded to the storage type, the denominator summed from the rounded P, one final rounding).  The mask is a select to
 * -inf on the scores, not an additive bias: a disallowed key has weight exactly 0, and finite k / v values there cannot change a bit of
 * the output.  Key tiles wholly above a query block's diagonal or wholly past key_len are skipped, not computed and masked. */
int dts_attention_masked(const void* qkv, void* out, int dtype, int n, int t, int heads, int d, float scale, int causal,
                         const int32_t* key_len, dts_stream s);
/* dts_attention_masked in the split-precision mode (the CLIP text tower in DTS_F16X3): dts_attention_x3's operand (qkv_split) and output
 * forms (f32 rows, or with out_split3 = 1 the proj convolution's operand image), its arithmetic and its 2 GiB limit on a sample's rows;
 * dts_attention_masked's mask, causal / key_len contract and refusals (d = 64 only, scale positive and finite, tensors 16-byte and key_len
 * 4-byte aligned); any t >= 1; causal = 0 with key_len = NULL is plain attention, bit for bit dts_attention_x3's one-query-tile form.  The
 * mask is a select to -inf on the f32 scores: a hidden key has P = 0 exactly, so both halves of its split are 0 and finite k / v values
 * there (|x| < 1023, the image's range) cannot change a bit of the output.  Rows between key_len and t are read like any other; key tiles
 * wholly above a query block's diagonal or wholly past key_len are skipped, not computed and masked. */
int dts_attention_x3_masked(const void* qkv_split, void* out, int out_split3, int n, int t, int heads, int d, float scale, int causal,
                            const int32_t* key_len, dts_stream s);

/* ---- K15-K17: the SD U-Net's transformer blocks (diffusers BasicTransformerBlock: attention.py, attention_processor.py) ---- */
/* Attention of tq queries over a SHORT foreign sequence (the text tokens): q [n][tq][heads*d], kv [kv_n][tk][2*heads*d] laid out
 * k[heads][d] | v[heads][d], out [n][tq][heads*d]; DTS_BF16 / DTS_F16; softmax(q.k * scale) in f32, Q.K^T and P.V on the 16-bit matrix
 * cores.  1 <= tk <= 128 (any length: the tail is masked): K and V of a (sample, head) sit in LDS at once, one pass over the keys, no online
 * rescale; a longer tk returns DTS_ERR_UNSUPPORTED.  d in {40, 64, 80, 128, 160, 256} in both dtypes; any tq >= 1; scale > 0.  40 / 80 / 160
 * are stored at the true head dim in q, kv and out, and follow dts_attention's zero-tail rule (K width 64 / 96 / 160 on chip, tail chunks zero
 * and never loaded, channels < d stored; LDS per block 2 * tkp * (2 * width + 32) bytes): the bits of the call on zero-padded heads.
 * kv_rows (device int32 [n], nullable): sample i attends to kv row kv_rows[i] (the 2N rows of the search loop share two text contexts:
 * their k|v projections are computed once each and never expanded); NULL: kv_n == n and sample i reads row i.  Entries must lie in
 * [0, kv_n); the kernel clamps them for memory safety only. */
int dts_cross_attention(const void* q, const void* kv, const int32_t* kv_rows, int kv_n, void* out, int dtype, int n, int tq, int tk,
                        int heads, int d, float scale, dts_stream s);
/* out[r][:] = (x[r][:] - mean_r) / sqrt(var_r + eps) * gamma + beta over rows of c channels (biased variance, as torch.nn.LayerNorm);
 * DTS_BF16 / DTS_F16 in and out, statistics in f32 (two passes over the row in registers), gamma / beta f32 [c]; c % 8 == 0, c <= 2048. */
int dts_layer_norm(const void* x, void* out, int dtype, int64_t rows, int c, float eps, const float* gamma, const float* beta, dts_stream s);
/* GEGLU (diffusers activations.py GEGLU): x [rows][2*inner] -> out[r][j] = x[r][j] * gelu(x[r][inner + j]), the exact (erf) GELU;
 * DTS_BF16 / DTS_F16 storage, f32 arithmetic; inner % 8 == 0. */
int dts_geglu(const void* x, void* out, int dtype, int64_t rows, int inner, dts_stream s);
/* Groups of bitwise-identical rows, numbered in order of first occurrence: what torch.unique(rows, dim=0, return_inverse=True) over the int16
 * view of encoder_hidden_states gave SDUNet._context_kv (sd_unet.py), without its row sort and without a host synchronisation of its own.
 * rows: n contiguous rows of row_bytes bytes; 1 <= n <= 1024, row_bytes % 16 == 0 (anything else returns DTS_ERR_UNSUPPORTED); 16-byte aligned.
 * slot int32 [n]: the group of row i (slot[0] == 0); reps int32 [n]: reps[g] = the first row of group g for g < count, -1 from count on;
 * count int32 [1]: the number of distinct rows.  workspace: 16 * n bytes, 16-byte aligned (one 128-bit fingerprint per row).
 * Equality is equality of the bytes (+0.0 and -0.0 differ, equal NaN payloads are equal).  Two launches: a fingerprint per row, then one block
 * that compares every row with the earlier rows of the same fingerprint, byte for byte, until one matches -- a fingerprint match is never
 * taken as equality, so the result is exact for any input.  Integer arithmetic only: two runs give the same bits. */
int dts_group_rows(const void* rows, int n, int64_t row_bytes, void* workspace, int32_t* slot, int32_t* reps, int32_t* count, dts_stream s);

/* ---- K18-K21: the CLIP scorer's vision tower (transformers models/clip/modeling_clip.py: CLIPVisionEmbeddings, CLIPMLP, the pooled head) ---- */
/* Patch rows for the patch embedding Conv2d(3, hidden, patch, stride = patch, bias = False): x f32 NCHW [n][3][size][size] (pixel_values) ->
 * out [n][g*g][kpad] in DTS_BF16 / DTS_F16, g = size / patch; column (c*patch + py)*patch + px = x[n][c][gy*patch + py][gx*patch + px] rounded
 * once (nearest-even) -- the flattening order of the conv weight [hidden][3][patch][patch] -- and columns 3*patch*patch .. kpad-1 are written
 * as zeros.  kpad % 8 == 0 (in use: 3*patch*patch rounded up to dts_conv2d's 64-channel granularity, 588 -> 640 at patch 14), size % patch == 0.
 * The source is read element-wise (a patch row of 14 floats is not 16-byte aligned); out is stored in whole 16-byte vectors.  The embedding
 * itself is one 1x1 dts_conv2d over [n][g][g][kpad] with the weight flattened and zero-padded the same way. */
int dts_patchify(const float* x, void* out, int dtype, int n, int size, int patch, int kpad, dts_stream s);
/* tokens [n][t][c]: tokens[n][0] = cls + pos[0], tokens[n][1 + p] = patches[n][p] + pos[1 + p]; patches [n][t-1][c] and tokens in DTS_BF16 /
 * DTS_F16, cls f32 [c], pos f32 [t][c] (CLIPVisionEmbeddings: class_embedding, position_embedding.weight); the sum is formed in f32 and rounded
 * once.  c % 8 == 0, t >= 2. */
int dts_vit_tokens(const void* patches, const float* cls, const float* pos, void* tokens, int dtype, int n, int t, int c, dts_stream s);
/* Elementwise GELU over `count` 16-bit values (count % 8 == 0; out may be x): kind 0 = quick-GELU x * sigmoid(1.702 x) (hidden_act of the OpenAI
 * CLIP checkpoints), kind 1 = the exact (erf) GELU x * erfc(-x / sqrt 2) / 2 (the LAION towers).  f32 arithmetic; finite over the whole storage
 * range (the most negative finite input gives -0, not inf * 0). */
int dts_gelu(const void* x, void* out, int dtype, int64_t count, int kind, dts_stream s);
/* The text counterpart of dts_vit_tokens (CLIPTextEmbeddings): out [n][t][c] in DTS_BF16 / DTS_F16 = tok[ids[n][t]][:] + pos[t][:], tok f32
 * [vocab][c] (token_embedding.weight), pos f32 [>= t][c] (position_embedding.weight), ids device int32 [n][t]; the sum is formed in f32 and
 * rounded once.  c % 8 == 0.  Ids must lie in [0, vocab): the kernel cannot report a bad one and clamps it for memory safety only -- check
 * them on the host before the upload. */
int dts_text_tokens(const int32_t* ids, const float* tok, const float* pos, void* out, int dtype, int n, int t, int c, int vocab, dts_stream s);
/* Pooled head, first half: out f32 [n][c] = LayerNorm(tokens[n][0][:]) * gamma + beta (CLIPVisionTransformer post_layernorm of the class token;
 * biased variance, statistics in f32 as dts_layer_norm) -- token 0 only, the other t - 1 tokens are never read.  tokens [n][t][c] DTS_BF16 /
 * DTS_F16; c % 8 == 0, c <= 2048.  visual_projection follows as dts_linear on the f32 rows. */
int dts_vit_head(const void* tokens, float* out, int dtype, int n, int t, int c, float eps, const float* gamma, const float* beta, dts_stream s);

/* ---- the CLIP vision tower in the split-precision mode (DTS_F16X3): f32 activations; a result whose only reader is a split-precision 1x1
 * dts_conv2d leaves as that convolution's operand image, bit for bit what dts_split3_f16 makes of the f32 values (f16 [rows][2*c], per 32
 * channels hi(32) | lo * 2^11 (32)), and the f32 tensor is not written.  All pointers 16-byte aligned. ---- */
/* torch.nn.LayerNorm (CLIPEncoderLayer.layer_norm1 / layer_norm2, CLIPVisionTransformer.pre_layrnorm) over f32 rows [rows][c]: biased variance
 * as the mean of (x - mean)^2 over the row in registers, one wave per row; the statistics and (x - mean) * rstd * gamma + beta are formed in f64
 * and rounded once to f32 (an f32 rstd's rounding error would scale every output of the row); gamma / beta f32 [c].  out_f32 (nullable): the normalised rows f32
 * [rows][c] (pre_layrnorm: the residual stream); out_split (nullable): their operand image f16 [rows][2*c] (the qkv and fc1 projections'
 * operand) -- the same bits whether or not out_f32 is written.  At least one of the two; c % 32 == 0, c <= 2048. */
int dts_layer_norm_x3(const float* x, float* out_f32, void* out_split, int64_t rows, int c, float eps, const float* gamma, const float* beta,
                      dts_stream s);
/* CLIPMLP's activation_fn between fc1 and fc2: x f32 [rows][c] -> the operand image f16 [rows][2*c] of act(x); kind as dts_gelu (0 = quick-GELU
 * x / (1 + exp(-1.702 x)), 1 = the erf GELU x * erfc(-x / sqrt 2) / 2: both finite over the whole f32 range).  c % 32 == 0. */
int dts_gelu_x3(const float* x, void* out_split, int64_t rows, int c, int kind, dts_stream s);
/* dts_patchify's gather for the split-precision patch embedding: x f32 NCHW [n][3][size][size] -> the operand image f16 [n][g*g][2*kpad] of the
 * unrounded patch rows, same column order (c*patch + py)*patch + px, columns 3*patch*patch .. kpad-1 written as zeros.  kpad % 32 == 0. */
int dts_patchify_x3(const float* x, void* out_split, int n, int size, int patch, int kpad, dts_stream s);
/* dts_vit_tokens in f32 (CLIPVisionEmbeddings: cat([class_embedding, patch_embeds], 1) + position_embedding): tokens f32 [n][t][c], tokens[n][0] =
 * cls + pos[0], tokens[n][1 + p] = patches[n][p] + pos[1 + p] -- one f32 add per element; patches f32 [n][t-1][c].  c % 4 == 0, t >= 2. */
int dts_vit_tokens_f32(const float* patches, const float* cls, const float* pos, float* tokens, int n, int t, int c, dts_stream s);
/* dts_vit_head over f32 tokens [n][t][c] (post_layernorm of the class token): out f32 [n][c] = LayerNorm(tokens[n][0][:]) * gamma + beta with
 * dts_layer_norm_x3's arithmetic, one wave per sample; the other tokens are never read.  c % 8 == 0, c <= 2048.  dts_linear follows. */
int dts_vit_head_f32(const float* tokens, float* out, int n, int t, int c, float eps, const float* gamma, const float* beta, dts_stream s);
/* dts_text_tokens in f32 (the text tower's counterpart of dts_vit_tokens_f32): out f32 [n][t][c] = tok[ids[n][t]][:] + pos[t][:], one f32 add
 * per element; ids as there (checked on the host, clamped here for memory safety only).  c % 8 == 0. */
int dts_text_tokens_f32(const int32_t* ids, const float* tok, const float* pos, float* out, int n, int t, int c, int vocab, dts_stream s);

/* ---- K7/K8: embedding MLP pieces and EDM preconditioning (networks.py:200-206,437-447,654-668) ---- */
/* y[m][n] = act_out( act_in(x[m][:]) . w[n][:] + bias[n] (+ y[m][n] if accumulate) ); all f32; act: 0 none, 1 SiLU */
int dts_linear(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy,
               int m, int k, int n, int act_in, int act_out, int accumulate, dts_stream s);
/* out[n][0:half] = cos(v[n]*freqs), out[n][half:2half] = sin(..) (swap=1: sin first, networks.py:323) */
int dts_pos_embedding(const float* v, const float* freqs, float* out, int n, int half, int swap, dts_stream s);
/* coef[n][4] = (c_skip, c_out, c_in, c_noise) in f32 from sigma (f64, nsigma = 1 or n); xin = c_in * f32(x) */
int dts_edm_precond_in(const double* x, const double* sigma, int nsigma, float sigma_data,
                       float* xin, float* coef, int n, int chw, dts_stream s);
/* The other three preconditioners (networks.py:495-509 VP, 548-562 VE, 601-625 iDDPM): the same coef[n][4] = (c_skip, c_out, c_in, c_noise)
 * and xin = c_in * f32(x), so dts_edm_precond_out serves every kind.  c_skip = 1 throughout;
 *   VP:    c_out = -s, c_in = 1 / sqrt(s^2 + 1), c_noise = (M-1) * ((sqrt(beta_min^2 + 2 beta_d * log(1 + s^2)) - beta_min) / beta_d)
 *   VE:    c_out =  s, c_in = 1,                 c_noise = log(0.5 * s)
 *   iDDPM: c_out, c_in as VP,                    c_noise = (M-1) - j, j = the index of the entry of table[0:table_n] (f32, device) nearest to s:
 *          the exact |s - table[j]|, the first index on a tie (the reference's torch.cdist takes a matrix-product route for a long table and
 *          can miss the nearest entry of a near-tie: INTEGRATION.md section 1)
 * with s = f32(sigma[row]).  float32 arithmetic, one rounding per tensor operation of the reference's expression and in its order, no fused
 * multiply-add.  params: HOST array of DTS_PRECOND_NPARAMS floats, read during the call, each a Python-scalar sub-expression of the reference
 * evaluated in double and rounded once: {M-1, beta_min^2, 2*beta_d, beta_min, beta_d} (VP: all five; iDDPM: [0]; VE: unread, may be NULL).
 * Two launches on `s` (coefficients: one wavefront per row; then the scaling pass), no host read: capturable into a HIP graph. */
enum dts_precond_kind { DTS_PRECOND_VP = 1, DTS_PRECOND_VE = 2, DTS_PRECOND_IDDPM = 3 };
#define DTS_PRECOND_NPARAMS 5
int dts_precond_in(int kind, const float* params, const float* table, int table_n, const double* x, const double* sigma, int nsigma,
                   float* xin, float* coef, int n, int chw, dts_stream s);
/* D = c_skip*f32(x) + c_out*F  (f32, NCHW) */
int dts_edm_precond_out(const double* x, const float* F, const float* coef, float* D, int n, int chw, dts_stream s);
/* split-precision operand image for dts_conv2d(dtype = DTS_F16X3): row p of concat(x1, x2) (f32 rows of c1 / c2 channels, x2 may be NULL
 * with c2 = 0; c1, c2 multiples of 8, C = c1 + c2 a multiple of 32) -> out[p][64*g + j] = hi, out[p][64*g + 32 + j] = lo * 2^11 of channel
 * 32*g + j: hi = f16(x) (0 when that would be subnormal; +-65504 beyond the f16 range), lo = f16((x - hi) * 2^11).  out: f16 [rows][2*C]. */
int dts_split3_f16(const float* x1, int c1, const float* x2, int c2, void* out, int64_t rows, dts_stream s);
/* out[p][0:c] = hi, [c:2c] = lo of x[p][:] * 2^6 (hi = f16(y), lo = f16(y - hi); |y| saturates at 65504, i.e. |x| at 1023.5): the operand image of dts_attention_x3 */
int dts_split2_f16(const float* x, int c, void* out, int64_t rows, dts_stream s);
/* f32 -> dtype cast of a dense array (embedding -> activation dtype) and back */
int dts_cast_from_f32(const float* src, void* dst, int dtype, int64_t count, dts_stream s);
int dts_cast_to_f32(const void* src, int dtype, float* dst, int64_t count, dts_stream s);

/* ---- K9: fused Heun / Euler ODE step with churn, fp64 state (edm/main.py:82-96) ------------------- */
/* x_hat[nb] = x_cur[src(i)] + noise_coef * eps[i];  src(i) = i % xb (bcast=0, Tensor.repeat, edm/main.py:803)
 * or i / (nb/xb) (bcast=1, repeat_interleave, edm/main.py:107).  eps is f64 (eps_f32=0) or f32 (edm/main.py:446). */
int dts_heun_xhat(const double* x_cur, int xb, int bcast, const void* eps, int eps_f32, double noise_coef,
                  double* x_hat, int nb, int chw, dts_stream s);
/* d_cur = (x_hat - D)/t_hat ; x_next = x_hat + (t_next - t_hat)*d_cur */
int dts_heun_euler(const double* x_hat, const float* D, double t_hat, double t_next,
                   double* d_cur, double* x_next, int64_t count, dts_stream s);
/* x_next = x_hat + (t_next - t_hat)*(0.5*d_cur + 0.5*(x_next - D2)/t_next)   (in place on x_next) */
int dts_heun_correct(const double* x_hat, const float* D2, const double* d_cur, double t_hat, double t_next,
                     double* x_next, int64_t count, dts_stream s);
/* The per-row forms of the three: noise_coef[nb], t_hat[n], t_next[n] are float64 DEVICE arrays, one entry per row of chw elements, read
 * by the kernel and never by the host (the launches stay capturable).  Row i holds, bit for bit, what the scalar entry point computes for
 * that row when launched with noise_coef[i], t_hat[i], t_next[i]: one body per op, the scalar entry is its broadcast case; a row with
 * noise_coef[i] == 0.0 is its source row of x_cur unchanged.  t_hat[i] != 0 (euler) and t_next[i] != 0 (correct) are the CALLER's to
 * check on its host copy before the upload: they cannot be refused here without a host read. */
int dts_heun_xhat_rows(const double* x_cur, int xb, int bcast, const void* eps, int eps_f32, const double* noise_coef,
                       double* x_hat, int nb, int chw, dts_stream s);
int dts_heun_euler_rows(const double* x_hat, const float* D, const double* t_hat, const double* t_next,
                        double* d_cur, double* x_next, int n, int chw, dts_stream s);
int dts_heun_correct_rows(const double* x_hat, const float* D2, const double* d_cur, const double* t_hat, const double* t_next,
                          double* x_next, int n, int chw, dts_stream s);

/* ---- K9b: the general ODE step of the ablation sampler, fp64 state (edm/generate.py:156-174) -------
 * dx/dt = a(t) x - b(t) D(x / s(t); sigma(t)) with a = sigma'/sigma + s'/s and b = sigma' s / sigma.  Every scalar is evaluated once per
 * step on the host and must be finite; D is the denoiser's f32 output; the arrays hold `count` elements, row for row (no broadcast).
 * Optional outputs may be NULL.  x_in = (the state just written) / s is the denoiser's next input: a true division. */
/* x_hat = ratio * x_cur + noise_coef * eps;  x_in (optional) = x_hat / s_hat.  eps is f64 (eps_f32=0) or f32; eps == NULL is legal
 * exactly when noise_coef == 0 (no noise is read). */
int dts_ode_xhat(const double* x_cur, const void* eps, int eps_f32, double ratio, double noise_coef, double s_hat,
                 double* x_hat, double* x_in, int64_t count, dts_stream s);
/* d (optional) = a * x - b * D;  x_out = base + step * d;  x_in (optional) = x_out / s_out.  x and base may be the same array; x_out is
 * neither.  step = h: the Euler step; step = alpha * h: the Heun predictor x_prime. */
int dts_ode_slope(const double* x, const float* D, double a, double b, const double* base, double step, double s_out,
                  double* d, double* x_out, double* x_in, int64_t count, dts_stream s);
/* x_next = x_hat + h * (w0 * d_cur + w1 * (a * x_prime - b * D2));  w0 = 1 - 1/(2 alpha), w1 = 1/(2 alpha).  x_next may be x_prime. */
int dts_ode_correct(const double* x_hat, const double* x_prime, const float* D2, const double* d_cur, double a, double b,
                    double h, double w0, double w1, double* x_next, int64_t count, dts_stream s);

/* ---- K10/K11: scorer pre-processing and brightness reward (edm/main.py:126; scorers.py:38-52) ----- */
/* u8 = trunc(clip(x*127.5+128, 0, 255)); x is f64 (is_f32=0) or f32 (1): arithmetic in f64 as the EDM loop's (.to(float64) first);
 * is_f32=2: f32 input AND f32 arithmetic, as the SD loop's (pipeline_stable_diffusion.py:1116).  The product is rounded, then the sum
 * (two tensor operations in the reference): never a fused multiply-add, whose single rounding changes the byte of ~2 values in a million */
int dts_quantize_u8(const void* x, int is_f32, uint8_t* out, int64_t count, dts_stream s);
/* rewards[n] = clamp(mean_hw(0.2126 R + 0.7152 G + 0.0722 B)/1, 0, 1) on u8/255 images NCHW [n][3][h][w] */
int dts_brightness(const uint8_t* img, float* rewards, int n, int hw, dts_stream s);
/* CLIP reward tail (sd/scorers.py:182-183,205-211): out[i] = <a_i/||a_i||, b_i/||b_i||>, f32; b has n rows or 1 (one prompt). */
int dts_cosine_rows(const float* a, const float* b, int b_rows, float* out, int n, int d, dts_stream s);
/* CLIP image pre-processing on the device (sd/scorers.py:166-180: `self.processor(images=...)` = transformers CLIPImageProcessor = Pillow's
 * bicubic resize of the uint8 image + rescale + normalise).  dts_resample_u8: ONE pass of Pillow's separable 8-bit resampling (Resample.c):
 * dst = clip8((2^21 + sum_k src[first + k] * coef[k]) >> 22) along a row (axis 1: [planes][h][w] -> [planes][h][out_len]) or down a column
 * (axis 0: -> [planes][out_len][w]); bounds [out_len][2] = (first, count), coefs [out_len][ksize] = Pillow's integer coefficients (built by
 * clip_preprocess.resample_tables).  dts_lut_u8_f32: out[n][c][hw] = lut[c][img]: the processor's rescale + normalise as a 256-entry table
 * per channel. */
int dts_resample_u8(const uint8_t* src, uint8_t* dst, int planes, int h, int w, int out_len, int axis, const int32_t* bounds,
                    const int32_t* coefs, int ksize, dts_stream s);
int dts_lut_u8_f32(const uint8_t* img, const float* lut, float* out, int n, int c, int hw, dts_stream s);
/* f32 NCHW = u8 / 255.0f (scorers.py:153) */
int dts_u8_to_unit_f32(const uint8_t* img, float* out, int64_t count, dts_stream s);

/* ---- K22: JPEG byte length, the compressibility reward (edm/scorers.py:176-243: len of PIL's JPEG bytes at quality q) ---- */
/* sizes[i] = length in bytes of the baseline JPEG file Pillow / libjpeg-turbo write for image i with quality q, 4:2:0 chroma and the standard
 * (non-optimised) Huffman tables -- computed without writing the file: quantised DCT coefficients, the bits of every 8x8 block, their prefix sum,
 * the entropy-coded bytes in a scratch bit buffer (for the count of 0xFF bytes, each of which the file follows with a stuffed 0x00), plus the
 * fixed header and the EOI marker.  Integer arithmetic throughout: the result is exact, not an estimate.
 * img uint8 NCHW [n][3][h][w] (what dts_quantize_u8 writes); h and w multiples of 16 (whole MCUs; other sizes return DTS_ERR_ARG: a partial MCU
 * is completed by libjpeg with dummy blocks, a rule this entry does not implement), 1 <= n <= 65535, h, w <= 16384, n * blocks <= 2^24, and
 * blocks * 1728 < 2^31 (blocks = h/16 * w/16 * 6 per image; 1728 = 64 * (16 + 11) bits, the most one block can cost): bit counts and offsets
 * are int, so an image whose scan could reach 2^31 bits is refused (DTS_ERR_ARG), not counted wrongly.  That is 207 126 MCUs, e.g. 7280 x 7280.
 * qtab: device uint16 [2][64], the luma and chroma quantisation tables for q in natural (row-major) order.
 * workspace: device scratch of at least dts_jpeg_workspace_bytes(n, h, w) bytes, 16-byte aligned; the query returns 0 for a refused shape.
 * coef_out (nullable): int16 [n][blocks][64], the quantised coefficients in zigzag order, blocks in scan order (per 16x16 MCU, row-major over
 * MCUs: Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr; blocks = h/16 * w/16 * 6) -- lets a wrong size be traced to the transform or to the entropy stage. */
int64_t dts_jpeg_workspace_bytes(int n, int h, int w);
int dts_jpeg_size(const uint8_t* img, int32_t* sizes, int n, int h, int w, const uint16_t* qtab, void* workspace, int64_t workspace_bytes,
                  int16_t* coef_out, dts_stream s);

/* ---- K12 tail: attention pool + softmax-gather (unet.py:61-69; scorers.py:162-172) ---------------- */
/* tokens[n][hw+1][c]: token 0 = mean_hw(x) + pos[:,0]; token 1+p = x[n][p] + pos[:,1+p]; pos f32 [c][hw+1] */
int dts_attnpool_tokens(const void* x, const float* pos, void* tokens, int dtype, int n, int hw, int c, dts_stream s);
/* out f32 [n][c] = src[n][token][:] */
int dts_take_token(const void* src, int dtype, float* out, int n, int t, int c, int token, dts_stream s);
/* rewards[n] = softmax(logits[n][:])[target[n]] */
int dts_softmax_gather(const float* logits, const int32_t* target, float* rewards, int n, int k, dts_stream s);

/* ---- K14: epsilon-greedy / zero-order candidate-noise builder (edm/main.py:749-800) --------------- */
/* g: host-drawn standard normals [nb][chw] f64 (uploaded); for row i (candidate n = i / b, sample = i % b):
 *   mode[n] == 0 : cand[i] = g[i]                                   (fresh Gaussian, edm/main.py:795)
 *   mode[n] == 1 : cand[i] = pivot[i % b] + (double)scale[n] * (g[i] / ||g[i]||_2)   (edm/main.py:767-788) */
int dts_candidate_noise(const double* pivot, const double* g, const int32_t* mode, const float* scale,
                        double* cand, int nb, int b, int chw, dts_stream s);
/* The same body with mode / scale per OUTPUT ROW (nb entries each): row r = n * b + sample reads mode[r], scale[r] and pivot[sample].  With
 * mode / scale constant over the b images of every candidate the output is dts_candidate_noise's bit for bit (same reduction order).
 * nb = b rebuilds b pivots, each from its own winner, in one launch. */
int dts_candidate_noise_rows(const double* pivot, const double* g, const int32_t* mode, const float* scale,
                             double* cand, int nb, int b, int chw, dts_stream s);
/* The SD backend's builder (sd/diffusers/.../pipeline_stable_diffusion.py:1371-1379), in the latents' storage type `dtype` with the
 * reference's roundings: u host-drawn normals [n][count]; mode[c] == 0: cand[c] = u[c] (fresh noise, :1375);
 * mode[c] == 1: cand[c] = pivot + ((((u[c] / ||u[c]||) * scale[3c]) * scale[3c+1]) * scale[3c+2]), scale[3c..] = (rand, lambda, sqrt(count)) as f32:
 * the reference's three tensor-by-scalar products, each rounded to `dtype` (:1377-1379).  pivot [count], scale [n][3]. */
int dts_candidate_noise_sd(const void* pivot, const void* u, const int32_t* mode, const float* scale, void* cand, int dtype, int n,
                           int64_t count, dts_stream s);
/* The same body for `searches` searches of `per` candidates each in lock-step (pipeline_stable_diffusion.py:1371-1379, once per search):
 * pivot [searches][count], u / cand [searches * per][count], mode [searches * per], scale [searches * per][3]; candidate row
 * r = s * per + n reads pivot[s], mode[r] and scale[3r..].  One block per row, the norm over that row's count values in the same reduction
 * order and with the same roundings, so searches == 1 is dts_candidate_noise_sd bit for bit. */
int dts_candidate_noise_sd_rows(const void* pivot, const void* u, const int32_t* mode, const float* scale, void* cand, int dtype,
                                int searches, int per, int64_t count, dts_stream s);

/* ---- K13: DDIM candidate step, SD backend (scheduling_ddim.py:402-463), eta*std = sigma_t ---------- */
/* For i in [0,count): x0 = (x - sqrt(1-a_t) e)/sqrt(a_t); [e' = (x - sqrt(a_t) x0)/sqrt(1-a_t) == e];
 * prev[cand] = sqrt(a_prev) x0 + sqrt(1 - a_prev - sigma_t^2) e + sigma_t z[cand]; ncand candidates share
 * one (x, e).  f32 math on dtype storage (DTS_F16 as the reference; DTS_F32 for tests). */
/* classifier-free guidance, out = uncond + guidance*(cond - uncond) (pipeline_stable_diffusion.py:1072-1074) */
int dts_cfg_combine(const void* uncond, const void* cond, float guidance, void* out, int dtype, int64_t count, dts_stream s);
int dts_ddim_candidates(const void* x, const void* e, const void* z, void* prev, void* x0_out, int dtype,
                        float alpha_t, float alpha_prev, float sigma_t, int ncand, int64_t count, dts_stream s);
/* The same step (scheduling_ddim.py:402-463) for `groups` independent (x, e) pairs with ncand candidates each, in one launch: the beams of
 * the SD beam search (pipeline_stable_diffusion.py:1077-1088) and the searches of several seeds in lock-step.  x / e / x0_out
 * [groups][count], z / prev [groups][ncand][count] (group-major, as the host draws arrive); z NULL as above, x0_out NULL to skip it.  The
 * three scalars are shared: lock-step searches sit at one timestep.  groups == 1 is dts_ddim_candidates bit for bit. */
int dts_ddim_candidates_groups(const void* x, const void* e, const void* z, void* prev, void* x0_out, int dtype,
                               float alpha_t, float alpha_prev, float sigma_t, int groups, int ncand, int64_t count, dts_stream s);

#ifdef __cplusplus
}
#endif
#endif /* DTS_H_ */
