// The CLIP vision tower between its matrix products, in the split-precision mode (dts.h DTS_F16X3): float32 twins of layer_norm_kernel
// (transformer.hip) and of the kernels of vit.hip.  Activations are float32; where the only reader of a result is a split-precision 1x1
// dts_conv2d, the result leaves as that convolution's operand image -- bit for bit what dts_split3_f16 would make of the f32 values (x3_split:
// per 32 channels hi(32) | lo * 2^11 (32), a hi below 2^-14 folded into lo, saturation at +-65504) -- and the f32 tensor is never written.
// A lane that owns 8 consecutive channels writes one 16-byte hi piece and one 16-byte lo piece of its 32-channel group's 128-byte line.
// No atomics, no LDS, no scratch; gfx950 only.
#include "dts_common.h"
#include <math.h>

namespace {

// 16-byte slot of the hi piece of 8-channel vector v (channels 8v .. 8v+7) inside an image row; its lo piece sits 4 slots further
__device__ __forceinline__ int x3_slot(int v) { return ((v >> 2) << 3) + (v & 3); }

__device__ __forceinline__ void store_x3(uint4* row, int v, const float* y) {
  float hi[8], lo[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x3_split(y[e], hi[e], lo[e]);
  uint4* o = row + x3_slot(v);
  o[0] = pack16<f16_t>(hi);
  o[4] = pack16<f16_t>(lo);
}

__device__ __forceinline__ void load8(const float* p, float* f) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

// ------------------------------------------------------------------------------------------------
// One wave's LayerNorm of one f32 row of c channels (c % 8 == 0, c <= 2048) held in registers: lane owns vectors lane + 64 i.  The order
// of layer_norm_kernel -- the mean, then the variance as the mean of (x - mean)^2 -- but the statistics and y = (x - mean) * rstd * gamma + beta
// are formed in float64 from the float32 row and y is rounded ONCE: in float32 the error of rstd (the sum's and the square root's roundings)
// scales every output of the row, and the mean of a row of large mean is good to an ulp OF THE MEAN only; here both are exact to float32
// and the result is the correctly rounded one but for double rounding.  The pass is bound by its 4 B in + 4 B out per element, not by
// the ~6 float64 operations per element (half the float32 vector rate on gfx950).
struct RowNorm {
  float f[4][8];
  double mean, rstd;
  __device__ __forceinline__ void load(const float* xr, int lane, int nvec, int c) {
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = lane + 64 * i;
      if (v < nvec) {
        load8(xr + 8 * v, f[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += (double)f[i][e];
      }
    }
    mean = wave_sum(sum) / (double)c;
  }
  __device__ __forceinline__ void stats(int lane, int nvec, int c, float eps) {
    double sq = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (lane + 64 * i < nvec) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { const double dlt = (double)f[i][e] - mean; sq = fma(dlt, dlt, sq); }
      }
    rstd = 1.0 / sqrt(wave_sum(sq) / (double)c + (double)eps);
  }
  __device__ __forceinline__ void apply(int i, int v, const float* gamma, const float* beta, float* y) const {
    float g[8], b[8];
    load8(gamma + 8 * v, g);
    load8(beta + 8 * v, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = (float)fma(((double)f[i][e] - mean) * rstd, (double)g[e], (double)b[e]);
  }
};

// LayerNorm over f32 rows [rows][c]; out_f32 (nullable): the normalised rows; out_split (nullable): their operand image [rows][2c].
// The two outputs come from the same registers, so the image is the split of the f32 rows whether or not those are written.
__global__ __launch_bounds__(256) void layer_norm_x3_kernel(const float* __restrict__ x, float* __restrict__ out_f32, uint4* __restrict__ out_split,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, long long rows, int c,
                                                             float eps) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nvec = c >> 3;
  RowNorm rn;
  rn.load(x + row * c, lane, nvec, c);
  rn.stats(lane, nvec, c, eps);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = lane + 64 * i;
    if (v < nvec) {
      float y[8];
      rn.apply(i, v, gamma, beta, y);
      if (out_f32) {
        float4* o = reinterpret_cast<float4*>(out_f32 + row * c + 8 * v);
        o[0] = make_float4(y[0], y[1], y[2], y[3]);
        o[1] = make_float4(y[4], y[5], y[6], y[7]);
      }
      if (out_split) store_x3(out_split + row * (2 * nvec), v, y);
    }
  }
}

// Pooled head: LayerNorm of token 0 of every sample of f32 tokens [n][t][c] -> f32 [n][c] (vit_head_kernel's float32 twin), one wave per sample
__global__ __launch_bounds__(256) void vit_head_f32_kernel(const float* __restrict__ tokens, float* __restrict__ out, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int n, long long tc, int c, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int nvec = c >> 3;
  RowNorm rn;
  rn.load(tokens + row * tc, lane, nvec, c);
  rn.stats(lane, nvec, c, eps);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = lane + 64 * i;
    if (v < nvec) {
      float y[8];
      rn.apply(i, v, gamma, beta, y);
      float4* o = reinterpret_cast<float4*>(out + (long long)row * c + 8 * v);
      o[0] = make_float4(y[0], y[1], y[2], y[3]);
      o[1] = make_float4(y[4], y[5], y[6], y[7]);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// act(x) of f32 rows [rows][c] as the operand image [rows][2c] (fc2's operand); gelu_kernel's two formulas, both without the 1 + erf
// cancellation and finite over the whole range: KIND 0 x / (1 + exp(-1.702 x)), KIND 1 x * (erfc(-x / sqrt 2) / 2).
template <int KIND>
__global__ __launch_bounds__(256) void gelu_x3_kernel(const float* __restrict__ x, uint4* __restrict__ out, long long nvec, int vpr) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nvec) return;
  const long long row = idx / vpr;
  const int v = (int)(idx - row * vpr);
  float a[8], y[8];
  load8(x + idx * 8, a);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (KIND == 0)
      y[e] = a[e] / (1.0f + expf(-1.702f * a[e]));
    else
      y[e] = a[e] * (0.5f * erfcf(a[e] * -0.70710678118654752f));
  }
  store_x3(out + row * (2 * vpr), v, y);
}

// ------------------------------------------------------------------------------------------------
// Patch rows as the operand image: patchify_kernel's gather (same column order, same kpad, pad columns zero) of f32 NCHW pixel_values,
// unrounded, -> [n][g*g][2*kpad].  One thread = 8 columns; the source is read with scalar 4-byte loads (a patch row of 14 floats is never
// assumed aligned), the two stores are whole 16-byte vectors.
__global__ __launch_bounds__(256) void patchify_x3_kernel(const float* __restrict__ x, uint4* __restrict__ out, long long nvec, int S, int patch,
                                                           int g, int kpad) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nvec) return;
  const int vpr = kpad >> 3;
  const long long row = idx / vpr;                 // (sample, patch)
  const int v = (int)(idx - row * vpr);
  const int gg = g * g;
  const long long n = row / gg;
  const int p = (int)(row - n * gg);
  const int gy = p / g, gx = p - gy * g;
  const int pp = patch * patch, K = 3 * pp;
  int k = v * 8;
  int c = k / pp;
  int r = k - c * pp;
  int py = r / patch, px = r - py * patch;
  float f[8];
#pragma unroll
  for (int e = 0; e < 8; ++e, ++k) {
    f[e] = 0.f;
    if (k < K) {                                   // k < K  =>  c < 3, py < patch, px < patch
      f[e] = x[((n * 3 + c) * S + (gy * patch + py)) * (long long)S + (gx * patch + px)];
      if (++px == patch) {
        px = 0;
        if (++py == patch) { py = 0; ++c; }
      }
    }
  }
  store_x3(out + row * (2 * vpr), v, f);
}

// ------------------------------------------------------------------------------------------------
// Token assembly in f32 (vit_tokens_kernel's twin): tokens[n][0] = cls + pos[0], tokens[n][1 + p] = patches[n][p] + pos[1 + p]: one f32 add.
// One thread = one 16-byte vector of 4 channels; c % 4 == 0.
__global__ __launch_bounds__(256) void vit_tokens_f32_kernel(const float* __restrict__ patches, const float* __restrict__ cls,
                                                              const float* __restrict__ pos, float* __restrict__ tokens, long long nvec, int t, int c) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nvec) return;
  const int vpr = c >> 2;
  const long long row = idx / vpr;                 // (sample, token)
  const int v = (int)(idx - row * vpr);
  const long long n = row / t;
  const int tok = (int)(row - n * t);
  const float4 a = tok == 0 ? reinterpret_cast<const float4*>(cls)[v]
                            : reinterpret_cast<const float4*>(patches + (n * (t - 1) + (tok - 1)) * c)[v];
  const float4 b = reinterpret_cast<const float4*>(pos + (long long)tok * c)[v];
  reinterpret_cast<float4*>(tokens)[idx] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

}  // namespace

extern "C" int dts_layer_norm_x3(const float* x, float* out_f32, void* out_split, int64_t rows, int c, float eps, const float* gamma,
                                 const float* beta, dts_stream s) {
  DTS_CHECK_ARG(x && gamma && beta, "dts_layer_norm_x3: null pointer");
  DTS_CHECK_ARG(out_f32 || out_split, "dts_layer_norm_x3: neither out_f32 nor out_split");
  DTS_CHECK_ARG(rows > 0 && rows < (1ll << 32), "dts_layer_norm_x3: bad row count");
  DTS_CHECK_ARG(c > 0 && c % 32 == 0 && c <= 2048, "dts_layer_norm_x3: %d channels (a multiple of 32, at most 2048)", c);
  DTS_CHECK_ARG(eps >= 0.f, "dts_layer_norm_x3: eps");
  DTS_CHECK_ARG(((uintptr_t)x | (uintptr_t)out_f32 | (uintptr_t)out_split | (uintptr_t)gamma | (uintptr_t)beta) % 16 == 0,
                "dts_layer_norm_x3: pointers must be 16-byte aligned");
  const unsigned grid = (unsigned)((rows + 3) / 4);
  hipLaunchKernelGGL(layer_norm_x3_kernel, dim3(grid), dim3(256), 0, to_stream(s), x, out_f32, (uint4*)out_split, gamma, beta, (long long)rows, c, eps);
  DTS_CHECK_LAUNCH("dts_layer_norm_x3");
  return DTS_OK;
}

extern "C" int dts_gelu_x3(const float* x, void* out_split, int64_t rows, int c, int kind, dts_stream s) {
  DTS_CHECK_ARG(x && out_split, "dts_gelu_x3: null pointer");
  DTS_CHECK_ARG(rows > 0 && c > 0 && c % 32 == 0, "dts_gelu_x3: %lld rows x %d channels (a multiple of 32)", (long long)rows, c);
  DTS_CHECK_ARG(kind == 0 || kind == 1, "dts_gelu_x3: kind %d (0 = quick-GELU, 1 = erf GELU)", kind);
  DTS_CHECK_ARG(((uintptr_t)x | (uintptr_t)out_split) % 16 == 0, "dts_gelu_x3: pointers must be 16-byte aligned");
  const long long nvec = rows * (c / 8), grid = (nvec + 255) / 256;
  DTS_CHECK_ARG(grid < (1ll << 31), "dts_gelu_x3: grid too large");
  const dim3 gd((unsigned)grid), bd(256);
  if (kind == 0) hipLaunchKernelGGL(gelu_x3_kernel<0>, gd, bd, 0, to_stream(s), x, (uint4*)out_split, nvec, c / 8);
  else hipLaunchKernelGGL(gelu_x3_kernel<1>, gd, bd, 0, to_stream(s), x, (uint4*)out_split, nvec, c / 8);
  DTS_CHECK_LAUNCH("dts_gelu_x3");
  return DTS_OK;
}

extern "C" int dts_patchify_x3(const float* x, void* out_split, int n, int size, int patch, int kpad, dts_stream s) {
  DTS_CHECK_ARG(x && out_split, "dts_patchify_x3: null pointer");
  DTS_CHECK_ARG(n > 0 && patch > 0 && size >= patch && size % patch == 0 && size < 32768,
                "dts_patchify_x3: %d images of %d pixels in patches of %d (the size a multiple of the patch)", n, size, patch);
  DTS_CHECK_ARG(kpad % 32 == 0 && kpad >= 3 * patch * patch, "dts_patchify_x3: kpad %d (a multiple of 32, at least 3*patch*patch = %d)", kpad,
                3 * patch * patch);
  DTS_CHECK_ARG((uintptr_t)out_split % 16 == 0 && (uintptr_t)x % 4 == 0, "dts_patchify_x3: out must be 16-byte aligned");
  const int g = size / patch;
  const long long nvec = (long long)n * g * g * (kpad / 8), grid = (nvec + 255) / 256;
  DTS_CHECK_ARG(grid < (1ll << 31), "dts_patchify_x3: grid too large");
  hipLaunchKernelGGL(patchify_x3_kernel, dim3((unsigned)grid), dim3(256), 0, to_stream(s), x, (uint4*)out_split, nvec, size, patch, g, kpad);
  DTS_CHECK_LAUNCH("dts_patchify_x3");
  return DTS_OK;
}

extern "C" int dts_vit_tokens_f32(const float* patches, const float* cls, const float* pos, float* tokens, int n, int t, int c, dts_stream s) {
  DTS_CHECK_ARG(patches && cls && pos && tokens, "dts_vit_tokens_f32: null pointer");
  DTS_CHECK_ARG(n > 0 && t >= 2 && c > 0 && c % 4 == 0, "dts_vit_tokens_f32: %d x %d tokens (class token + at least one patch) x %d channels (a multiple of 4)",
                n, t, c);
  DTS_CHECK_ARG(((uintptr_t)patches | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)tokens) % 16 == 0, "dts_vit_tokens_f32: pointers must be 16-byte aligned");
  const long long nvec = (long long)n * t * (c / 4), grid = (nvec + 255) / 256;
  DTS_CHECK_ARG(grid < (1ll << 31), "dts_vit_tokens_f32: grid too large");
  hipLaunchKernelGGL(vit_tokens_f32_kernel, dim3((unsigned)grid), dim3(256), 0, to_stream(s), patches, cls, pos, tokens, nvec, t, c);
  DTS_CHECK_LAUNCH("dts_vit_tokens_f32");
  return DTS_OK;
}

extern "C" int dts_vit_head_f32(const float* tokens, float* out, int n, int t, int c, float eps, const float* gamma, const float* beta, dts_stream s) {
  DTS_CHECK_ARG(tokens && out && gamma && beta, "dts_vit_head_f32: null pointer");
  DTS_CHECK_ARG(n > 0 && t > 0, "dts_vit_head_f32: bad shape");
  DTS_CHECK_ARG(c > 0 && c % 8 == 0 && c <= 2048, "dts_vit_head_f32: %d channels (a multiple of 8, at most 2048)", c);
  DTS_CHECK_ARG(eps >= 0.f, "dts_vit_head_f32: eps");
  DTS_CHECK_ARG(((uintptr_t)tokens | (uintptr_t)out | (uintptr_t)gamma | (uintptr_t)beta) % 16 == 0, "dts_vit_head_f32: pointers must be 16-byte aligned");
  const unsigned grid = (unsigned)((n + 3) / 4);
  hipLaunchKernelGGL(vit_head_f32_kernel, dim3(grid), dim3(256), 0, to_stream(s), tokens, out, gamma, beta, n, (long long)t * c, c, eps);
  DTS_CHECK_LAUNCH("dts_vit_head_f32");
  return DTS_OK;
}
