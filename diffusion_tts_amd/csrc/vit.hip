// The pieces of a CLIP vision tower (transformers models/clip/modeling_clip.py: CLIPVisionEmbeddings, CLIPMLP's activation, the pooled
// head of CLIPVisionTransformer + CLIPModel.visual_projection) that the U-Nets never needed: non-overlapping patch rows for the patch
// embedding, class token + position table, GELU as an op of its own, LayerNorm of the class token alone.  Everything else of the tower is
// dts_layer_norm, dts_conv2d (1x1), dts_attention and dts_linear.  Also the one piece CLIP's TEXT tower adds (CLIPTextEmbeddings): token
// embedding + position table.  16-bit storage (bf16 / f16), f32 arithmetic, gfx950 only.
#include "dts_common.h"
#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------
// Patch rows: replaces the gather of Conv2d(3, hidden, patch, stride = patch) (CLIPVisionEmbeddings.patch_embedding), whose matrix product
// then is ONE 1x1 dts_conv2d over [n][g][g][kpad].  x f32 NCHW [n][3][S][S] -> out [n][g*g][kpad], g = S / patch, column
// (c*patch + py)*patch + px = x[n][c][gy*patch + py][gx*patch + px] rounded once (RNE) -- the flattening order of the conv weight -- and
// columns 3*patch*patch .. kpad-1 zero.  One thread = one 16-byte vector of 8 columns, which may straddle patch rows and channels: the
// source is read with scalar 4-byte loads (a patch row of 14 floats is 56 bytes, never assumed aligned), the store is a whole vector.
template <typename T>
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ x, T* __restrict__ out, long long nvec, int S, int patch,
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
  reinterpret_cast<uint4*>(out)[idx] = pack16<T>(f);
}

// ------------------------------------------------------------------------------------------------
// Token assembly (CLIPVisionEmbeddings.forward: cat([class_embedding, patch_embeds], 1) + position_embedding): tokens [n][t][c] with
// tokens[n][0] = cls + pos[0], tokens[n][1 + p] = patches[n][p] + pos[1 + p]; patches [n][t-1][c] 16-bit, cls f32 [c], pos f32 [t][c].
// The sum is formed in f32 and rounded once.  One thread = one 16-byte vector; c % 8 == 0.
template <typename T>
__global__ __launch_bounds__(256) void vit_tokens_kernel(const T* __restrict__ patches, const float* __restrict__ cls,
                                                          const float* __restrict__ pos, T* __restrict__ tokens, long long nvec, int t, int c) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nvec) return;
  const int vpr = c >> 3;
  const long long row = idx / vpr;                 // (sample, token)
  const int v = (int)(idx - row * vpr);
  const long long n = row / t;
  const int tok = (int)(row - n * t);
  float a[8];
  if (tok == 0) {
    const float4 c0 = reinterpret_cast<const float4*>(cls)[2 * v], c1 = reinterpret_cast<const float4*>(cls)[2 * v + 1];
    a[0] = c0.x; a[1] = c0.y; a[2] = c0.z; a[3] = c0.w; a[4] = c1.x; a[5] = c1.y; a[6] = c1.z; a[7] = c1.w;
  } else {
    unpack16<T>(reinterpret_cast<const uint4*>(patches + (n * (t - 1) + (tok - 1)) * c)[v], a);
  }
  const float4* pr = reinterpret_cast<const float4*>(pos + (long long)tok * c);
  const float4 p0 = pr[2 * v], p1 = pr[2 * v + 1];
  const float b[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
  float y[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = a[e] + b[e];
  reinterpret_cast<uint4*>(tokens)[idx] = pack16<T>(y);
}

// ------------------------------------------------------------------------------------------------
// Text token assembly (CLIPTextEmbeddings.forward: token_embedding(input_ids) + position_embedding): out [n][t][c] = tok[ids[n][t]] + pos[t],
// both tables f32, the sum formed in f32 and rounded once -- the text counterpart of vit_tokens_kernel.  One thread = one 16-byte vector;
// c % 8 == 0.  An id outside [0, vocab) cannot be reported from here: it is clamped, for memory safety only (the caller checks the ids on
// the host, ops.text_tokens).
template <typename T>
__global__ __launch_bounds__(256) void text_tokens_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok,
                                                           const float* __restrict__ pos, T* __restrict__ out, long long nvec, int t, int c, int vocab) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nvec) return;
  const int vpr = c >> 3;
  const long long row = idx / vpr;                 // (sample, token)
  const int v = (int)(idx - row * vpr);
  const int pt = (int)(row % t);
  const int id = min(max(ids[row], 0), vocab - 1);
  const float4* tr = reinterpret_cast<const float4*>(tok + (long long)id * c);
  const float4* pr = reinterpret_cast<const float4*>(pos + (long long)pt * c);
  const float4 a0 = tr[2 * v], a1 = tr[2 * v + 1], p0 = pr[2 * v], p1 = pr[2 * v + 1];
  const float y[8] = {a0.x + p0.x, a0.y + p0.y, a0.z + p0.z, a0.w + p0.w, a1.x + p1.x, a1.y + p1.y, a1.z + p1.z, a1.w + p1.w};
  reinterpret_cast<uint4*>(out)[idx] = pack16<T>(y);
}

// ------------------------------------------------------------------------------------------------
// GELU over a dense 16-bit tensor (transformers activations.py), in place or not; one thread = one vector of 8.
//   KIND 0: QuickGELUActivation, x * sigmoid(1.702 x) = x / (1 + exp(-1.702 x)) -- hidden_act of every OpenAI CLIP checkpoint.  The
//           quotient form stays finite over the whole storage range: for very negative x the exponential overflows to +inf and
//           x / inf = -0 (the form x * e / (1 + e), e = exp(1.702 x), would be inf / inf at the other end).
//   KIND 1: the erf GELU x * Phi(x), Phi(x) = erfc(-x / sqrt 2) / 2: geglu_kernel's form (transformer.hip), without the cancellation of
//           1 + erf for negative x; erfc underflows to 0 and x * 0 = -0.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void gelu_kernel(const T* x, T* out, long long nvec) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nvec) return;
  float a[8], y[8];
  unpack16<T>(reinterpret_cast<const uint4*>(x)[idx], a);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (KIND == 0)
      y[e] = a[e] / (1.0f + expf(-1.702f * a[e]));
    else
      y[e] = a[e] * (0.5f * erfcf(a[e] * -0.70710678118654752f));
  }
  reinterpret_cast<uint4*>(out)[idx] = pack16<T>(y);
}

// ------------------------------------------------------------------------------------------------
// Pooled head, first half (CLIPVisionTransformer.forward: post_layernorm(last_hidden_state[:, 0, :])): LayerNorm of token 0 of every
// sample only -- the other t - 1 tokens are never normalised -- written as an f32 row [n][c], the operand of dts_linear with
// visual_projection.  layer_norm_kernel's arithmetic (transformer.hip): one wave per sample, the row in registers (c <= 2048), mean first,
// then the mean of (x - mean)^2.
template <typename T>
__global__ __launch_bounds__(256) void vit_head_kernel(const T* __restrict__ tokens, float* __restrict__ out, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int n, long long tc, int c, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int nvec = c >> 3;
  const uint4* xr = reinterpret_cast<const uint4*>(tokens + row * tc);
  float f[4][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = lane + 64 * i;
    if (v < nvec) {
      unpack16<T>(xr[v], f[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += f[i][e];
    }
  }
  const float mean = wave_sum(sum) / (float)c;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (lane + 64 * i < nvec) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float dlt = f[i][e] - mean; sq += dlt * dlt; }
    }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)c + eps);
  float4* orow = reinterpret_cast<float4*>(out + (long long)row * c);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = lane + 64 * i;
    if (v < nvec) {
      const float4 g0 = reinterpret_cast<const float4*>(gamma)[2 * v], g1 = reinterpret_cast<const float4*>(gamma)[2 * v + 1];
      const float4 b0 = reinterpret_cast<const float4*>(beta)[2 * v], b1 = reinterpret_cast<const float4*>(beta)[2 * v + 1];
      orow[2 * v] = make_float4(fmaf((f[i][0] - mean) * rstd, g0.x, b0.x), fmaf((f[i][1] - mean) * rstd, g0.y, b0.y),
                                fmaf((f[i][2] - mean) * rstd, g0.z, b0.z), fmaf((f[i][3] - mean) * rstd, g0.w, b0.w));
      orow[2 * v + 1] = make_float4(fmaf((f[i][4] - mean) * rstd, g1.x, b1.x), fmaf((f[i][5] - mean) * rstd, g1.y, b1.y),
                                    fmaf((f[i][6] - mean) * rstd, g1.z, b1.z), fmaf((f[i][7] - mean) * rstd, g1.w, b1.w));
    }
  }
}

}  // namespace

#define DTS_VIT_16BIT(name, dtype) DTS_CHECK_ARG(dtype == DTS_BF16 || dtype == DTS_F16, name ": dtype %d (16-bit types only)", dtype)

extern "C" int dts_patchify(const float* x, void* out, int dtype, int n, int size, int patch, int kpad, dts_stream s) {
  DTS_CHECK_ARG(x && out, "dts_patchify: null pointer");
  DTS_VIT_16BIT("dts_patchify", dtype);
  DTS_CHECK_ARG(n > 0 && patch > 0 && size >= patch && size % patch == 0 && size < 32768,
                "dts_patchify: %d images of %d pixels in patches of %d (the size a multiple of the patch)", n, size, patch);
  DTS_CHECK_ARG(kpad % 8 == 0 && kpad >= 3 * patch * patch, "dts_patchify: kpad %d (a multiple of 8, at least 3*patch*patch = %d)", kpad,
                3 * patch * patch);
  DTS_CHECK_ARG((uintptr_t)out % 16 == 0 && (uintptr_t)x % 4 == 0, "dts_patchify: out must be 16-byte aligned");
  const int g = size / patch;
  const long long nvec = (long long)n * g * g * (kpad / 8), grid = (nvec + 255) / 256;
  DTS_CHECK_ARG(grid < (1ll << 31), "dts_patchify: grid too large");
  if (dtype == DTS_BF16)
    hipLaunchKernelGGL(patchify_kernel<bf16_t>, dim3((unsigned)grid), dim3(256), 0, to_stream(s), x, (bf16_t*)out, nvec, size, patch, g, kpad);
  else
    hipLaunchKernelGGL(patchify_kernel<f16_t>, dim3((unsigned)grid), dim3(256), 0, to_stream(s), x, (f16_t*)out, nvec, size, patch, g, kpad);
  DTS_CHECK_LAUNCH("dts_patchify");
  return DTS_OK;
}

extern "C" int dts_vit_tokens(const void* patches, const float* cls, const float* pos, void* tokens, int dtype, int n, int t, int c,
                              dts_stream s) {
  DTS_CHECK_ARG(patches && cls && pos && tokens, "dts_vit_tokens: null pointer");
  DTS_VIT_16BIT("dts_vit_tokens", dtype);
  DTS_CHECK_ARG(n > 0 && t >= 2 && c > 0 && c % 8 == 0, "dts_vit_tokens: %d x %d tokens (class token + at least one patch) x %d channels (a multiple of 8)",
                n, t, c);
  DTS_CHECK_ARG(((uintptr_t)patches | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)tokens) % 16 == 0, "dts_vit_tokens: pointers must be 16-byte aligned");
  const long long nvec = (long long)n * t * (c / 8), grid = (nvec + 255) / 256;
  DTS_CHECK_ARG(grid < (1ll << 31), "dts_vit_tokens: grid too large");
  if (dtype == DTS_BF16)
    hipLaunchKernelGGL(vit_tokens_kernel<bf16_t>, dim3((unsigned)grid), dim3(256), 0, to_stream(s), (const bf16_t*)patches, cls, pos, (bf16_t*)tokens, nvec, t, c);
  else
    hipLaunchKernelGGL(vit_tokens_kernel<f16_t>, dim3((unsigned)grid), dim3(256), 0, to_stream(s), (const f16_t*)patches, cls, pos, (f16_t*)tokens, nvec, t, c);
  DTS_CHECK_LAUNCH("dts_vit_tokens");
  return DTS_OK;
}

extern "C" int dts_text_tokens(const int32_t* ids, const float* tok, const float* pos, void* out, int dtype, int n, int t, int c, int vocab,
                               dts_stream s) {
  DTS_CHECK_ARG(ids && tok && pos && out, "dts_text_tokens: null pointer");
  DTS_VIT_16BIT("dts_text_tokens", dtype);
  DTS_CHECK_ARG(n > 0 && t > 0 && vocab > 0 && c > 0 && c % 8 == 0, "dts_text_tokens: %d x %d tokens x %d channels (a multiple of 8), vocabulary %d",
                n, t, c, vocab);
  DTS_CHECK_ARG(((uintptr_t)tok | (uintptr_t)pos | (uintptr_t)out) % 16 == 0 && (uintptr_t)ids % 4 == 0, "dts_text_tokens: pointers must be 16-byte aligned");
  const long long nvec = (long long)n * t * (c / 8), grid = (nvec + 255) / 256;
  DTS_CHECK_ARG(grid < (1ll << 31), "dts_text_tokens: grid too large");
  if (dtype == DTS_BF16)
    hipLaunchKernelGGL(text_tokens_kernel<bf16_t>, dim3((unsigned)grid), dim3(256), 0, to_stream(s), ids, tok, pos, (bf16_t*)out, nvec, t, c, vocab);
  else
    hipLaunchKernelGGL(text_tokens_kernel<f16_t>, dim3((unsigned)grid), dim3(256), 0, to_stream(s), ids, tok, pos, (f16_t*)out, nvec, t, c, vocab);
  DTS_CHECK_LAUNCH("dts_text_tokens");
  return DTS_OK;
}

extern "C" int dts_gelu(const void* x, void* out, int dtype, int64_t count, int kind, dts_stream s) {
  DTS_CHECK_ARG(x && out, "dts_gelu: null pointer");
  DTS_VIT_16BIT("dts_gelu", dtype);
  DTS_CHECK_ARG(count > 0 && count % 8 == 0, "dts_gelu: count %lld (a positive multiple of 8)", (long long)count);
  DTS_CHECK_ARG(kind == 0 || kind == 1, "dts_gelu: kind %d (0 = quick-GELU, 1 = erf GELU)", kind);
  DTS_CHECK_ARG(((uintptr_t)x | (uintptr_t)out) % 16 == 0, "dts_gelu: pointers must be 16-byte aligned");
  const long long nvec = count / 8, grid = (nvec + 255) / 256;
  DTS_CHECK_ARG(grid < (1ll << 31), "dts_gelu: grid too large");
  const dim3 gd((unsigned)grid), bd(256);
  hipStream_t st = to_stream(s);
  if (dtype == DTS_BF16) {
    if (kind == 0) hipLaunchKernelGGL((gelu_kernel<bf16_t, 0>), gd, bd, 0, st, (const bf16_t*)x, (bf16_t*)out, nvec);
    else hipLaunchKernelGGL((gelu_kernel<bf16_t, 1>), gd, bd, 0, st, (const bf16_t*)x, (bf16_t*)out, nvec);
  } else {
    if (kind == 0) hipLaunchKernelGGL((gelu_kernel<f16_t, 0>), gd, bd, 0, st, (const f16_t*)x, (f16_t*)out, nvec);
    else hipLaunchKernelGGL((gelu_kernel<f16_t, 1>), gd, bd, 0, st, (const f16_t*)x, (f16_t*)out, nvec);
  }
  DTS_CHECK_LAUNCH("dts_gelu");
  return DTS_OK;
}

extern "C" int dts_vit_head(const void* tokens, float* out, int dtype, int n, int t, int c, float eps, const float* gamma, const float* beta,
                            dts_stream s) {
  DTS_CHECK_ARG(tokens && out && gamma && beta, "dts_vit_head: null pointer");
  DTS_VIT_16BIT("dts_vit_head", dtype);
  DTS_CHECK_ARG(n > 0 && t > 0, "dts_vit_head: bad shape");
  DTS_CHECK_ARG(c > 0 && c % 8 == 0 && c <= 2048, "dts_vit_head: %d channels (a multiple of 8, at most 2048)", c);
  DTS_CHECK_ARG(eps >= 0.f, "dts_vit_head: eps");
  DTS_CHECK_ARG(((uintptr_t)tokens | (uintptr_t)out | (uintptr_t)gamma | (uintptr_t)beta) % 16 == 0, "dts_vit_head: pointers must be 16-byte aligned");
  const unsigned grid = (unsigned)((n + 3) / 4);
  const long long tc = (long long)t * c;
  if (dtype == DTS_BF16)
    hipLaunchKernelGGL(vit_head_kernel<bf16_t>, dim3(grid), dim3(256), 0, to_stream(s), (const bf16_t*)tokens, out, gamma, beta, n, tc, c, eps);
  else
    hipLaunchKernelGGL(vit_head_kernel<f16_t>, dim3(grid), dim3(256), 0, to_stream(s), (const f16_t*)tokens, out, gamma, beta, n, tc, c, eps);
  DTS_CHECK_LAUNCH("dts_vit_head");
  return DTS_OK;
}
