// The pieces of a CLIP vision tower (transformers models/clip/modeling_clip.py: CLIPVisionEmbeddings, CLIPMLP's activation, the pooled
// head of CLIPVisionTransformer + CLIPModel.visual_projection) that the U-Nets never needed: non-overlapping patch rows for the patch
// embedding, class token + position table, GELU as an op of its own, LayerNorm of the class token alone.  Everything else of the tower is
// dts_layer_norm, dts_conv2d (1x1), dts_attention and dts_linear.  Also the one piece CLIP's TEXT tower adds (CLIPTextEmbeddings): token
// embedding + position table.  Each kernel has ONE body, in f32 arithmetic, and the forms of row_forms.h decide what it reads and writes:
// 16-bit storage (bf16 / f16) for the 16-bit towers; for the split-precision tower (dts.h DTS_F16X3) float32 activations, and where the
// only reader of a result is a split-precision 1x1 dts_conv2d, that convolution's operand image.  No atomics, no LDS, no scratch; gfx950
// only.
#include "row_forms.h"
#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------
// Patch rows: replaces the gather of Conv2d(3, hidden, patch, stride = patch) (CLIPVisionEmbeddings.patch_embedding), whose matrix product
// then is ONE 1x1 dts_conv2d over [n][g][g][kpad].  x f32 NCHW [n][3][S][S] -> out [n][g*g][kpad], g = S / patch, column
// (c*patch + py)*patch + px = x[n][c][gy*patch + py][gx*patch + px] -- the flattening order of the conv weight -- and columns
// 3*patch*patch .. kpad-1 zero; rounded once (RNE) in the 16-bit forms, unrounded in the image.  One thread = 8 columns, which may straddle
// patch rows and channels: the source is read with scalar 4-byte loads (a patch row of 14 floats is 56 bytes, never assumed aligned), the
// stores are whole 16-byte vectors.
template <typename Out>
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ x, Out out, long long nvec, int S, int patch, int g, int kpad) {
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
  out.flat(idx, vpr, f);
}

// ------------------------------------------------------------------------------------------------
// Token assembly (CLIPVisionEmbeddings.forward: cat([class_embedding, patch_embeds], 1) + position_embedding): tokens [n][t][c] with
// tokens[n][0] = cls + pos[0], tokens[n][1 + p] = patches[n][p] + pos[1 + p]; patches [n][t-1][c] of T (16-bit or float), cls f32 [c],
// pos f32 [t][c].  The sum is formed in f32 and rounded once (for T = float: one f32 add).  One thread = one 16-byte vector of
// EPV = 8 or 4 channels; c % EPV == 0.
template <typename T>
__global__ __launch_bounds__(256) void vit_tokens_kernel(const T* __restrict__ patches, const float* __restrict__ cls,
                                                          const float* __restrict__ pos, T* __restrict__ tokens, long long nvec, int t, int c) {
  constexpr int EPV = ET<T>::EPV;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nvec) return;
  const int vpr = c >> (EPV == 8 ? 3 : 2);
  const long long row = idx / vpr;                 // (sample, token)
  const int v = (int)(idx - row * vpr);
  const long long n = row / t;
  const int tok = (int)(row - n * t);
  float a[EPV], b[EPV], y[EPV];
  if (tok == 0)
    load_f32<EPV>(cls + EPV * v, a);
  else
    unpack16<T>(reinterpret_cast<const uint4*>(patches + (n * (t - 1) + (tok - 1)) * c)[v], a);
  load_f32<EPV>(pos + (long long)tok * c + EPV * v, b);
#pragma unroll
  for (int e = 0; e < EPV; ++e) y[e] = a[e] + b[e];
  reinterpret_cast<uint4*>(tokens)[idx] = pack16<T>(y);
}

// ------------------------------------------------------------------------------------------------
// Text token assembly (CLIPTextEmbeddings.forward: token_embedding(input_ids) + position_embedding): out [n][t][c] = tok[ids[n][t]] + pos[t],
// both tables f32, the sum formed in f32 and rounded once (the float32 form: one f32 add, unrounded) -- the text counterpart of
// vit_tokens_kernel.  One thread = 8 channels, stored through the form Out (row_forms.h: Out16<T> or OutF32); c % 8 == 0.  An id outside [0, vocab) cannot be reported from here: it is clamped, for memory safety only (the caller checks the ids on
// the host, ops.text_tokens).
template <typename Out>
__global__ __launch_bounds__(256) void text_tokens_kernel(const int32_t* __restrict__ ids, const float* __restrict__ tok,
                                                           const float* __restrict__ pos, Out out, long long nvec, int t, int c, int vocab) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nvec) return;
  const int vpr = c >> 3;
  const long long row = idx / vpr;                 // (sample, token)
  const int v = (int)(idx - row * vpr);
  const int pt = (int)(row % t);
  const int id = min(max(ids[row], 0), vocab - 1);
  float a[8], b[8], y[8];
  load8(tok + (long long)id * c + 8 * v, a);
  load8(pos + (long long)pt * c + 8 * v, b);
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = a[e] + b[e];
  out.flat(idx, vpr, y);
}

// ------------------------------------------------------------------------------------------------
// GELU over a dense tensor (transformers activations.py), 16-bit to 16-bit (in place or not) or float32 rows of 8 vpr channels to their
// operand image (fc2's operand); one thread = 8 values.  Both formulas are in f32 and finite over the whole range:
//   KIND 0: QuickGELUActivation, x * sigmoid(1.702 x) = x / (1 + exp(-1.702 x)) -- hidden_act of every OpenAI CLIP checkpoint.  The
//           quotient form stays finite over the whole storage range: for very negative x the exponential overflows to +inf and
//           x / inf = -0 (the form x * e / (1 + e), e = exp(1.702 x), would be inf / inf at the other end).
//   KIND 1: the erf GELU x * Phi(x), Phi(x) = erfc(-x / sqrt 2) / 2: geglu_kernel's form (transformer.hip), without the cancellation of
//           1 + erf for negative x; erfc underflows to 0 and x * 0 = -0.
template <typename In, typename Out, int KIND>
__global__ __launch_bounds__(256) void gelu_kernel(const In* x, Out out, long long nvec, int vpr) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nvec) return;
  float a[8], y[8];
  load8(x + idx * 8, a);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (KIND == 0)
      y[e] = a[e] / (1.0f + expf(-1.702f * a[e]));
    else
      y[e] = a[e] * (0.5f * erfcf(a[e] * -0.70710678118654752f));
  }
  out.flat(idx, vpr, y);
}

// ---- the launcher halves: what an entry point shares with its other forms; `name` is the entry point's, for its messages ----------------

// kmul: the multiple kpad must be (8: a whole vector; 32: a whole group of the operand image)
template <typename Out>
int patchify(const char* name, const float* x, Out out, int n, int size, int patch, int kpad, int kmul, dts_stream s) {
  DTS_CHECK_ARG(n > 0 && patch > 0 && size >= patch && size % patch == 0 && size < 32768,
                "%s: %d images of %d pixels in patches of %d (the size a multiple of the patch)", name, n, size, patch);
  DTS_CHECK_ARG(kpad % kmul == 0 && kpad >= 3 * patch * patch, "%s: kpad %d (a multiple of %d, at least 3*patch*patch = %d)", name, kpad, kmul,
                3 * patch * patch);
  DTS_CHECK_ARG(out.addr() % 16 == 0 && (uintptr_t)x % 4 == 0, "%s: out must be 16-byte aligned", name);
  const int g = size / patch;
  const long long nvec = (long long)n * g * g * (kpad / 8), grid = (nvec + 255) / 256;
  DTS_CHECK_ARG(grid < (1ll << 31), "%s: grid too large", name);
  hipLaunchKernelGGL(patchify_kernel<Out>, dim3((unsigned)grid), dim3(256), 0, to_stream(s), x, out, nvec, size, patch, g, kpad);
  DTS_CHECK_LAUNCH(name);
  return DTS_OK;
}

template <typename T>
int vit_tokens(const char* name, const T* patches, const float* cls, const float* pos, T* tokens, int n, int t, int c, dts_stream s) {
  constexpr int EPV = ET<T>::EPV;
  DTS_CHECK_ARG(n > 0 && t >= 2 && c > 0 && c % EPV == 0, "%s: %d x %d tokens (class token + at least one patch) x %d channels (a multiple of %d)",
                name, n, t, c, EPV);
  DTS_CHECK_ARG(((uintptr_t)patches | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)tokens) % 16 == 0, "%s: pointers must be 16-byte aligned", name);
  const long long nvec = (long long)n * t * (c / EPV), grid = (nvec + 255) / 256;
  DTS_CHECK_ARG(grid < (1ll << 31), "%s: grid too large", name);
  hipLaunchKernelGGL(vit_tokens_kernel<T>, dim3((unsigned)grid), dim3(256), 0, to_stream(s), patches, cls, pos, tokens, nvec, t, c);
  DTS_CHECK_LAUNCH(name);
  return DTS_OK;
}

template <typename Out>
int text_tokens(const char* name, const int32_t* ids, const float* tok, const float* pos, Out out, int n, int t, int c, int vocab, dts_stream s) {
  DTS_CHECK_ARG(n > 0 && t > 0 && vocab > 0 && c > 0 && c % 8 == 0, "%s: %d x %d tokens x %d channels (a multiple of 8), vocabulary %d", name, n, t, c, vocab);
  DTS_CHECK_ARG(((uintptr_t)tok | (uintptr_t)pos | out.addr()) % 16 == 0 && (uintptr_t)ids % 4 == 0, "%s: pointers must be 16-byte aligned", name);
  const long long nvec = (long long)n * t * (c / 8), grid = (nvec + 255) / 256;
  DTS_CHECK_ARG(grid < (1ll << 31), "%s: grid too large", name);
  hipLaunchKernelGGL(text_tokens_kernel<Out>, dim3((unsigned)grid), dim3(256), 0, to_stream(s), ids, tok, pos, out, nvec, t, c, vocab);
  DTS_CHECK_LAUNCH(name);
  return DTS_OK;
}

// nvec vectors of 8 values, vpr of them per row (read by the image form alone)
template <typename In, typename Out>
int gelu(const char* name, const In* x, Out out, long long nvec, int vpr, int kind, dts_stream s) {
  DTS_CHECK_ARG(kind == 0 || kind == 1, "%s: kind %d (0 = quick-GELU, 1 = erf GELU)", name, kind);
  DTS_CHECK_ARG(((uintptr_t)x | out.addr()) % 16 == 0, "%s: pointers must be 16-byte aligned", name);
  const long long grid = (nvec + 255) / 256;
  DTS_CHECK_ARG(grid < (1ll << 31), "%s: grid too large", name);
  const dim3 gd((unsigned)grid), bd(256);
  if (kind == 0) hipLaunchKernelGGL((gelu_kernel<In, Out, 0>), gd, bd, 0, to_stream(s), x, out, nvec, vpr);
  else hipLaunchKernelGGL((gelu_kernel<In, Out, 1>), gd, bd, 0, to_stream(s), x, out, nvec, vpr);
  DTS_CHECK_LAUNCH(name);
  return DTS_OK;
}

}  // namespace

extern "C" int dts_patchify(const float* x, void* out, int dtype, int n, int size, int patch, int kpad, dts_stream s) {
  DTS_CHECK_ARG(x && out, "dts_patchify: null pointer");
  DTS_DISPATCH_16BIT("dts_patchify", dtype, return patchify("dts_patchify", x, Out16<T>{(T*)out}, n, size, patch, kpad, 8, s));
}

extern "C" int dts_patchify_x3(const float* x, void* out_split, int n, int size, int patch, int kpad, dts_stream s) {
  DTS_CHECK_ARG(x && out_split, "dts_patchify_x3: null pointer");
  return patchify("dts_patchify_x3", x, OutX3{(uint4*)out_split}, n, size, patch, kpad, 32, s);
}

extern "C" int dts_vit_tokens(const void* patches, const float* cls, const float* pos, void* tokens, int dtype, int n, int t, int c,
                              dts_stream s) {
  DTS_CHECK_ARG(patches && cls && pos && tokens, "dts_vit_tokens: null pointer");
  DTS_DISPATCH_16BIT("dts_vit_tokens", dtype, return vit_tokens("dts_vit_tokens", (const T*)patches, cls, pos, (T*)tokens, n, t, c, s));
}

extern "C" int dts_vit_tokens_f32(const float* patches, const float* cls, const float* pos, float* tokens, int n, int t, int c, dts_stream s) {
  DTS_CHECK_ARG(patches && cls && pos && tokens, "dts_vit_tokens_f32: null pointer");
  return vit_tokens("dts_vit_tokens_f32", patches, cls, pos, tokens, n, t, c, s);
}

extern "C" int dts_text_tokens(const int32_t* ids, const float* tok, const float* pos, void* out, int dtype, int n, int t, int c, int vocab,
                               dts_stream s) {
  DTS_CHECK_ARG(ids && tok && pos && out, "dts_text_tokens: null pointer");
  DTS_DISPATCH_16BIT("dts_text_tokens", dtype, return text_tokens("dts_text_tokens", ids, tok, pos, Out16<T>{(T*)out}, n, t, c, vocab, s));
}

extern "C" int dts_text_tokens_f32(const int32_t* ids, const float* tok, const float* pos, float* out, int n, int t, int c, int vocab, dts_stream s) {
  DTS_CHECK_ARG(ids && tok && pos && out, "dts_text_tokens_f32: null pointer");
  return text_tokens("dts_text_tokens_f32", ids, tok, pos, OutF32{out}, n, t, c, vocab, s);
}

extern "C" int dts_gelu(const void* x, void* out, int dtype, int64_t count, int kind, dts_stream s) {
  DTS_CHECK_ARG(x && out, "dts_gelu: null pointer");
  DTS_DISPATCH_16BIT("dts_gelu", dtype, {
    DTS_CHECK_ARG(count > 0 && count % 8 == 0, "dts_gelu: count %lld (a positive multiple of 8)", (long long)count);
    return gelu("dts_gelu", (const T*)x, Out16<T>{(T*)out}, count / 8, 0, kind, s);
  });
}

extern "C" int dts_gelu_x3(const float* x, void* out_split, int64_t rows, int c, int kind, dts_stream s) {
  DTS_CHECK_ARG(x && out_split, "dts_gelu_x3: null pointer");
  DTS_CHECK_ARG(rows > 0 && c > 0 && c % 32 == 0, "dts_gelu_x3: %lld rows x %d channels (a multiple of 32)", (long long)rows, c);
  return gelu("dts_gelu_x3", x, OutX3{(uint4*)out_split}, rows * (c / 8), c / 8, kind, s);
}

// Pooled head, first half (CLIPVisionTransformer.forward: post_layernorm(last_hidden_state[:, 0, :])): LayerNorm of token 0 of every
// sample only -- the other t - 1 tokens are never normalised, the row stride is t * c -- written as an f32 row [n][c], the operand of
// dts_linear with visual_projection.  dts_layer_norm's arithmetic for 16-bit tokens, dts_layer_norm_x3's for float32 tokens.
extern "C" int dts_vit_head(const void* tokens, float* out, int dtype, int n, int t, int c, float eps, const float* gamma, const float* beta,
                            dts_stream s) {
  DTS_CHECK_ARG(tokens && out && gamma && beta, "dts_vit_head: null pointer");
  DTS_DISPATCH_16BIT("dts_vit_head", dtype, {
    DTS_CHECK_ARG(n > 0 && t > 0, "dts_vit_head: bad shape");
    return row_norm<float>("dts_vit_head", (const T*)tokens, (long long)t * c, OutF32{out}, gamma, beta, n, c, 8, eps, s);
  });
}

extern "C" int dts_vit_head_f32(const float* tokens, float* out, int n, int t, int c, float eps, const float* gamma, const float* beta, dts_stream s) {
  DTS_CHECK_ARG(tokens && out && gamma && beta, "dts_vit_head_f32: null pointer");
  DTS_CHECK_ARG(n > 0 && t > 0, "dts_vit_head_f32: bad shape");
  return row_norm<double>("dts_vit_head_f32", tokens, (long long)t * c, OutF32{out}, gamma, beta, n, c, 8, eps, s);
}
