// The forms in which 8 consecutive channels of a row enter and leave the element-wise and row kernels of vit.hip and transformer.hip,
// and the wave-per-row LayerNorm they share.  A kernel body is written once over `float[8]`; the form decides what a load reads and what
// a store writes:
//   16-bit T      one 16-byte vector of 8 values, rounded once (RNE)                                         load8, Out16<T>
//   float32       two 16-byte vectors                                                                         load8, OutF32
//   operand image the split-precision convolution's operand (dts.h DTS_F16X3), bit for bit what dts_split3_f16 would make of the f32
//                 values (x3_split: per 32 channels hi(32) | lo * 2^11 (32)); the f32 tensor is never written                OutX3
//   both          float32 rows and / or their image from the same registers (either may be null)              OutF32X3
// A store form owns its address computation: at(row, v, vpr, y) writes vector v of a row of vpr vectors, flat(idx, vpr, y) vector
// idx = row * vpr + v of a dense tensor -- only the image form divides by vpr there, the others never see the division.
#pragma once
#include "dts_common.h"

template <int N> __device__ __forceinline__ void load_f32(const float* p, float* f) {   // N = 4 or 8 floats from a 16-byte aligned f32 table
#pragma unroll
  for (int q = 0; q < N / 4; ++q) {
    const float4 a = reinterpret_cast<const float4*>(p)[q];
    f[4 * q] = a.x; f[4 * q + 1] = a.y; f[4 * q + 2] = a.z; f[4 * q + 3] = a.w;
  }
}
__device__ __forceinline__ void load8(const float* p, float* f) { load_f32<8>(p, f); }
template <typename T> __device__ __forceinline__ void load8(const T* p, float* f) { unpack16<T>(*reinterpret_cast<const uint4*>(p), f); }

template <typename T> struct Out16 {
  T* p;
  uintptr_t addr() const { return (uintptr_t)p; }
  __device__ __forceinline__ void flat(long long idx, int, const float* y) const { reinterpret_cast<uint4*>(p)[idx] = pack16<T>(y); }
  __device__ __forceinline__ void at(long long row, int v, int vpr, const float* y) const { Out16{p + row * (8 * vpr)}.flat(v, vpr, y); }
};

struct OutF32 {
  float* p;
  uintptr_t addr() const { return (uintptr_t)p; }
  __device__ __forceinline__ void flat(long long idx, int, const float* y) const {
    float4* o = reinterpret_cast<float4*>(p + idx * 8);
    o[0] = make_float4(y[0], y[1], y[2], y[3]);
    o[1] = make_float4(y[4], y[5], y[6], y[7]);
  }
  __device__ __forceinline__ void at(long long row, int v, int vpr, const float* y) const { OutF32{p + row * (8 * vpr)}.flat(v, vpr, y); }
};

// 16-byte slot of the hi piece of 8-channel vector v (channels 8v .. 8v+7) inside an image row; its lo piece sits 4 slots further: a lane
// that owns 8 consecutive channels writes one 16-byte hi piece and one 16-byte lo piece of its 32-channel group's 128-byte line
__device__ __forceinline__ int x3_slot(int v) { return ((v >> 2) << 3) + (v & 3); }

__device__ __forceinline__ void store_x3(uint4* row, int v, const float* y) {
  float hi[8], lo[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x3_split(y[e], hi[e], lo[e]);
  uint4* o = row + x3_slot(v);
  o[0] = pack16<f16_t>(hi);
  o[4] = pack16<f16_t>(lo);
}

struct OutX3 {
  uint4* p;
  uintptr_t addr() const { return (uintptr_t)p; }
  __device__ __forceinline__ void at(long long row, int v, int vpr, const float* y) const { store_x3(p + row * (2 * vpr), v, y); }
  __device__ __forceinline__ void flat(long long idx, int vpr, const float* y) const {
    const long long row = idx / vpr;
    at(row, (int)(idx - row * vpr), vpr, y);
  }
};

struct OutF32X3 {
  float* f32;
  uint4* split;
  uintptr_t addr() const { return (uintptr_t)f32 | (uintptr_t)split; }
  __device__ __forceinline__ void at(long long row, int v, int vpr, const float* y) const {
    if (f32) OutF32{f32}.at(row, v, vpr, y);
    if (split) OutX3{split}.at(row, v, vpr, y);
  }
};

// ------------------------------------------------------------------------------------------------
// The two steps of RowNorm in which the accumulator types differ in more than width.  The float sum of squares adds the ROUNDED square
// (the 16-bit kernels have always been compiled to a multiply and an add, and their outputs are pinned bit for bit), the double one is
// fused.
__device__ __forceinline__ float rsqrt_of(float x) { return 1.0f / sqrtf(x); }
__device__ __forceinline__ double rsqrt_of(double x) { return 1.0 / sqrt(x); }
__device__ __forceinline__ float add_square(float sq, float d) {
#pragma clang fp contract(off)
  return sq + d * d;
}
__device__ __forceinline__ double add_square(double sq, double d) { return fma(d, d, sq); }

// One wave's LayerNorm of one row of c channels (c % 8 == 0, c <= 2048) held in registers: lane owns vectors lane + 64 i, so the variance
// is the mean of (x - mean)^2 with the mean already known -- no E[x^2] - E[x]^2 cancellation for rows with a large mean.  A is the type
// the statistics and y = (x - mean) * rstd * gamma + beta are formed in; y is rounded to float ONCE.
//   A = float   the 16-bit rows: their storage rounding (2^-9 / 2^-12) dwarfs float32's.
//   A = double  the float32 rows: in float32 the error of rstd (the sum's and the square root's roundings) scales every output of the row,
//               and the mean of a row of large mean is good to an ulp OF THE MEAN only; here both are exact to float32 and the result is
//               the correctly rounded one but for double rounding.  The pass is bound by its 4 B in + 4 B out per element, not by the ~6
//               float64 operations per element (half the float32 vector rate on gfx950).
template <typename A> struct RowNorm {
  float f[4][8];
  A mean, rstd;
  template <typename In> __device__ __forceinline__ void load(const In* xr, int lane, int nvec, int c) {
    A sum = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = lane + 64 * i;
      if (v < nvec) {
        load8(xr + 8 * v, f[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += (A)f[i][e];
      }
    }
    mean = wave_sum(sum) / (A)c;
  }
  __device__ __forceinline__ void stats(int lane, int nvec, int c, float eps) {
    A sq = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (lane + 64 * i < nvec) {
#pragma unroll
        for (int e = 0; e < 8; ++e) sq = add_square(sq, (A)f[i][e] - mean);
      }
    rstd = rsqrt_of(wave_sum(sq) / (A)c + (A)eps);
  }
  __device__ __forceinline__ void apply(int i, int v, const float* gamma, const float* beta, float* y) const {
    float g[8], b[8];
    load8(gamma + 8 * v, g);
    load8(beta + 8 * v, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = (float)fma(((A)f[i][e] - mean) * rstd, (A)g[e], (A)b[e]);
  }
};

namespace {

// LayerNorm of rows [rows] of c channels, row r starting at x + r * stride, in the accumulator type A, written through the form Out as
// rows of c channels; 4 waves = 4 rows per block.
template <typename In, typename A, typename Out>
__global__ __launch_bounds__(256) void row_norm_kernel(const In* __restrict__ x, long long stride, Out out, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, long long rows, int c, float eps) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nvec = c >> 3;
  RowNorm<A> rn;
  rn.load(x + row * stride, lane, nvec, c);
  rn.stats(lane, nvec, c, eps);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = lane + 64 * i;
    if (v < nvec) {
      float y[8];
      rn.apply(i, v, gamma, beta, y);
      out.at(row, v, nvec, y);
    }
  }
}

// The checks every LayerNorm entry point makes after those on its own shape, and the launch; `name` is the entry point's, for its
// messages, cmul the multiple its channel count must be (8: a whole vector; 32: a whole group of the operand image).
template <typename A, typename In, typename Out>
int row_norm(const char* name, const In* x, long long stride, Out out, const float* gamma, const float* beta, long long rows, int c, int cmul,
             float eps, dts_stream s) {
  DTS_CHECK_ARG(c > 0 && c % cmul == 0 && c <= 2048, "%s: %d channels (a multiple of %d, at most 2048)", name, c, cmul);
  DTS_CHECK_ARG(eps >= 0.f, "%s: eps", name);
  DTS_CHECK_ARG(((uintptr_t)x | out.addr() | (uintptr_t)gamma | (uintptr_t)beta) % 16 == 0, "%s: pointers must be 16-byte aligned", name);
  hipLaunchKernelGGL((row_norm_kernel<In, A, Out>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, to_stream(s), x, stride, out, gamma, beta,
                     rows, c, eps);
  DTS_CHECK_LAUNCH(name);
  return DTS_OK;
}

}  // namespace
