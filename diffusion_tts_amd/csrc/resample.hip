// The NCSN++ resampling passes (SongUNet with resample_filter = [1,3,3,1], encoder_type = 'residual'; networks.py:64-90, 290-292):
//   dts_resample_fir      2x down / up sampling of an NHWC tensor with the separable [1,3,3,1] filter
//   dts_space_to_depth2   the 2x2 pixel-block -> channel rearrangement that turns the residual encoder's fused-resample convolution
//                         (3x3 pad 2, then the depthwise filter at stride 2) into ONE 3x3 pad-1 convolution for dts_conv2d
// Both are HBM-bound gathers: a thread owns one 16-byte vector of output channels (two in the split-precision form), reads its 4x4 / 2x2
// neighbourhood with 16-byte loads along C (adjacent threads = adjacent channel vectors of one pixel: coalesced; the overlap between
// neighbouring outputs is served by L2) and writes 16-byte vectors.  No LDS.  Arithmetic in f32.
#include "dts_common.h"

namespace {

inline int grid1d(long long total, int block = 256, int cap = 256 * 8) {
  long long g = (total + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// E consecutive channels of a pixel as floats: NV 16-byte vectors of T
template <typename T, int NV>
__device__ __forceinline__ void load_vec(const T* p, float* f) {
#pragma unroll
  for (int v = 0; v < NV; ++v) unpack16<T>(reinterpret_cast<const uint4*>(p)[v], f + v * ET<T>::EPV);
}

// store E = 8 f32 results as the split-precision operand image (dts_split3_f16's arithmetic and layout): `row` = the pixel's 2*C f16 row
__device__ __forceinline__ void store_split8(void* row, int c0, const float* r) {
  float hi[8], lo[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x3_split(r[e], hi[e], lo[e]);
  f16_t* o = reinterpret_cast<f16_t*>(row) + x3_off(c0);              // c0 % 8 == 0: the 8 channels stay inside one group of 32
  *reinterpret_cast<uint4*>(o) = pack16<f16_t>(hi);
  *reinterpret_cast<uint4*>(o + 32) = pack16<f16_t>(lo);
}

// SPLIT: T = float in, f16 split image [..][2*c] out, 8 channels per thread; else T in, T out, one 16-byte vector per thread.
// up = 0: out[i][j] = sum_{a,b} k[a] k[b] / 64 * x[2i-1+a][2j-1+b]      (conv2d with outer(k,k)/64, stride 2, padding 1)
// up = 1: per axis out[2m] = 3/4 x[m] + 1/4 x[m-1], out[2m+1] = 3/4 x[m] + 1/4 x[m+1]   (conv_transpose2d with 4 * that filter, stride 2,
//         padding 1); pixels outside the image are zero in both.
template <typename T, bool SPLIT>
__global__ __launch_bounds__(256) void resample_fir_kernel(const T* __restrict__ x, void* __restrict__ out, int n_total, int h, int w, int c,
                                                            int up) {
  constexpr int NV = SPLIT ? 2 : 1, E = ET<T>::EPV * NV;
  const int nchunk = c / E;
  const int ho = up ? 2 * h : h / 2, wo = up ? 2 * w : w / 2;
  const long long total = (long long)n_total * ho * wo * nchunk;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int chunk = (int)(idx % nchunk), c0 = chunk * E;
    long long pix = idx / nchunk;
    const int xo = (int)(pix % wo); pix /= wo;
    const int yo = (int)(pix % ho);
    const int n = (int)(pix / ho);
    const T* img = x + (size_t)n * h * w * c + c0;
    float r[E];
#pragma unroll
    for (int e = 0; e < E; ++e) r[e] = 0.f;
    if (up) {
      // the two source rows / columns of this output and their weights: the nearer one 3/4, the farther one 1/4
      const int my = yo >> 1, mx = xo >> 1;
      const int y2 = (yo & 1) ? my + 1 : my - 1, x2 = (xo & 1) ? mx + 1 : mx - 1;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int yy = a ? y2 : my;
        if (yy < 0 || yy >= h) continue;
        float row[E];
#pragma unroll
        for (int e = 0; e < E; ++e) row[e] = 0.f;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int xx = b ? x2 : mx;
          if (xx < 0 || xx >= w) continue;
          float f[E];
          load_vec<T, NV>(img + ((size_t)yy * w + xx) * c, f);
          const float kb = b ? 0.25f : 0.75f;
#pragma unroll
          for (int e = 0; e < E; ++e) row[e] += kb * f[e];
        }
        const float ka = a ? 0.25f : 0.75f;
#pragma unroll
        for (int e = 0; e < E; ++e) r[e] += ka * row[e];
      }
    } else {
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int yy = 2 * yo - 1 + a;
        if (yy < 0 || yy >= h) continue;
        float row[E];
#pragma unroll
        for (int e = 0; e < E; ++e) row[e] = 0.f;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int xx = 2 * xo - 1 + b;
          if (xx < 0 || xx >= w) continue;
          float f[E];
          load_vec<T, NV>(img + ((size_t)yy * w + xx) * c, f);
          const float kb = (b == 1 || b == 2) ? 0.375f : 0.125f;       // [1,3,3,1] / 8 per axis: exact binary fractions
#pragma unroll
          for (int e = 0; e < E; ++e) row[e] += kb * f[e];
        }
        const float ka = (a == 1 || a == 2) ? 0.375f : 0.125f;
#pragma unroll
        for (int e = 0; e < E; ++e) r[e] += ka * row[e];
      }
    }
    const size_t opix = ((size_t)n * ho + yo) * wo + xo;
    if constexpr (SPLIT) {
      store_split8(reinterpret_cast<f16_t*>(out) + opix * 2 * c, c0, r);
    } else {
      *reinterpret_cast<uint4*>(reinterpret_cast<T*>(out) + opix * c + c0) = pack16<T>(r);
    }
  }
}

// out[n][i][j][(ry*2+rx)*c + ci] = x[n][2i+ry][2j+rx][ci]  (x NHWC in T, or f32 NCHW when NCHW), channels 4c .. cpad-1 zero.
// VEC: c is a multiple of the thread's E channels, so a thread's output vector comes from one input vector; otherwise (the 3-channel image,
// odd channel counts) element by element.  SPLIT / T as above; with NCHW the input is float whatever T is.
template <typename T, bool SPLIT, bool NCHW, bool VEC>
__global__ __launch_bounds__(256) void space_to_depth2_kernel(const void* __restrict__ xv, void* __restrict__ out, int n_total, int h, int w,
                                                               int c, int cpad) {
  constexpr int NV = SPLIT ? 2 : 1, E = ET<T>::EPV * NV;
  const int nchunk = cpad / E;
  const int ho = h / 2, wo = w / 2;
  const long long total = (long long)n_total * ho * wo * nchunk;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int chunk = (int)(idx % nchunk), k0 = chunk * E;
    long long pix = idx / nchunk;
    const int xo = (int)(pix % wo); pix /= wo;
    const int yo = (int)(pix % ho);
    const int n = (int)(pix / ho);
    float r[E];
    if constexpr (VEC) {
      if (k0 < 4 * c) {
        const int ph = k0 / c, ci = k0 - ph * c;
        const T* src = reinterpret_cast<const T*>(xv) + (((size_t)n * h + 2 * yo + (ph >> 1)) * w + 2 * xo + (ph & 1)) * c + ci;
        load_vec<T, NV>(src, r);
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) r[e] = 0.f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int k = k0 + e;
        float v = 0.f;
        if (k < 4 * c) {
          const int ph = k / c, ci = k - ph * c, yy = 2 * yo + (ph >> 1), xx = 2 * xo + (ph & 1);
          if constexpr (NCHW) v = reinterpret_cast<const float*>(xv)[(((size_t)n * c + ci) * h + yy) * w + xx];
          else v = ld1<T>(reinterpret_cast<const T*>(xv) + (((size_t)n * h + yy) * w + xx) * c + ci);
        }
        r[e] = v;
      }
    }
    const size_t opix = ((size_t)n * ho + yo) * wo + xo;
    if constexpr (SPLIT) {
      store_split8(reinterpret_cast<f16_t*>(out) + opix * 2 * cpad, k0, r);
    } else {
      *reinterpret_cast<uint4*>(reinterpret_cast<T*>(out) + opix * cpad + k0) = pack16<T>(r);
    }
  }
}

}  // namespace

extern "C" int dts_resample_fir(const void* x, void* out, int dtype, int n, int h, int w, int c, int up, int split_out, dts_stream s) {
  DTS_CHECK_ARG(x && out, "dts_resample_fir: null pointer");
  DTS_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0, "dts_resample_fir: n=%d h=%d w=%d c=%d", n, h, w, c);
  DTS_CHECK_ARG(up == 1 || (up == 0 && h % 2 == 0 && w % 2 == 0), "dts_resample_fir: down needs even h,w (up=%d h=%d w=%d)", up, h, w);
  DTS_CHECK_ARG(!split_out || (dtype == DTS_F32 && c % 32 == 0), "dts_resample_fir: the split image takes f32 input and c %% 32 == 0 (dtype=%d c=%d)",
                dtype, c);
  const int e = split_out ? 8 : (dtype == DTS_F32 ? 4 : 8);
  DTS_CHECK_ARG(c % e == 0, "dts_resample_fir: c=%d is not a multiple of %d", c, e);
  hipStream_t st = to_stream(s);
  const long long total = (long long)n * (up ? 2 * h : h / 2) * (up ? 2 * w : w / 2) * (c / e);
  if (split_out) {
    hipLaunchKernelGGL((resample_fir_kernel<float, true>), dim3(grid1d(total)), dim3(256), 0, st, (const float*)x, out, n, h, w, c, up);
    DTS_CHECK_LAUNCH("dts_resample_fir");
    return DTS_OK;
  }
  DTS_DISPATCH_DTYPE(dtype, {
    hipLaunchKernelGGL((resample_fir_kernel<T, false>), dim3(grid1d(total)), dim3(256), 0, st, (const T*)x, out, n, h, w, c, up);
    DTS_CHECK_LAUNCH("dts_resample_fir");
  });
  return DTS_OK;
}

extern "C" int dts_space_to_depth2(const void* x, int x_nchw_f32, void* out, int dtype, int n, int h, int w, int c, int cpad, int split_out,
                                   dts_stream s) {
  DTS_CHECK_ARG(x && out, "dts_space_to_depth2: null pointer");
  DTS_CHECK_ARG(n > 0 && h > 0 && w > 0 && c > 0 && h % 2 == 0 && w % 2 == 0, "dts_space_to_depth2: n=%d h=%d w=%d c=%d (even h,w)", n, h, w, c);
  DTS_CHECK_ARG(!split_out || (dtype == DTS_F32 && cpad % 32 == 0), "dts_space_to_depth2: the split image is f32 in, cpad %% 32 == 0 (dtype=%d cpad=%d)",
                dtype, cpad);
  const int e = split_out ? 8 : (dtype == DTS_F32 ? 4 : 8);
  DTS_CHECK_ARG(cpad >= 4 * c && cpad % e == 0, "dts_space_to_depth2: cpad=%d must be >= 4*c=%d and a multiple of %d", cpad, 4 * c, e);
  hipStream_t st = to_stream(s);
  const long long total = (long long)n * (h / 2) * (w / 2) * (cpad / e);
  const bool vec = !x_nchw_f32 && c % e == 0;
  const dim3 g(grid1d(total)), b(256);
#define DTS_S2D(T, SPLIT)                                                                                                         \
  do {                                                                                                                            \
    if (x_nchw_f32) hipLaunchKernelGGL((space_to_depth2_kernel<T, SPLIT, true, false>), g, b, 0, st, x, out, n, h, w, c, cpad);   \
    else if (vec) hipLaunchKernelGGL((space_to_depth2_kernel<T, SPLIT, false, true>), g, b, 0, st, x, out, n, h, w, c, cpad);     \
    else hipLaunchKernelGGL((space_to_depth2_kernel<T, SPLIT, false, false>), g, b, 0, st, x, out, n, h, w, c, cpad);             \
    DTS_CHECK_LAUNCH("dts_space_to_depth2");                                                                                      \
  } while (0)
  if (split_out) {
    DTS_S2D(float, true);
    return DTS_OK;
  }
  DTS_DISPATCH_DTYPE(dtype, { DTS_S2D(T, false); });
#undef DTS_S2D
  return DTS_OK;
}
