// The three primitives of the SD U-Net's transformer blocks (diffusers BasicTransformerBlock: attention.py, attention_processor.py, activations.py
// of the reference's vendored diffusers) that the EDM networks never needed: attention over a SHORT foreign sequence (the 77 text tokens),
// LayerNorm over channels, and GEGLU.  16-bit storage (bf16 / f16), f32 arithmetic, gfx950 only.  LayerNorm also serves the CLIP towers,
// and has a second form for the split-precision vision tower (dts.h DTS_F16X3): float32 rows, float64 arithmetic, the result as float32
// rows and / or the next convolution's operand image (row_forms.h holds the one kernel behind both forms and behind dts_vit_head).
#include "row_forms.h"
#include <math.h>
#include <map>
#include <mutex>
#include <utility>

namespace {

template <typename T> struct XMma;
template <> struct XMma<bf16_t> {
  static __device__ __forceinline__ f32x4_t run(const uint4& a, const uint4& b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint32_t pack2(float lo, float hi) { return pack2_bf16(lo, hi); }
  static constexpr uint32_t ONES2 = 0x3F803F80u;            // two 1.0
};
template <> struct XMma<f16_t> {
  static __device__ __forceinline__ f32x4_t run(const uint4& a, const uint4& b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint32_t pack2(float lo, float hi) { return pack2_f16(lo, hi); }
  static constexpr uint32_t ONES2 = 0x3C003C00u;
};

// ------------------------------------------------------------------------------------------------
// Cross-attention: queries from the image tokens, keys / values from another, short sequence (tk <= 128).
//
// The MFMA arrangement is attention16_kernel's (attention.hip): one wave = 16 queries with the query on the MFMA column,
//   S^T[key][q] = K . Q^T,   O^T[d][q] = V^T . P^T  (V^T through transposed LDS reads, P straight from the S^T accumulators),
// but the whole K and V of a (sample, head) -- at most 128 rows -- sit in LDS at once (<= 2 * 128 * (2d + 32) B = 136 KiB at d = 256), so
// there is no key-tile loop and no online softmax: every score of a query is in registers (8 accumulator tiles of 16 keys) before the
// maximum is taken, the exponentials are taken once, and O is never rescaled.  A block stages K / V once and then walks `qchunks` chunks of
// 64 queries, so the staging is shared by up to 512 queries.  Keys past tk are masked to -inf (P = 0 exactly) and their LDS rows are zero,
// so a ragged tail (77 = 64 + 13) adds nothing to O or to the denominator.  The denominator is the sum of the ROUNDED P (an all-ones A
// operand against P^T), the same values that weigh V.
struct XAttP {
  const char* q; const char* kv; const int32_t* kv_rows; char* out;
  int n, kv_n, tq, tk, tkp, heads;
  float scale_log2e;
  int qblocks, qchunks;          // blocks per (sample, head); chunks of 64 queries per block
};

// DM < D (head dims 40 and 80 in memory on K widths 64 and 96; 160 is its own width), as in attention16_kernel: q, the k | v rows and out are
// heads * DM wide, the staging walks the on-chip chunk grid and writes zeros it never loaded for chunks >= DM/8 (they are the next head's
// bytes), the Q fragments get the same zero tail, ceil(DM/16) value tiles are multiplied and only channels < DM are stored.
template <typename T, int D, int DM = D>
__global__ __launch_bounds__(256) void cross_attention_kernel(const XAttP p) {
  static_assert(DM == D || (DM < D && DM % 8 == 0 && D == (DM + 31) / 32 * 32), "head dim in memory: whole 16-byte chunks, K width the next multiple of 32");
  constexpr int ES = 2, ROWB = D * ES + 32;        // LDS row stride: conflict-free for the b128 row reads of K and the transposed reads of V
  constexpr int CH = D / 8;                        // 16-byte chunks per row
  constexpr int CHM = DM / 8;                      // ... that exist in memory
  constexpr int KSTEPS = D / 32;
  constexpr int DT = DM == D ? D / 16 : (DM + 15) / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + p.tkp * ROWB;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lq = lane & 15, lg = lane >> 4;
  const int nh = blockIdx.x / p.qblocks, qblk = blockIdx.x - nh * p.qblocks;
  const int n = nh / p.heads, head = nh - n * p.heads;
  const int C = p.heads * DM;
  int kvn = p.kv_rows ? p.kv_rows[n] : n;
  kvn = min(max(kvn, 0), p.kv_n - 1);              // memory safety only: the caller's map is in range
  const char* kbase = p.kv + (size_t)kvn * p.tk * ((size_t)2 * C * ES) + (size_t)head * DM * ES;
  const size_t kvstride = (size_t)2 * C * ES;

  // ---- K and V of this (sample, head), zero rows from tk up to tkp (a multiple of 32: whole P.V k-steps)
  const int nchunks = p.tkp * CH;
#pragma unroll 4
  for (int idx = tid; idx < nchunks; idx += 256) {
    const int r = idx / CH, c = idx - r * CH;
    uint4 k = make_uint4(0, 0, 0, 0), v = make_uint4(0, 0, 0, 0);
    if (r < p.tk && (DM == D || c < CHM)) {
      const char* src = kbase + (size_t)r * kvstride + c * 16;
      k = *reinterpret_cast<const uint4*>(src);
      v = *reinterpret_cast<const uint4*>(src + (size_t)C * ES);
    }
    *reinterpret_cast<uint4*>(sK + r * ROWB + c * 16) = k;
    *reinterpret_cast<uint4*>(sV + r * ROWB + c * 16) = v;
  }
  __syncthreads();

  const float sc2 = p.scale_log2e;
  const uint4 ones = make_uint4(XMma<T>::ONES2, XMma<T>::ONES2, XMma<T>::ONES2, XMma<T>::ONES2);
  const size_t qstride = (size_t)C * ES;
  const char* qbase = p.q + (size_t)n * p.tq * qstride + (size_t)head * DM * ES;

  for (int qc = 0; qc < p.qchunks; ++qc) {
    const int q0 = (qblk * p.qchunks + qc) * 64 + wid * 16;
    if (q0 >= p.tq) break;                         // wave-uniform; no barrier follows
    const int qrow = q0 + lq;
    // Q fragments: B operand, lane holds Q[q][8*(lg + 4s) .. +8]
    uint4 qf[KSTEPS];
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      qf[s] = make_uint4(0, 0, 0, 0);
      if (qrow < p.tq && (DM == D || lg + 4 * s < CHM)) qf[s] = *reinterpret_cast<const uint4*>(qbase + (size_t)qrow * qstride + (lg + 4 * s) * 16);
    }
    // ---- S^T: up to 8 tiles of 16 keys x 16 queries; lane holds keys j*16 + lg*4 + r of query lq
    f32x4_t sacc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j * 16 < p.tkp) {
        sacc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
          const uint4 ka = *reinterpret_cast<const uint4*>(sK + (j * 16 + lq) * ROWB + (lg + 4 * s) * 16);
          sacc[j] = XMma<T>::run(ka, qf[s], sacc[j]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (j * 16 + lg * 4 + r >= p.tk) sacc[j][r] = -INFINITY;
      } else {
        sacc[j] = f32x4_t{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      }
    }
    // ---- softmax over ALL keys in one pass: maximum (finite: key 0 is always valid), exponentials, no rescale
    float m = sacc[0][0];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) m = fmaxf(m, sacc[j][r]);
    m = fmaxf(fmaxf(m, __shfl_xor(m, 16, 64)), fmaxf(__shfl_xor(m, 32, 64), __shfl_xor(m, 48, 64)));
    const float mb = m * sc2;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) sacc[j][r] = __builtin_amdgcn_exp2f(fmaf(sacc[j][r], sc2, -mb));     // exp2(-inf) = 0 for masked keys
    // ---- O^T = V^T . P^T and l = ones . P^T; P^T k-slot (lg, e): e < 4 -> key 32kk + 4lg + e, e >= 4 -> key 32kk + 16 + 4lg + e - 4
    f32x4_t o[DT];
    f32x4_t ol = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < DT; ++i) o[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (kk * 32 < p.tkp) {
        uint4 pb;
        pb.x = XMma<T>::pack2(sacc[2 * kk][0], sacc[2 * kk][1]);
        pb.y = XMma<T>::pack2(sacc[2 * kk][2], sacc[2 * kk][3]);
        pb.z = XMma<T>::pack2(sacc[2 * kk + 1][0], sacc[2 * kk + 1][1]);
        pb.w = XMma<T>::pack2(sacc[2 * kk + 1][2], sacc[2 * kk + 1][3]);
        ol = XMma<T>::run(ones, pb, ol);
        // transposed read: lane 4q'+p' of each 16-lane group addresses row q', columns 4p'..4p'+3 of a 4x16 block
        const int rq = (lane & 15) >> 2, rp = lane & 3;
        const char* va = sV + (32 * kk + 4 * lg + rq) * ROWB + rp * 8;
        const char* vb = va + 16 * ROWB;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(va + dt * 32));
          const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(vb + dt * 32));
          const uint2 lo2 = __builtin_bit_cast(uint2, lo), hi2 = __builtin_bit_cast(uint2, hi);
          o[dt] = XMma<T>::run(make_uint4(lo2.x, lo2.y, hi2.x, hi2.y), pb, o[dt]);
        }
      }
    }
    // ---- store: lane holds channels dt*16 + lg*4 .. +4 of query lq (8 bytes)
    if (qrow < p.tq) {
      const float inv = 1.f / ol[0];
      char* orow = p.out + ((size_t)n * p.tq + qrow) * qstride + (size_t)head * DM * ES;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        // DM = 40: channels 40..47 of the last tile are another block's to write
        if constexpr (DM % 16 != 0) { if (dt * 16 + lg * 4 >= DM) continue; }
        uint2 w;
        w.x = XMma<T>::pack2(o[dt][0] * inv, o[dt][1] * inv);
        w.y = XMma<T>::pack2(o[dt][2] * inv, o[dt][3] * inv);
        *reinterpret_cast<uint2*>(orow + (dt * 16 + lg * 4) * ES) = w;
      }
    }
  }
}

template <typename K>
int launch_xatt(K kernel, const XAttP& p, size_t lds, unsigned grid, hipStream_t st) {
  {   // the dynamic-LDS ceiling is a per-device attribute of the kernel: raise it once per (device, kernel)
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> done;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lk(mu);
    size_t& have = done[std::make_pair(dev, reinterpret_cast<const void*>(kernel))];
    if (lds > have) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) {      // nothing recorded: the next call tries again instead of launching with too small a ceiling
        dts_set_error("dts_cross_attention: cannot reserve %zu bytes of LDS per block: %s", lds, hipGetErrorString(e));
        return DTS_ERR_LAUNCH;
      }
      have = lds;
    }
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, st, p);
  DTS_CHECK_LAUNCH("dts_cross_attention");
  return DTS_OK;
}

template <typename T>
int xatt(const XAttP& p, int d, unsigned grid, hipStream_t st) {
  const size_t lds = (size_t)2 * p.tkp * ((d + 31) / 32 * 32 * 2 + 32);     // K and V rows at the on-chip K width (the head dim up to a multiple of 32)
  switch (d) {
    case 40: return launch_xatt(cross_attention_kernel<T, 64, 40>, p, lds, grid, st);
    case 80: return launch_xatt(cross_attention_kernel<T, 96, 80>, p, lds, grid, st);
    case 160: return launch_xatt(cross_attention_kernel<T, 160>, p, lds, grid, st);
    case 64: return launch_xatt(cross_attention_kernel<T, 64>, p, lds, grid, st);
    case 128: return launch_xatt(cross_attention_kernel<T, 128>, p, lds, grid, st);
    case 256: return launch_xatt(cross_attention_kernel<T, 256>, p, lds, grid, st);
  }
  return DTS_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------------
// GEGLU: out[r][j] = x[r][j] * gelu(x[r][inner + j]), gelu(g) = g * Phi(g) with Phi(g) = erfc(-g / sqrt 2) / 2 -- the erf form
// 0.5 * (1 + erf(g / sqrt 2)) written without its cancellation for negative g (at g = -6 the sum 1 + erf keeps no correct bit in f32).
template <typename T>
__global__ __launch_bounds__(256) void geglu_kernel(const T* __restrict__ x, T* __restrict__ out, long long rows, int inner) {
  const int vpr = inner >> 3;                      // vectors per output row
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * vpr) return;
  const long long r = idx / vpr;
  const int v = (int)(idx - r * vpr);
  const uint4* xr = reinterpret_cast<const uint4*>(x + r * 2 * inner);
  float a[8], g[8], y[8];
  unpack16<T>(xr[v], a);
  unpack16<T>(xr[vpr + v], g);
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = a[e] * (g[e] * (0.5f * erfcf(g[e] * -0.70710678118654752f)));
  reinterpret_cast<uint4*>(out + r * inner)[v] = pack16<T>(y);
}

}  // namespace

extern "C" int dts_cross_attention(const void* q, const void* kv, const int32_t* kv_rows, int kv_n, void* out, int dtype, int n, int tq, int tk,
                                   int heads, int d, float scale, dts_stream s) {
  DTS_CHECK_ARG(q && kv && out, "dts_cross_attention: null pointer");
  DTS_CHECK_ARG(n > 0 && tq > 0 && tk > 0 && heads > 0 && kv_n > 0, "dts_cross_attention: bad shape");
  DTS_CHECK_ARG(kv_rows != nullptr || kv_n == n, "dts_cross_attention: %d key/value rows for %d samples need a kv_rows map", kv_n, n);
  int (*run)(const XAttP&, int, unsigned, hipStream_t) = nullptr;
  DTS_DISPATCH_16BIT("dts_cross_attention", dtype, run = xatt<T>);
  DTS_CHECK_ARG(d == 64 || d == 128 || d == 256 || d == 40 || d == 80 || d == 160, "dts_cross_attention: head dim %d unsupported (40/64/80/128/160/256)", d);
  DTS_CHECK_ARG(scale > 0.f && isfinite(scale), "dts_cross_attention: scale must be positive and finite");
  DTS_CHECK_ARG(((uintptr_t)q | (uintptr_t)kv | (uintptr_t)out) % 16 == 0, "dts_cross_attention: pointers must be 16-byte aligned");
  if (tk > 128) {
    dts_set_error("dts_cross_attention: %d keys exceed the 128 whose K and V fit in LDS at once (dts_attention takes long sequences)", tk);
    return DTS_ERR_UNSUPPORTED;
  }
  XAttP p{(const char*)q, (const char*)kv, kv_rows, (char*)out, n, kv_n, tq, tk, (tk + 31) & ~31, heads, scale * 1.4426950408889634f, 0, 1};
  // chunks of 64 queries per block: share the K/V staging as widely as still leaves ~4 blocks per CU
  const long long nh = (long long)n * heads, chunks = (tq + 63) / 64;
  while (p.qchunks < 8 && nh * ((chunks + 2 * p.qchunks - 1) / (2 * p.qchunks)) >= 1024) p.qchunks *= 2;
  p.qblocks = (int)((chunks + p.qchunks - 1) / p.qchunks);
  const long long grid = nh * p.qblocks;
  DTS_CHECK_ARG(grid < (1ll << 31), "dts_cross_attention: grid too large");
  int r = run(p, d, (unsigned)grid, to_stream(s));
  if (r == DTS_ERR_UNSUPPORTED) dts_set_error("dts_cross_attention: head dim %d unsupported", d);
  return r;
}

extern "C" int dts_layer_norm(const void* x, void* out, int dtype, int64_t rows, int c, float eps, const float* gamma, const float* beta,
                              dts_stream s) {
  DTS_CHECK_ARG(x && out && gamma && beta, "dts_layer_norm: null pointer");
  DTS_DISPATCH_16BIT("dts_layer_norm", dtype, {
    DTS_CHECK_ARG(rows > 0 && rows < (1ll << 32), "dts_layer_norm: bad row count");
    return row_norm<float>("dts_layer_norm", (const T*)x, c, Out16<T>{(T*)out}, gamma, beta, rows, c, 8, eps, s);
  });
}

// LayerNorm over f32 rows [rows][c]; out_f32 (nullable): the normalised rows; out_split (nullable): their operand image [rows][2c].
// The two outputs come from the same registers, so the image is the split of the f32 rows whether or not those are written.
extern "C" int dts_layer_norm_x3(const float* x, float* out_f32, void* out_split, int64_t rows, int c, float eps, const float* gamma,
                                 const float* beta, dts_stream s) {
  DTS_CHECK_ARG(x && gamma && beta, "dts_layer_norm_x3: null pointer");
  DTS_CHECK_ARG(out_f32 || out_split, "dts_layer_norm_x3: neither out_f32 nor out_split");
  DTS_CHECK_ARG(rows > 0 && rows < (1ll << 32), "dts_layer_norm_x3: bad row count");
  return row_norm<double>("dts_layer_norm_x3", x, c, OutF32X3{out_f32, (uint4*)out_split}, gamma, beta, rows, c, 32, eps, s);
}

extern "C" int dts_geglu(const void* x, void* out, int dtype, int64_t rows, int inner, dts_stream s) {
  DTS_CHECK_ARG(x && out, "dts_geglu: null pointer");
  DTS_DISPATCH_16BIT("dts_geglu", dtype, {
    DTS_CHECK_ARG(rows > 0 && inner > 0 && inner % 8 == 0, "dts_geglu: %lld rows x %d (inner a multiple of 8)", (long long)rows, inner);
    DTS_CHECK_ARG(((uintptr_t)x | (uintptr_t)out) % 16 == 0, "dts_geglu: pointers must be 16-byte aligned");
    const long long nvec = rows * (inner / 8), grid = (nvec + 255) / 256;
    DTS_CHECK_ARG(grid < (1ll << 31), "dts_geglu: grid too large");
    hipLaunchKernelGGL(geglu_kernel<T>, dim3((unsigned)grid), dim3(256), 0, to_stream(s), (const T*)x, (T*)out, (long long)rows, inner);
  });
  DTS_CHECK_LAUNCH("dts_geglu");
  return DTS_OK;
}
