// Grouping of bitwise-identical rows on the device: which rows of a [n][row_bytes] matrix are the same bytes, groups numbered in order of
// first occurrence.  It replaces the row sort + host synchronisation of torch.unique(dim=0, return_inverse=True) in front of the SD U-Net's
// forward (the 2N rows of a search step carry two distinct text contexts; sd_unet.SDUNet projects each distinct one once).  gfx950 only.
//
// Two short launches.  (1) one block per row sums a position-salted 32-bit mix of every dword of the row into a 128-bit fingerprint (integer
// adds: the result does not depend on the order of the partial sums).  (2) ONE block of 16 waves: a wave takes a row i, finds the rows j < i
// with the same fingerprint (64 candidates per LDS pass, one ballot), and compares row i with them in ascending j, all 64 lanes on 16-byte
// loads, until one is the same bytes -- a fingerprint match alone never counts as equality, so the result is exact for any input; a colliding
// fingerprint only costs a comparison.  Equal rows have equal fingerprints, so the earliest equal row is always among the candidates, and
// rows that have no earlier twin are never compared at all.  The group numbers are a prefix count of the first occurrences in LDS.
#include "dts_common.h"

namespace {

constexpr int GR_MAX_ROWS = 1024;       // one thread per row in the second launch
constexpr int GR_WAVES = GR_MAX_ROWS / 64;

__device__ __forceinline__ uint32_t gr_mix(uint32_t h) {      // the 32-bit finaliser of MurmurHash3 (public domain): a bijection
  h ^= h >> 16; h *= 0x85EBCA6Bu;
  h ^= h >> 13; h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

__global__ __launch_bounds__(256) void row_fingerprint_kernel(const uint4* __restrict__ rows, int chunks, uint4* __restrict__ fp) {
  const uint4* row = rows + (size_t)blockIdx.x * chunks;
  uint32_t h0 = 0, h1 = 0, h2 = 0, h3 = 0;
  for (int c = threadIdx.x; c < chunks; c += 256) {
    const uint4 v = row[c];
    const uint32_t salt = (uint32_t)c * 0x9E3779B1u;
    h0 += gr_mix(v.x ^ (salt + 0x1B873593u));
    h1 += gr_mix(v.y ^ (salt + 0xCC9E2D51u));
    h2 += gr_mix(v.z ^ (salt + 0x27D4EB2Fu));
    h3 += gr_mix(v.w ^ (salt + 0x165667B1u));
  }
  h0 = wave_sum(h0); h1 = wave_sum(h1); h2 = wave_sum(h2); h3 = wave_sum(h3);
  __shared__ uint4 part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = make_uint4(h0, h1, h2, h3);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint4 s = part[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) { s.x += part[w].x; s.y += part[w].y; s.z += part[w].z; s.w += part[w].w; }
    fp[blockIdx.x] = s;
  }
}

// whether rows a and b (chunks 16-byte vectors each) are the same bytes; the whole wave calls it with the same arguments
__device__ __forceinline__ bool gr_rows_equal(const uint4* __restrict__ a, const uint4* __restrict__ b, int chunks, int lane) {
  for (int c0 = 0; c0 < chunks; c0 += 256) {          // 4 KiB of each row per step, then leave at the first difference
    uint32_t diff = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + u * 64 + lane;
      if (c < chunks) {
        const uint4 x = a[c], y = b[c];
        diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
      }
    }
    if (__ballot(diff != 0) != 0) return false;
  }
  return true;
}

__global__ __launch_bounds__(GR_MAX_ROWS) void group_rows_kernel(const uint4* __restrict__ rows, int n, int chunks, const uint4* __restrict__ fp,
                                                                 int32_t* __restrict__ slot, int32_t* __restrict__ reps, int32_t* __restrict__ count) {
  __shared__ uint4 s_fp[GR_MAX_ROWS];
  __shared__ int s_first[GR_MAX_ROWS];                 // the earliest row with the same bytes (itself for a first occurrence)
  __shared__ int s_group[GR_MAX_ROWS];                 // first occurrences before row i
  __shared__ int s_wave[GR_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid < n) s_fp[tid] = fp[tid];
  __syncthreads();

  for (int i = wid; i < n; i += GR_WAVES) {            // wave-uniform: i, the ballots and every branch below
    const uint4 mine = s_fp[i];
    int first = i;
    for (int base = 0; base < i && first == i; base += 64) {
      const int j = base + lane;
      bool cand = false;
      if (j < i) {
        const uint4 f = s_fp[j];
        cand = f.x == mine.x && f.y == mine.y && f.z == mine.z && f.w == mine.w;
      }
      unsigned long long m = __ballot(cand);
      while (m != 0) {
        const int jj = base + __ffsll((long long)m) - 1;
        if (gr_rows_equal(rows + (size_t)i * chunks, rows + (size_t)jj * chunks, chunks, lane)) { first = jj; break; }
        m &= m - 1;                                    // same fingerprint, other bytes: on to the next candidate
      }
    }
    if (lane == 0) s_first[i] = first;
  }
  __syncthreads();

  // group numbers in order of first occurrence: exclusive prefix count of the first occurrences
  const bool is_first = tid < n && s_first[tid] == tid;
  const unsigned long long b = __ballot(is_first);
  if (lane == 0) s_wave[wid] = __popcll(b);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < GR_WAVES; ++w) {
    const int c = s_wave[w];
    before += w < wid ? c : 0;
    total += c;
  }
  const int g = before + __popcll(b & ((1ull << lane) - 1ull));
  if (tid < n) s_group[tid] = g;
  __syncthreads();
  if (tid < n) {
    slot[tid] = s_group[s_first[tid]];
    if (is_first) reps[g] = tid;
    if (tid >= total) reps[tid] = -1;
  }
  if (tid == 0) count[0] = total;
}

}  // namespace

extern "C" int dts_group_rows(const void* rows, int n, int64_t row_bytes, void* workspace, int32_t* slot, int32_t* reps, int32_t* count,
                              dts_stream s) {
  DTS_CHECK_ARG(rows && workspace && slot && reps && count, "dts_group_rows: null pointer");
  if (n < 1 || n > GR_MAX_ROWS || row_bytes < 16 || row_bytes % 16 != 0 || row_bytes / 16 > 0x7fffffffll) {
    dts_set_error("dts_group_rows: %d rows of %lld bytes (1 .. %d rows, whole 16-byte vectors)", n, (long long)row_bytes, GR_MAX_ROWS);
    return DTS_ERR_UNSUPPORTED;
  }
  DTS_CHECK_ARG(((uintptr_t)rows | (uintptr_t)workspace) % 16 == 0, "dts_group_rows: rows and workspace must be 16-byte aligned");
  DTS_CHECK_ARG(((uintptr_t)slot | (uintptr_t)reps | (uintptr_t)count) % 4 == 0, "dts_group_rows: outputs must be 4-byte aligned");
  const int chunks = (int)(row_bytes / 16);
  hipLaunchKernelGGL(row_fingerprint_kernel, dim3((unsigned)n), dim3(256), 0, to_stream(s), (const uint4*)rows, chunks, (uint4*)workspace);
  DTS_CHECK_LAUNCH("dts_group_rows (fingerprints)");
  hipLaunchKernelGGL(group_rows_kernel, dim3(1), dim3(GR_MAX_ROWS), 0, to_stream(s), (const uint4*)rows, n, chunks, (const uint4*)workspace, slot, reps,
                     count);
  DTS_CHECK_LAUNCH("dts_group_rows");
  return DTS_OK;
}
