// K22: byte length of the baseline JPEG file of a uint8 RGB image, without writing the file (CompressibilityScorer(codec='hip'),
// edm/scorers.py:176-243: the reward is a function of len(PIL JPEG bytes) only).  The arithmetic is that of a baseline sequential
// JPEG (ITU T.81) as Pillow / libjpeg-turbo write it for quality=q: 16-bit fixed-point YCbCr, 4:2:0 chroma (2x2 mean with the
// alternating 1,2 rounding bias), the 13-bit "slow integer" forward DCT, quantisation with rounding half away from zero, the four
// Annex K Huffman tables, one scan of interleaved 16x16 MCUs.  Integer VALU / LDS work throughout; every intermediate fits int32.
//
// Five launches per call, all on the caller's stream:
//   jpeg_coef_kernel   one workgroup per MCU: colour, downsample, level shift, DCT, quantise -> int16 [block][64] zigzag, scan order
//   jpeg_bits_kernel   one wave per 8x8 block, one lane per coefficient: bits the block costs
//   jpeg_scan_kernel   one workgroup per image: exclusive prefix sum of the block bit counts = each block's bit offset
//   jpeg_emit_kernel   one wave per block: every lane ORs its own code into the image's zeroed bit buffer (integer OR commutes: the
//                      buffer does not depend on arrival order)
//   jpeg_count_kernel  0xFF bytes of the buffer (each is followed by a stuffed 0x00 in the file), the 1-padded last byte included
#include "dts_common.h"

namespace {

// ---- ITU T.81 Annex K.3: the typical Huffman tables (what a non-optimised encoder writes) -----------------------------------------
constexpr uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
constexpr uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
constexpr uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
constexpr uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

// code and length of every symbol (T.81 Annex C: codes of one length are consecutive, the first of the next length is the successor doubled);
// length 0 = the table has no such symbol
struct HuffTab {
  uint16_t code[256];
  uint8_t len[256];
};
constexpr HuffTab make_tab(const uint8_t (&bits)[16], const uint8_t* vals) {
  HuffTab t{};
  unsigned code = 0;
  int k = 0;
  for (int ln = 1; ln <= 16; ++ln) {
    for (int i = 0; i < bits[ln - 1]; ++i, ++k, ++code) {
      t.code[vals[k]] = (uint16_t)code;
      t.len[vals[k]] = (uint8_t)ln;
    }
    code <<= 1;
  }
  return t;
}
constexpr HuffTab kDcLuma = make_tab(kDcLumaBits, kDcVals), kDcChroma = make_tab(kDcChromaBits, kDcVals);
constexpr HuffTab kAcLuma = make_tab(kAcLumaBits, kAcLumaVals), kAcChroma = make_tab(kAcChromaBits, kAcChromaVals);
__constant__ HuffTab c_huff[4] = {kDcLuma, kDcChroma, kAcLuma, kAcChroma};       // [2 * is_ac + is_chroma]

// natural (row-major) index of the k-th coefficient of the zigzag sequence (T.81 figure A.6)
__constant__ uint8_t c_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kBlockMaxBits = 64 * (16 + 11);      // the most an 8x8 block costs: 64 coefficients of a 16-bit code and 11 value bits
constexpr int kBlockBufBytes = 256;                // bit-buffer bytes per 8x8 block: kBlockMaxBits = 1728 bits = 216 bytes
static_assert(kBlockMaxBits <= 8 * kBlockBufBytes, "a block's bits must fit its stretch of the bit buffer");
constexpr int kBlockBufWords = kBlockBufBytes / 4;

// ---- stage A ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One 8-point pass of the "slow integer" forward DCT (Loeffler-Ligtenberg-Moschytz, 12 multiplies): constants are cos / sin products
// scaled by 2^13.  The first (row) pass keeps 2 extra bits, the second (column) pass removes them again, so the 2-D result is the DCT
// scaled by 8 -- the factor the quantiser divides out with the table entry.
template <bool FIRST> __device__ __forceinline__ void fdct8(int (&d)[8]) {
  constexpr int N = FIRST ? 13 - 2 : 13 + 2;
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
  d[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
  const int e = (t12 + t13) * 4433;                       // 0.541196100
  d[2] = descale(e + t13 * 6270, N);                      // 0.765366865
  d[6] = descale(e - t12 * 15137, N);                     // 1.847759065
  const int z5 = (t4 + t6 + t5 + t7) * 9633;              // 1.175875602
  const int z1 = (t4 + t7) * -7373;                       // 0.899976223
  const int z2 = (t5 + t6) * -20995;                      // 2.562915447
  const int z3 = (t4 + t6) * -16069 + z5;                 // 1.961570560
  const int z4 = (t5 + t7) * -3196 + z5;                  // 0.390180644
  d[7] = descale(t4 * 2446 + z1 + z3, N);                 // 0.298631336
  d[5] = descale(t5 * 16819 + z2 + z4, N);                // 2.053119869
  d[3] = descale(t6 * 25172 + z2 + z3, N);                // 3.072711026
  d[1] = descale(t7 * 12299 + z1 + z4, N);                // 1.501321110
}

// grid = n * (h/16) * (w/16) workgroups of 256 threads, one per 16x16 MCU; coef [n][mcus][6][64]: Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr
__global__ __launch_bounds__(256) void jpeg_coef_kernel(const uint8_t* __restrict__ img, const uint16_t* __restrict__ qtab,
                                                         int16_t* __restrict__ coef, int h, int w) {
  __shared__ int blk[6][64];          // level-shifted samples, then DCT coefficients, natural order
  __shared__ int chroma[2][256];      // full-resolution Cb, Cr of the MCU
  __shared__ int16_t quant[6][64];
  const int mw = w >> 4, mcus = mw * (h >> 4);
  const int im = blockIdx.x / mcus, m = blockIdx.x % mcus;
  const int t = threadIdx.x, py = t >> 4, px = t & 15;
  const size_t plane = (size_t)h * w;
  const uint8_t* p = img + (size_t)im * 3 * plane + (size_t)((m / mw) * 16 + py) * w + (m % mw) * 16 + px;
  const int R = p[0], G = p[plane], B = p[2 * plane];
  blk[(py >> 3) * 2 + (px >> 3)][(py & 7) * 8 + (px & 7)] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
  chroma[0][t] = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
  chroma[1][t] = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
  __syncthreads();
  if (t < 128) {                      // 2x2 mean; the rounding bias alternates 1, 2 along a row so that halves do not all round up
    const int c = t >> 6, i = t & 63, ox = i & 7;
    const int* s = &chroma[c][(i >> 3) * 32 + ox * 2];
    blk[4 + c][i] = ((s[0] + s[1] + s[16] + s[17] + 1 + (ox & 1)) >> 2) - 128;
  }
  __syncthreads();
  if (t < 48) {                       // rows
    int* r = &blk[t >> 3][(t & 7) * 8];
    int d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = r[i];
    fdct8<true>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = d[i];
  }
  __syncthreads();
  if (t < 48) {                       // columns, then quantise: round half away from zero
    const int b = t >> 3, c = t & 7;
    int d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = blk[b][i * 8 + c];
    fdct8<false>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const unsigned q8 = 8u * qtab[(b >= 4 ? 64 : 0) + i * 8 + c];
      const int a = (int)(((unsigned)abs(d[i]) + (q8 >> 1)) / q8);
      quant[b][i * 8 + c] = (int16_t)(d[i] < 0 ? -a : a);
    }
  }
  __syncthreads();
  if (t < 192) {                      // two coefficients per thread, zigzag order
    const int b = t >> 5, k = (t & 31) * 2;
    const uint32_t lo = (uint16_t)quant[b][c_zigzag[k]], hi = (uint16_t)quant[b][c_zigzag[k + 1]];
    reinterpret_cast<uint32_t*>(coef + (size_t)blockIdx.x * 6 * 64)[t] = lo | (hi << 16);
  }
}

// ---- stages B and C: what lane k of a block's wave contributes to the stream ------------------------------------------------------
// Lane 0 sends the DC difference, a lane with a non-zero AC coefficient sends the ZRL codes its zero run needs, its run/size code and
// its value bits (at most 3 * 11 + 16 + 10 = 59 bits), lane 63 sends EOB when the last coefficient is zero.  Nothing is carried from
// lane to lane: a run is the distance to the previous non-zero position, read off the wave's ballot.
struct LaneBits {
  uint64_t bits;      // right-aligned, first bit of the stream in the highest of the n bits
  int n;
};
__device__ __forceinline__ int bit_size(int v) { return 32 - __clz(abs(v)); }                     // 0 for v == 0
__device__ __forceinline__ uint32_t value_bits(int v, int size) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u); }

// coef: the image's coefficients; b: block index in scan order.  Every lane of the wave must call this (ballot).
__device__ __forceinline__ LaneBits lane_code(const int16_t* __restrict__ coef, int b, int lane) {
  const int k6 = b % 6, is_chroma = k6 >= 4;
  const int v = coef[(size_t)b * 64 + lane];
  const uint64_t nz = __ballot(v != 0) | 1ull;              // position 0 (DC) bounds the first run
  LaneBits r{0, 0};
  if (lane == 0) {
    // previous block of the same component in scan order: the MCU's preceding Y block, else the previous MCU's last Y / its Cb / its Cr
    const int pb = k6 == 0 ? b - 3 : (k6 < 4 ? b - 1 : b - 6);
    const int diff = v - (pb >= 0 ? (int)coef[(size_t)pb * 64] : 0);
    const int size = bit_size(diff);
    const HuffTab& T = c_huff[is_chroma];
    r.bits = ((uint64_t)T.code[size] << size) | value_bits(diff, size);
    r.n = T.len[size] + size;
  } else if (v != 0) {
    const int prev = 63 - __clzll((long long)(nz & ((1ull << lane) - 1ull)));
    const int run = lane - 1 - prev;
    const HuffTab& T = c_huff[2 + is_chroma];
    for (int i = run >> 4; i > 0; --i) {                     // ZRL: sixteen zeros
      r.bits = (r.bits << T.len[0xF0]) | T.code[0xF0];
      r.n += T.len[0xF0];
    }
    const int size = bit_size(v), sym = ((run & 15) << 4) | size;
    r.bits = (((r.bits << T.len[sym]) | T.code[sym]) << size) | value_bits(v, size);
    r.n += T.len[sym] + size;
  } else if (lane == 63) {                                   // the tail is zero: EOB
    const HuffTab& T = c_huff[2 + is_chroma];
    r.bits = T.code[0];
    r.n = T.len[0];
  }
  return r;
}

// one wave per block; bitoff[n * nb] receives the block's bit count
__global__ __launch_bounds__(256) void jpeg_bits_kernel(const int16_t* __restrict__ coef, int* __restrict__ bitoff, int nb, int total) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= total) return;                                    // whole waves leave together
  const int im = g / nb;
  const LaneBits r = lane_code(coef + (size_t)im * nb * 64, g - im * nb, lane);
  const int s = wave_sum(r.n);
  if (lane == 0) bitoff[g] = s;
}

// one workgroup per image: bitoff[im][:] bit counts -> exclusive prefix sums, in place; totals[im] = bits of the image's scan;
// sizes[im] = header + entropy bytes + EOI (jpeg_count_kernel adds the stuffed bytes)
__global__ __launch_bounds__(256) void jpeg_scan_kernel(int* __restrict__ bitoff, int* __restrict__ totals, int* __restrict__ sizes, int nb,
                                                         int header) {
  __shared__ int part[256];
  const int t = threadIdx.x;
  int* p = bitoff + (size_t)blockIdx.x * nb;
  const int per = (nb + 255) / 256, lo = min(t * per, nb), hi = min(lo + per, nb);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += p[i];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;
  for (int i = lo; i < hi; ++i) {
    const int c = p[i];
    p[i] = run;
    run += c;
  }
  if (t == 255) {
    totals[blockIdx.x] = part[255];
    sizes[blockIdx.x] = header + ((part[255] + 7) >> 3) + 2;
  }
}

// one wave per block; bitbuf [n][nb * kBlockBufWords] zeroed words, bit i of the stream = bit 31 - (i & 31) of word i >> 5
__global__ __launch_bounds__(256) void jpeg_emit_kernel(const int16_t* __restrict__ coef, const int* __restrict__ bitoff,
                                                         uint32_t* __restrict__ bitbuf, int nb, int total) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= total) return;
  const int im = g / nb;
  const LaneBits r = lane_code(coef + (size_t)im * nb * 64, g - im * nb, lane);
  int incl = r.n;                                            // inclusive prefix sum over the lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  const int pos = bitoff[g] + incl - r.n, word = pos >> 5, sh = pos & 31;
  if (r.n == 0 || word + 2 >= nb * kBlockBufWords) return;   // (the bound cannot bind: see kBlockBufBytes)
  const uint64_t v = r.bits << (64 - r.n);                   // left-aligned
  const uint64_t top = v >> sh;
  const uint32_t w0 = (uint32_t)(top >> 32), w1 = (uint32_t)top, w2 = sh ? (uint32_t)v << (32 - sh) : 0u;
  uint32_t* dst = bitbuf + (size_t)im * nb * kBlockBufWords + word;
  if (w0) atomicOr(dst, w0);
  if (w1) atomicOr(dst + 1, w1);
  if (w2) atomicOr(dst + 2, w2);
}

// grid (ceil(nb * kBlockBufWords / 256), n); one word per thread
__global__ __launch_bounds__(256) void jpeg_count_kernel(const uint32_t* __restrict__ bitbuf, const int* __restrict__ totals,
                                                          int* __restrict__ sizes, int nb) {
  const int im = blockIdx.y, bits = totals[im], nbytes = (bits + 7) >> 3;
  const int i = blockIdx.x * 256 + threadIdx.x;
  int c = 0;
  if (i < nb * kBlockBufWords && i * 4 < nbytes) {
    uint32_t w = bitbuf[(size_t)im * nb * kBlockBufWords + i];
    if ((bits & 7) && i == (bits >> 5)) {                    // the last, partial byte is completed with 1-bits
      const int a = bits & 31, e = (a | 7) + 1;
      w |= (0xFFFFFFFFu >> a) & (e == 32 ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> e));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) c += (i * 4 + j < nbytes) && ((w >> (24 - 8 * j)) & 0xFFu) == 0xFFu;
  }
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&sizes[im], c);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// SOI | APP0 (JFIF) | 2 x DQT | SOF0 (3 components) | 4 x DHT | SOS (3 components): marker (2) + length field (2) + payload each
constexpr int kHeaderBytes = 2 + (4 + 14) + 2 * (4 + 1 + 64) + (4 + 6 + 3 * 3) + 2 * (4 + 1 + 16 + sizeof(kDcVals)) +
                             (4 + 1 + 16 + sizeof(kAcLumaVals)) + (4 + 1 + 16 + sizeof(kAcChromaVals)) + (4 + 1 + 3 * 2 + 3);

inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }
inline bool shape_ok(int n, int h, int w) {
  return n >= 1 && n <= 65535 && h >= 16 && w >= 16 && h % 16 == 0 && w % 16 == 0 && h <= 16384 && w <= 16384 &&
         (int64_t)n * (h / 16) * (w / 16) * 6 <= (1 << 24) &&
         // bit counts, offsets and positions are int: an image's blocks, at the most a block costs, must stay below 2^31 bits
         (int64_t)(h / 16) * (w / 16) * 6 * kBlockMaxBits < ((int64_t)1 << 31);
}
struct Layout {
  int nb;                                   // 8x8 blocks per image
  int64_t coef, bitoff, totals, bitbuf, bytes;
};
inline Layout layout(int n, int h, int w) {
  Layout L;
  L.nb = (h / 16) * (w / 16) * 6;
  const int64_t blocks = (int64_t)n * L.nb;
  L.coef = 0;
  L.bitoff = L.coef + align256(blocks * 64 * 2);
  L.totals = L.bitoff + align256(blocks * 4);
  L.bitbuf = L.totals + align256((int64_t)n * 4);
  L.bytes = L.bitbuf + align256(blocks * kBlockBufBytes);
  return L;
}

}  // namespace

extern "C" int64_t dts_jpeg_workspace_bytes(int n, int h, int w) { return shape_ok(n, h, w) ? layout(n, h, w).bytes : 0; }

extern "C" int dts_jpeg_size(const uint8_t* img, int32_t* sizes, int n, int h, int w, const uint16_t* qtab, void* workspace,
                             int64_t workspace_bytes, int16_t* coef_out, dts_stream s) {
  DTS_CHECK_ARG(img && sizes && qtab && workspace, "dts_jpeg_size: null pointer");
  DTS_CHECK_ARG(shape_ok(n, h, w), "dts_jpeg_size: n=%d h=%d w=%d: whole 16x16 MCUs only (h, w multiples of 16), 1 <= n <= 65535, blocks per image * %d bits < 2^31", n, h, w, kBlockMaxBits);
  const Layout L = layout(n, h, w);
  DTS_CHECK_ARG(workspace_bytes >= L.bytes && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                "dts_jpeg_size: workspace of %lld bytes, 16-byte aligned, needed (dts_jpeg_workspace_bytes); got %lld", (long long)L.bytes,
                (long long)workspace_bytes);
  DTS_CHECK_ARG(!coef_out || (reinterpret_cast<uintptr_t>(coef_out) & 3) == 0, "dts_jpeg_size: coef_out must be 4-byte aligned");
  hipStream_t st = to_stream(s);
  char* ws = static_cast<char*>(workspace);
  int16_t* coef = coef_out ? coef_out : reinterpret_cast<int16_t*>(ws + L.coef);
  int* bitoff = reinterpret_cast<int*>(ws + L.bitoff);
  int* totals = reinterpret_cast<int*>(ws + L.totals);
  uint32_t* bitbuf = reinterpret_cast<uint32_t*>(ws + L.bitbuf);
  const int blocks = n * L.nb, waves4 = (blocks + 3) / 4;
  if (hipMemsetAsync(bitbuf, 0, (size_t)blocks * kBlockBufBytes, st) != hipSuccess) {
    dts_set_error("dts_jpeg_size: hipMemsetAsync failed: %s", hipGetErrorString(hipGetLastError()));
    return DTS_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(jpeg_coef_kernel, dim3(n * (L.nb / 6)), dim3(256), 0, st, img, qtab, coef, h, w);
  DTS_CHECK_LAUNCH("dts_jpeg_size (coefficients)");
  hipLaunchKernelGGL(jpeg_bits_kernel, dim3(waves4), dim3(256), 0, st, (const int16_t*)coef, bitoff, L.nb, blocks);
  DTS_CHECK_LAUNCH("dts_jpeg_size (bit counts)");
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(n), dim3(256), 0, st, bitoff, totals, sizes, L.nb, kHeaderBytes);
  DTS_CHECK_LAUNCH("dts_jpeg_size (offsets)");
  hipLaunchKernelGGL(jpeg_emit_kernel, dim3(waves4), dim3(256), 0, st, (const int16_t*)coef, (const int*)bitoff, bitbuf, L.nb, blocks);
  DTS_CHECK_LAUNCH("dts_jpeg_size (emission)");
  hipLaunchKernelGGL(jpeg_count_kernel, dim3((L.nb * kBlockBufWords + 255) / 256, n), dim3(256), 0, st, (const uint32_t*)bitbuf,
                     (const int*)totals, sizes, L.nb);
  DTS_CHECK_LAUNCH("dts_jpeg_size (stuffed bytes)");
  return DTS_OK;
}
