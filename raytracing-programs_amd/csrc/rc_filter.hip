// rc_filter.hip — the separable reconstruction filter of the supersampled image.
//
// dst (W x H) <- src (s*W x s*H), both compact RGB, through a 1-D integer tap vector k[0..L),
// L = s + 2h, applied along x and then along y with src's coordinates clamped to the image:
//     acc = sum_j sum_i k[j] k[i] src[clamp(s*y - h + j)][clamp(s*x - h + i)][c]
//     dst = clamp((acc + S*S/2) / (S*S), 0, 255),  S = sum k
// With sum |k| <= 2048 a horizontal sum is below 2048 * 255 < 2^19 in magnitude and acc + S*S/2
// below 2048^2 * 255 + 2^21 < 2^31: every intermediate fits int32 and the separable evaluation
// is exact (include/raycast_hip.h, rc_filter).
//
// The kernel is compiled per factor s and per halo class hk in {0, s/2, s}: a tap vector with
// halo h runs in the smallest class hk >= h with hk - h zero taps added at either end, which
// changes no sum.  So the tap count, the staged region and every loop bound are constants.
//
// One workgroup (256 threads) per TW x TH tile of output pixels:
//   stage   the tile's (s*TW + 2hk) x (s*TH + 2hk) pixels of src into LDS as packed dwords, one
//           wave per region row.  The clamp is applied here, to the load indices, so the passes
//           below are uniform.  A dword whose four bytes lie inside a source row is one dword
//           load from whatever address that is (src's rows are 3*s*W bytes: no alignment is
//           assumed); one that touches a clamped column is put together from byte loads.
//   pass 1  one thread per (region row, output column): its 3L bytes are contiguous in the row;
//           they are read as dwords, taken apart in registers, and the three channels' sums are
//           stored as int32.
//   pass 2  one thread per four consecutive bytes of an output row: L reads of 16 bytes of
//           partial sums, the rounding division, the clamp, and one dword store (byte stores where
//           the output row is not 4-byte aligned or ends inside the dword).
// LDS per workgroup (region + partial sums), at the widest halo class:
//   s = 2   32 x 16 tile    7.5 + 13.5 = 21.0 KiB
//   s = 4   32 x  8 tile   16.3 + 15.0 = 31.3 KiB
//   s = 8   16 x  8 tile   34.4 + 15.0 = 49.4 KiB
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rc_kernels.h"

namespace rc {
namespace {

constexpr int kFilterThreads = 256;

struct FilterTaps {
  int k[kFilterMaxTaps];   // the class's S + 2*HK taps (zero-extended), by value: scalar registers
};

template <int S, int HK>
struct FilterGeom {
  static constexpr int TW = filter_tile_w(S), TH = filter_tile_h(S);
  static constexpr int L = S + 2 * HK;            // taps
  static constexpr int RW = S * TW + 2 * HK;      // region: pixels per row
  static constexpr int RH = S * TH + 2 * HK;      // region: rows
  static constexpr int SBW = (3 * RW + 3) / 4;    // staged dwords per region row
  static constexpr int SB = SBW + 2;              // row stride: pass 1 reads up to one dword past
                                                  // the last staged one (never its bytes)
  static constexpr int PW = TW * 3;               // partial sums per region row
  static constexpr int NW = (3 * L + 3) / 4;      // dwords holding one thread's 3L bytes
  static_assert(TW % 4 == 0, "an output row segment is a whole number of dwords");
  static_assert((RH * SB + RH * PW) * 4 <= 64 * 1024, "static LDS");
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// Bytes 4j .. 4j+3 of a region row whose pixel 0 is column gx0 of the source row at rowp, with
// the clamp applied to each byte's column: the dwords that touch the image's left or right edge.
__device__ __forceinline__ uint32_t stage_bytes(const uint8_t* __restrict__ rowp, int gx0, int sw,
                                                int j) {
  uint32_t v = 0u;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int b = 4 * j + t, p = b / 3, ch = b - 3 * p;
    const int gx = clampi(gx0 + p, 0, sw - 1);
    v |= (uint32_t)rowp[(size_t)gx * 3 + ch] << (8 * t);
  }
  return v;
}

// Four bytes from any address: one dword load (the target's global loads take unaligned
// addresses; src's rows are 3*s*W bytes, so a region row starts at any byte).
__device__ __forceinline__ uint32_t load_u32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

template <int S, int HK>
__global__ void __launch_bounds__(kFilterThreads) k_filter_down(
    const uint8_t* __restrict__ src, int W, int H, FilterTaps f, unsigned div, int shift,
    int tiles_x, uint8_t* __restrict__ dst) {
  using G = FilterGeom<S, HK>;
  __shared__ uint32_t region[G::RH * G::SB];
  __shared__ __attribute__((aligned(16))) int part[G::RH * G::PW];
  const int tid = threadIdx.x;
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x % (unsigned)tiles_x);
  const int sw = W * S, sh = H * S;               // <= 2^28 each (launch_filter_down)
  const size_t rowb = (size_t)sw * 3;
  const int gx0 = tx * G::TW * S - HK, gy0 = ty * G::TH * S - HK;

  // stage: region[r][j] = bytes 4j .. 4j+3 of region row r (pixel p = byte / 3 of the row is
  // src's column clamp(gx0 + p) of row clamp(gy0 + r)).  One wave per region row, so a row's
  // clamp and address are scalar work, and all of a wave's kRows rows in one step, their loads
  // issued before the first use (a step of fewer rows would load the tail's rows twice: measured,
  // DESIGN.md section 13).  A dword with no clamped column is one load of the four contiguous bytes; the others
  // (tiles on the image's left and right edge only) load from a clamped address all the same,
  // so that no branch splits the loads, and are then put together from byte loads.
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  constexpr int kWaves = kFilterThreads / 64, kCols = (G::SBW + 63) / 64;
  constexpr int kRows = (G::RH + kWaves - 1) / kWaves;
  const int rowb4 = sw * 3 - 4;   // the last offset four bytes of a row can be loaded at (sw >= 2)
  int bo[kCols];                  // the dword's byte offset in the source row, and whether
  bool whole[kCols];              // all four bytes lie in the row
#pragma unroll
  for (int q = 0; q < kCols; ++q) {
    const int o = gx0 * 3 + 4 * min(lane + 64 * q, G::SBW - 1);
    whole[q] = o >= 0 && o <= rowb4;
    bo[q] = clampi(o, 0, rowb4);
  }
  {
    const int r0 = wave;
    uint32_t v[kRows][kCols];
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
      // past the last row (fewer than kWaves rows a tile): the last row again, the same bytes
      // to the same place
      const int r = min(r0 + u * kWaves, G::RH - 1);
      const uint8_t* rowp = src + (size_t)clampi(gy0 + r, 0, sh - 1) * rowb;
#pragma unroll
      for (int q = 0; q < kCols; ++q) v[u][q] = load_u32(rowp + bo[q]);
    }
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
      const int r = min(r0 + u * kWaves, G::RH - 1);
      const uint8_t* rowp = src + (size_t)clampi(gy0 + r, 0, sh - 1) * rowb;
#pragma unroll
      for (int q = 0; q < kCols; ++q) {
        const int j = lane + 64 * q;
        if (j < G::SBW)
          region[r * G::SB + j] = whole[q] ? v[u][q] : stage_bytes(rowp, gx0, sw, j);
      }
    }
  }
  __syncthreads();

  // pass 1: part[r][3x + c] = sum_i k[i] * byte(r, 3*(S*x + i) + c)
  for (int it = tid; it < G::RH * G::TW; it += kFilterThreads) {
    const int r = it / G::TW, x = it % G::TW;
    const int b0 = 3 * S * x;
    const uint32_t* row = region + r * G::SB + (b0 >> 2);
    uint32_t a[G::NW];
    if constexpr (S % 4 == 0) {   // b0 is a multiple of 4
#pragma unroll
      for (int q = 0; q < G::NW; ++q) a[q] = row[q];
    } else {
      const uint32_t off = (uint32_t)(b0 & 3);
      uint32_t w[G::NW + 1];
#pragma unroll
      for (int q = 0; q <= G::NW; ++q) w[q] = row[q];
#pragma unroll
      for (int q = 0; q < G::NW; ++q) a[q] = __builtin_amdgcn_alignbyte(w[q + 1], w[q], off);
    }
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < G::L; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int n = 3 * i + c;
        acc[c] += f.k[i] * (int)((a[n >> 2] >> (8 * (n & 3))) & 0xffu);
      }
    int* p = part + r * G::PW + 3 * x;
    p[0] = acc[0];
    p[1] = acc[1];
    p[2] = acc[2];
  }
  __syncthreads();

  // pass 2: four consecutive bytes e0 .. e0+3 of output row y of the tile
  const unsigned half = div >> 1;
  const size_t orow = (size_t)W * 3;
  for (int it = tid; it < G::TH * (G::PW / 4); it += kFilterThreads) {
    const int y = it / (G::PW / 4), e0 = (it % (G::PW / 4)) * 4;
    int acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < G::L; ++j) {
      const int4 v = *(const int4*)(part + (S * y + j) * G::PW + e0);
      acc[0] += f.k[j] * v.x;
      acc[1] += f.k[j] * v.y;
      acc[2] += f.k[j] * v.z;
      acc[3] += f.k[j] * v.w;
    }
    const int oy = ty * G::TH + y;
    const long long ex = (long long)tx * G::PW + e0;   // byte column in the output row
    if (oy >= H || ex >= (long long)orow) continue;
    uint32_t o = 0u;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int u = acc[t] + (int)half;   // < 2^31; negative: clamps to 0 whatever the rounding
      unsigned q = 0u;
      if (u > 0) q = shift >= 0 ? (unsigned)u >> shift : (unsigned)u / div;
      o |= (q > 255u ? 255u : q) << (8 * t);
    }
    uint8_t* d = dst + (size_t)oy * orow + (size_t)ex;
    const long long left = (long long)orow - ex;
    if (left >= 4 && ((uintptr_t)d & 3) == 0) {
      *(uint32_t*)d = o;
    } else {
      const int n = left < 4 ? (int)left : 4;
      for (int t = 0; t < n; ++t) d[t] = (uint8_t)(o >> (8 * t));
    }
  }
}

template <int S, int HK>
hipError_t launch_one(const uint8_t* src, int W, int H, const int16_t* taps, int ntaps, unsigned div,
                      int shift, uint8_t* dst, hipStream_t stream) {
  using G = FilterGeom<S, HK>;
  FilterTaps f{};
  const int pad = (G::L - ntaps) / 2;   // ntaps - S is even and so is L - S
  for (int i = 0; i < ntaps; ++i) f.k[pad + i] = taps[i];
  const long long tiles_x = ((long long)W + G::TW - 1) / G::TW;
  const long long tiles_y = ((long long)H + G::TH - 1) / G::TH;
  if (tiles_x * tiles_y > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_filter_down<S, HK>), dim3((unsigned)(tiles_x * tiles_y)),
                     dim3(kFilterThreads), 0, stream, src, W, H, f, div, shift, (int)tiles_x, dst);
  return hipGetLastError();
}

template <int S>
hipError_t launch_class(const uint8_t* src, int W, int H, const int16_t* taps, int ntaps,
                        unsigned div, int shift, uint8_t* dst, hipStream_t stream) {
  const int h = (ntaps - S) / 2;
  if (h == 0) return launch_one<S, 0>(src, W, H, taps, ntaps, div, shift, dst, stream);
  if (h <= S / 2) return launch_one<S, S / 2>(src, W, H, taps, ntaps, div, shift, dst, stream);
  return launch_one<S, S>(src, W, H, taps, ntaps, div, shift, dst, stream);
}

}  // namespace

hipError_t launch_filter_down(const uint8_t* src, int W, int H, int ssaa, const int16_t* taps,
                              int ntaps, uint8_t* dst, hipStream_t stream) {
  if (!src || !dst || !taps || W <= 0 || H <= 0 || !(ssaa == 2 || ssaa == 4 || ssaa == 8) ||
      W > (1 << 28) / ssaa || H > (1 << 28) / ssaa || ntaps < ssaa || ntaps > 3 * ssaa ||
      ntaps > kFilterMaxTaps || ((ntaps - ssaa) & 1))
    return hipErrorInvalidValue;
  long long sum = 0, mag = 0;
  for (int i = 0; i < ntaps; ++i) {
    sum += taps[i];
    mag += taps[i] < 0 ? -(long long)taps[i] : taps[i];
  }
  if (sum <= 0 || mag > 2048) return hipErrorInvalidValue;
  const unsigned div = (unsigned)(sum * sum);   // <= 2^22
  int shift = -1;
  if ((div & (div - 1)) == 0)
    for (shift = 0; (1u << shift) != div; ++shift) {}
  switch (ssaa) {
    case 2: return launch_class<2>(src, W, H, taps, ntaps, div, shift, dst, stream);
    case 4: return launch_class<4>(src, W, H, taps, ntaps, div, shift, dst, stream);
    default: return launch_class<8>(src, W, H, taps, ntaps, div, shift, dst, stream);
  }
}

}  // namespace rc
