// rc_lists.hpp — the list builders of the sampling family: k_aa_mark, the 3 x 3
// contrast test that lists the edge pixels, and the constant and hooks of rc_rates_bin.inc, the
// block of k_rates_render that bins a rate map into one list per factor.  rc_sample_kernels.hip's
// launchers and kernels use them; the plane-by-plane test harness (tests/tools/list_check.hip)
// includes them too, so both run the same text.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rc_pixel.hpp"

namespace rc {

// Eight places of the text below, by role, each used in one statement.  Only the test harness's wrong
// variants (list_check.hip, LV_WRONG) define them otherwise, before this header; the product never
// does.  Expressions and their arguments are parenthesised and statements are single expressions
// or do-while blocks, so a hook means the same wherever it stands.
#ifndef RC_MARK_LEFT
#define RC_MARK_LEFT(q, x, v) (mark_load((q) + (size_t)((x) - 1u) * 3))    // lane 0: the pixel before the wave
#endif
#ifndef RC_MARK_RIGHT
#define RC_MARK_RIGHT(q, x, v) (mark_load((q) + (size_t)((x) + 1u) * 3))   // lane 63: the pixel after the wave
#endif
#ifndef RC_MARK_SHIFT
#define RC_MARK_SHIFT(c) (8 * (c))               // mark_row: channel c of a packed pixel
#endif
#ifndef RC_MARK_FIRST_ROW
#define RC_MARK_FIRST_ROW(y0) ((y0) > 0u ? (y0) - 1u : 0u)   // k_aa_mark: the row above the tile, clamped
#endif
#ifndef RC_MARK_REACHES
#define RC_MARK_REACHES(con, thr) ((con) >= (thr))   // k_aa_mark: the contrast reaches the threshold
#endif
#ifndef RC_MARK_ROW_DONE
#define RC_MARK_ROW_DONE(base, m) ((base) += (unsigned)__popcll(m))   // k_aa_mark: the next row's first slot
#endif
#ifndef RC_RATES_LAST_CHUNK   // binning: a last partial chunk whose turn is no workgroup's goes to its first
#define RC_RATES_LAST_CHUNK(chunk, duty, nwg) \
  do {                                        \
    if ((chunk) * kRateChunk + (duty) >= (nwg)) (duty) = 0; \
  } while (0)
#endif
#ifndef RC_RATES_WAVE_BASE
#define RC_RATES_WAVE_BASE(base, sum) ((base) += (sum))   // binning: the earlier waves' flagged pixels
#endif

// k_aa_mark: one lane per pixel.  A workgroup is four waves side by side, each taking 64 adjacent
// columns of kMarkRows rows of tile (tx, ty) (the tile index is divided once per workgroup, in
// scalars).  A wave walks down its rows with a rolling window of three: of every row it loads
// each lane's own pixel once (packed R | G << 8 | B << 16), takes the left and right neighbours
// from the adjacent lanes, and only lanes 0 and 63 load the pixel beyond the wave, so a pixel
// costs 3 * (kMarkRows + 2) / kMarkRows byte loads instead of 27.  Coordinates are clamped to
// the image: a clamped neighbour is a pixel of the window taken twice, which changes neither max
// nor min.  List slots are reserved per wave: a ballot of the flagged lanes of every row, one
// atomicAdd of their popcounts' sum by lane 0, and each flagged lane writes at base + the flagged
// pixels of the rows above + the popcount of the flagged lanes below it in its row.  Every lane
// of a wave reaches the shuffles and the ballots (lanes past the image load and flag nothing;
// skipping a row past the image is uniform).  The list's order follows
// the atomics' arrival and is not deterministic; no output byte depends on it.
constexpr int kMarkBlock = 256, kMarkRows = 8;
struct MarkRow {
  int lo[3], hi[3];   // per channel, over the pixel and its two neighbours in the row
};
__device__ __forceinline__ unsigned mark_load(const uint8_t* __restrict__ q) {
  return (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
}
// in: x < W.  y < H.  Called by every lane of the wave.
__device__ __forceinline__ MarkRow mark_row(const uint8_t* __restrict__ img, unsigned W, unsigned x,
                                            unsigned y, int lane, bool in) {
  const uint8_t* q = img + (size_t)y * W * 3;
  const unsigned v = in ? mark_load(q + (size_t)x * 3) : 0u;
  unsigned l = __shfl_up(v, 1, 64), r = __shfl_down(v, 1, 64);
  if (in) {
    if (x == 0u) l = v;
    else if (lane == 0) l = RC_MARK_LEFT(q, x, v);
    if (x + 1u >= W) r = v;
    else if (lane == 63) r = RC_MARK_RIGHT(q, x, v);
  }
  MarkRow m;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int a = (int)((v >> RC_MARK_SHIFT(c)) & 255u), b = (int)((l >> RC_MARK_SHIFT(c)) & 255u),
              d = (int)((r >> RC_MARK_SHIFT(c)) & 255u);
    const int lo = a < b ? a : b, hi = a > b ? a : b;
    m.lo[c] = lo < d ? lo : d;
    m.hi[c] = hi > d ? hi : d;
  }
  return m;
}
__global__ void __launch_bounds__(kMarkBlock) k_aa_mark(const uint8_t* __restrict__ img, int W,
                                                        int H, unsigned tiles_x, int thr,
                                                        uint32_t* __restrict__ list,
                                                        unsigned* __restrict__ count) {
  const unsigned ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
  const int lane = threadIdx.x & 63;
  const unsigned x = tx * kMarkBlock + threadIdx.x;   // tx * 256 < W + 256 <= 2^31 + 255
  const unsigned y0 = ty * kMarkRows, w = (unsigned)W, h = (unsigned)H;   // y0 < H
  const bool in = x < w;
  MarkRow p = mark_row(img, w, x, RC_MARK_FIRST_ROW(y0), lane, in);
  MarkRow c = mark_row(img, w, x, y0, lane, in);
  unsigned long long flagged[kMarkRows];   // per row, the ballot of its flagged lanes (uniform)
  unsigned total = 0u;
#pragma unroll
  for (int k = 0; k < kMarkRows; ++k) {
    const unsigned y = y0 + (unsigned)k;
    flagged[k] = 0ull;
    if (y >= h) continue;   // uniform
    const MarkRow n = mark_row(img, w, x, y + 1u < h ? y + 1u : y, lane, in);
    int con = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      int lo = p.lo[ch] < c.lo[ch] ? p.lo[ch] : c.lo[ch];
      int hi = p.hi[ch] > c.hi[ch] ? p.hi[ch] : c.hi[ch];
      lo = n.lo[ch] < lo ? n.lo[ch] : lo;
      hi = n.hi[ch] > hi ? n.hi[ch] : hi;
      con = hi - lo > con ? hi - lo : con;
    }
    flagged[k] = __ballot(in && RC_MARK_REACHES(con, thr));
    total += (unsigned)__popcll(flagged[k]);
    p = c;
    c = n;
  }
  // one reservation per wave for all its rows: the atomics all hit one address
  unsigned base = 0u;
  if (lane == 0 && total) base = atomicAdd(count, total);
  base = __shfl(base, 0, 64);
#pragma unroll
  for (int k = 0; k < kMarkRows; ++k) {
    const unsigned long long m = flagged[k];
    if ((m >> lane) & 1ull)   // y*W + x < W*H < 2^32 (launch_aa_mark)
      list[base + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] =
          (uint32_t)((size_t)(y0 + (unsigned)k) * w + x);
    RC_MARK_ROW_DONE(base, m);
  }
}

// The binning block of k_rates_render is rc_rates_bin.inc, text that the kernel and the test
// harness include in a kernel body; its constant and its two hooks are here.
constexpr int kRateChunk = 8;   // tiles' worth of pixels per binning workgroup (a power of two)

}  // namespace rc
