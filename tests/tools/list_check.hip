// list_check.hip — test-only device harness of the sampling family's list builders
// (rc_lists.hpp's k_aa_mark and rc_rates_bin.inc, the binning block of k_rates_render), for
// tests/test_gpu_lists.py.  Every entry takes host arrays (planes of bytes), launches the
// product's text with the launchers' own grid and block shapes (rc_sample_kernels.hip:
// launch_aa_mark's 1-D grid of tiles_x * ceil(H / 8) workgroups of 256, launch_rates_render's 2-D
// grid of 16 x 16 tiles) and copies whole buffers back.  Every device buffer is filled with a
// sentinel byte before the run (kFill) and sits between two guard blocks of the same byte, which
// are compared afterwards (-3: a guard changed; -4: the input plane changed).  No kernel here
// waits for another, and no case is meant to fault.  Compiled with the product's HIPFLAGS; the
// product library never links it.
//
// LV_WRONG = 1..8 builds a wrong variant (tests/build/liblistcheck_w<k>.so), which the suite must
// catch.  None stores outside the slots the right build may write: each only drops entries or
// overwrites slots inside a reservation.
//   1 lane 63 keeps its own pixel as its right neighbour instead of loading beyond the wave
//   2 lane 0 keeps its own pixel as its left neighbour
//   3 the window's first row is taken at y0 instead of y0 - 1
//   4 con > thr in place of >=
//   5 a row's base += popcount is dropped: slots are overwritten inside the wave's reservation
//   6 binning: the duty = 0 fallback of a last partial chunk is removed
//   7 binning: a wave's base omits the earlier waves' sums
//   8 the blue channel is unpacked from the red one's bits
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#ifndef LV_WRONG
#define LV_WRONG 0
#endif
#if LV_WRONG == 1
#define RC_MARK_RIGHT(q, x, v) (v)
#endif
#if LV_WRONG == 2
#define RC_MARK_LEFT(q, x, v) (v)
#endif
#if LV_WRONG == 3
#define RC_MARK_FIRST_ROW(y0) (y0)
#endif
#if LV_WRONG == 4
#define RC_MARK_REACHES(con, thr) ((con) > (thr))
#endif
#if LV_WRONG == 5
#define RC_MARK_ROW_DONE(base, m) (void)0
#endif
#if LV_WRONG == 6
#define RC_RATES_LAST_CHUNK(chunk, duty, nwg) (void)0
#endif
#if LV_WRONG == 7
#define RC_RATES_WAVE_BASE(base, sum) (void)0
#endif
#if LV_WRONG == 8
#define RC_MARK_SHIFT(c) (8 * ((c) & 1))
#endif

// The header's kernels are compiled here under a namespace of the harness's own (one a variant):
// under the product's names the dynamic linker binds their launch stubs to the product library's
// kernels, which the test process has loaded first, and a wrong variant would run the right code.
#pragma clang diagnostic ignored "-Wunused-function"   // rc_pixel.hpp's host helpers of the launchers
#include "rc_pixel.hpp"
#define LV_CAT2(a, b) a##b
#define LV_CAT(a, b) LV_CAT2(a, b)
#define LV_NS LV_CAT(rc_lv, LV_WRONG)
namespace LV_NS {
using namespace rc;
}
#define rc LV_NS
#include "rc_lists.hpp"
#undef rc
using namespace LV_NS;
using namespace rc;

namespace {

constexpr uint8_t kFill = 0xa5;
constexpr size_t kGuard = 256;

// a HIP error ends the entry with its (positive) code; -2: arguments refused; -3: a guard
// changed; -4: the input plane changed
#define LV_TRY(e)                             \
  do {                                        \
    const hipError_t e_ = (e);                \
    if (e_ != hipSuccess) return (int)e_;     \
  } while (0)

// a device buffer of n bytes between two guard blocks, all of it kFill; `odd` shifts the buffer
// (and nothing else) by that many bytes
struct Dev {
  uint8_t* base = nullptr;
  size_t n = 0, front = 0;
  Dev() = default;
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  ~Dev() {
    if (base) (void)hipFree(base);
  }
  hipError_t alloc(size_t bytes, size_t odd = 0) {
    n = bytes;
    front = kGuard + odd;
    hipError_t e = hipMalloc((void**)&base, front + n + kGuard);
    if (e != hipSuccess) return e;
    return hipMemset(base, kFill, front + n + kGuard);
  }
  template <class T>
  T* p(size_t i = 0) const { return (T*)(base + front) + i; }
  hipError_t put(const void* h, size_t bytes, size_t at = 0) const {
    return bytes ? hipMemcpy(base + front + at, h, bytes, hipMemcpyHostToDevice) : hipSuccess;
  }
  hipError_t get(void* h) const {
    return n ? hipMemcpy(h, base + front, n, hipMemcpyDeviceToHost) : hipSuccess;
  }
  // 0: both guards as they were; 1: not; -1: the copy failed
  int guards() const {
    std::vector<uint8_t> g(front + kGuard);
    if (hipMemcpy(g.data(), base, front, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(g.data() + front, base + front + n, kGuard, hipMemcpyDeviceToHost) != hipSuccess)
      return -1;
    for (uint8_t b : g)
      if (b != kFill) return 1;
    return 0;
  }
};

int guards_of(std::initializer_list<const Dev*> ds) {
  for (const Dev* d : ds) {
    const int g = d->base ? d->guards() : 0;
    if (g < 0) return (int)hipErrorUnknown;
    if (g > 0) return -3;
  }
  return 0;
}

// the planes of a batch go to the device in one copy: plane b at b * stride, the gaps kFill
hipError_t put_planes(const Dev& d, const uint8_t* host, int B, size_t bytes, size_t stride) {
  std::vector<uint8_t> staged(d.n, kFill);
  for (int b = 0; b < B; ++b) memcpy(staged.data() + b * stride, host + b * bytes, bytes);
  return d.put(staged.data(), d.n);
}
// 0: they still lie there as put_planes left them; 1: not; -1: the copy failed
int planes_kept(const Dev& d, const uint8_t* host, int B, size_t bytes, size_t stride) {
  std::vector<uint8_t> back(d.n);
  if (d.get(back.data()) != hipSuccess) return -1;
  for (int b = 0; b < B; ++b) {
    if (memcmp(back.data() + b * stride, host + b * bytes, bytes)) return 1;
    for (size_t i = bytes; i < stride; ++i)
      if (back[b * stride + i] != kFill) return 1;
  }
  return 0;
}

// the binning block as k_rates_render holds it: first thing, for every thread of the 2-D grid,
// with the kernel's own two LDS arrays; then the kernel returns
__global__ void __launch_bounds__(kBlock) k_bin(const uint8_t* __restrict__ rates, int W, int H,
                                                uint32_t* __restrict__ list2up,
                                                uint32_t* __restrict__ list4,
                                                uint32_t* __restrict__ list8down,
                                                unsigned* __restrict__ cnt) {
  __shared__ unsigned wsum[kBlock / 64][5];
  __shared__ unsigned wbase[3];
#include "rc_rates_bin.inc"
}

}  // namespace

extern "C" {

int lv_wrong(void) { return LV_WRONG; }
int lv_fill(void) { return kFill; }
int lv_mark_block(void) { return kMarkBlock; }
int lv_mark_rows(void) { return kMarkRows; }
int lv_rate_chunk(void) { return kRateChunk * kBlock; }
int lv_tile_w(void) { return kTileW; }
int lv_tile_h(void) { return kTileH; }

// k_aa_mark over B images of W x H (3 bytes a pixel, one after the other in img) with threshold
// thr[b], as launch_aa_mark launches it.  Image b lies at a 16-byte aligned device address, plus
// `odd` bytes.  Out, per image (P = W * H): count [1] and the whole list buffer [P].
int lv_mark(const uint8_t* img, int B, int W, int H, const int* thr, int odd, unsigned* count,
            uint32_t* list) {
  if (B < 1 || W < 1 || H < 1 || odd < 0 || odd > 15 || (long long)W * H > (1ll << 26)) return -2;
  for (int b = 0; b < B; ++b)
    if (thr[b] < 1 || thr[b] > 255) return -2;
  const size_t P = (size_t)W * H, bytes = P * 3, stride = (bytes + 15) / 16 * 16 + 16;
  Dev dI, dL, dC;
  LV_TRY(dI.alloc(B * stride, (size_t)odd));
  LV_TRY(put_planes(dI, img, B, bytes, stride));
  LV_TRY(dL.alloc(B * P * 4));
  LV_TRY(dC.alloc((size_t)B * 4));
  LV_TRY(hipMemset(dC.p<unsigned>(), 0, (size_t)B * 4));   // the counter starts at 0, as the callers'
  const unsigned tiles_x = ((unsigned)W + kMarkBlock - 1) / kMarkBlock;
  const unsigned tiles = tiles_x * (((unsigned)H + kMarkRows - 1) / kMarkRows);
  for (int b = 0; b < B; ++b)
    hipLaunchKernelGGL(k_aa_mark, dim3(tiles), dim3(kMarkBlock), 0, 0,
                       (const uint8_t*)dI.p<uint8_t>(b * stride), W, H, tiles_x, thr[b],
                       dL.p<uint32_t>(b * P), dC.p<unsigned>(b));
  LV_TRY(hipGetLastError());
  LV_TRY(hipDeviceSynchronize());
  LV_TRY(dL.get(list));
  LV_TRY(dC.get(count));
  const int kept = planes_kept(dI, img, B, bytes, stride);
  if (kept) return kept < 0 ? (int)hipErrorUnknown : -4;
  return guards_of({&dI, &dL, &dC});
}

// The binning block over B rate maps of W x H (one byte a pixel) on launch_rates_render's grid.  Out, per
// map (P = W * H): cnt [5] (zeroed before the launch, as the callers do), list4 [P] and list28
// [P], whole: the rate-2 list grows up from list28[0], the rate-8 list down from list28[P - 1].
int lv_bin(const uint8_t* rates, int B, int W, int H, unsigned* cnt, uint32_t* list4,
           uint32_t* list28) {
  if (B < 1 || W < 1 || H < 1 || (long long)W * H > (1ll << 26)) return -2;
  const size_t P = (size_t)W * H, stride = (P + 15) / 16 * 16 + 16;
  Dev dR, dL4, dL28, dC;
  LV_TRY(dR.alloc(B * stride));
  LV_TRY(put_planes(dR, rates, B, P, stride));
  LV_TRY(dL4.alloc(B * P * 4));
  LV_TRY(dL28.alloc(B * P * 4));
  LV_TRY(dC.alloc((size_t)B * 5 * 4));
  LV_TRY(hipMemset(dC.p<unsigned>(), 0, (size_t)B * 5 * 4));
  const dim3 grid((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH);
  for (int b = 0; b < B; ++b)
    hipLaunchKernelGGL(k_bin, grid, dim3(kBlock), 0, 0, (const uint8_t*)dR.p<uint8_t>(b * stride),
                       W, H, dL28.p<uint32_t>(b * P), dL4.p<uint32_t>(b * P),
                       dL28.p<uint32_t>(b * P + (P - 1)), dC.p<unsigned>((size_t)b * 5));
  LV_TRY(hipGetLastError());
  LV_TRY(hipDeviceSynchronize());
  LV_TRY(dC.get(cnt));
  LV_TRY(dL4.get(list4));
  LV_TRY(dL28.get(list28));
  const int kept = planes_kept(dR, rates, B, P, stride);
  if (kept) return kept < 0 ? (int)hipErrorUnknown : -4;
  return guards_of({&dR, &dL4, &dL28, &dC});
}

}  // extern "C"
