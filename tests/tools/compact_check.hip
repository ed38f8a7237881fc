// compact_check.hip — test-only device harness of the stage between phase A and the resolver
// (rc_compact.hpp: writer_may_key, k_row_stats, k_row_scan, k_row_compact, k_seg_order and the row
// shards' k_shard_pack, k_shard_rows, k_shard_unpack, k_deinterleave), for
// tests/test_gpu_compact.py.  Every entry takes host arrays (class maps, segment tables), launches
// the product's kernels with the launchers' own grid and block shapes (rc_kernels.hip:
// launch_parity, launch_shard_local, launch_shard_resolve, launch_deinterleave) and copies whole
// buffers back.  Every device buffer is filled with a sentinel byte before the run (kFill; the
// writer carries with kPoison) and sits between two guard blocks of the same byte, which are
// compared afterwards (-3: a guard changed).  No kernel here waits for another, and no case is
// meant to fault.  Compiled with the product's HIPFLAGS; the product library never links it.
//
// CV_WRONG = 1..5 builds a wrong variant (tests/build/libcompactcheck_w<k>.so), which the suite
// must catch: 1 a lane with no writer before it in its 64-lane group takes -1 instead of the
// carried last writer; 2 k_row_scan drops the last writer at a scan chunk (2 048 rows); 3
// k_row_compact forgets the last DEP pixel at an LDS chunk (4 096 pixels); 4 the segment order's
// length bucket is taken from len + 1; 5 writer_may_key looks at a 16-lane fragment.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#ifndef CV_WRONG
#define CV_WRONG 0
#endif
#if CV_WRONG == 1
#define RC_GROUP_CARRY_W(lw) -1ll
#endif
#if CV_WRONG == 2
#define RC_CHUNK_CARRY_W(w) -1ll
#endif
#if CV_WRONG == 3
#define RC_ROW_CHUNK_END(ld) __syncthreads(); ld = -1
#endif
#if CV_WRONG == 4
#define RC_SEG_BUCKET(len) (len + 1) >> 5
#endif
#if CV_WRONG == 5
#define RC_WKEY_FRAG 15
#endif

// The header's kernels are compiled here under a namespace of the harness's own (one a variant):
// under the product's names the dynamic linker binds their launch stubs to the product library's
// kernels, which the test process has loaded first, and a wrong variant would run the right code.
#include "rc_device.hpp"
#include "rc_kernels.h"
#define CV_CAT2(a, b) a##b
#define CV_CAT(a, b) CV_CAT2(a, b)
#define CV_NS CV_CAT(rc_cv, CV_WRONG)
namespace CV_NS {
using namespace rc;
}
#define rc CV_NS
#include "rc_compact.hpp"
#undef rc
using namespace CV_NS;
#pragma clang diagnostic ignored "-Wunused-function"   // rc_pixel.hpp's host helpers of the launchers
#include "rc_pixel.hpp"

using namespace rc;

namespace {

constexpr uint8_t kFill = 0xa5, kPoison = 0xee;
constexpr size_t kGuard = 256;
constexpr int kThinPad = 0x7777;   // pad / pad2 as the harness's phase A leaves them

// a HIP error ends the entry with its (positive) code; -2: arguments refused; -3: a guard changed
#define CV_TRY(e)                             \
  do {                                        \
    const hipError_t e_ = (e);                \
    if (e_ != hipSuccess) return (int)e_;     \
  } while (0)

// a device buffer of n bytes between two guard blocks, all of it `fill`; `odd` shifts the buffer
// (and nothing else) by that many bytes
struct Dev {
  uint8_t* base = nullptr;
  size_t n = 0, front = 0;
  uint8_t fill = kFill;
  Dev() = default;
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  ~Dev() {
    if (base) (void)hipFree(base);
  }
  hipError_t alloc(size_t bytes, uint8_t f = kFill, size_t odd = 0) {
    n = bytes;
    front = kGuard + odd;
    fill = f;
    hipError_t e = hipMalloc((void**)&base, front + n + kGuard);
    if (e != hipSuccess) return e;
    return hipMemset(base, fill, front + n + kGuard);
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
      if (b != fill) return 1;
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

// the tags of the shard entry: every word of a DEP line and of a writer's carry names its image
// pixel and its own place
__device__ __forceinline__ DepLine tag_line(int p) {
  DepLine l;
  int* w = (int*)&l;
  for (int k = 0; k < 16; ++k) w[k] = p * 16 + k;
  l.r.pad = kThinPad;
  l.r.pad2 = kThinPad;
  return l;
}
__device__ __forceinline__ float4 tag_carry(int p) {
  return make_float4(__int_as_float(0x40000000 | (p * 4)), __int_as_float(0x40000000 | (p * 4 + 1)),
                     __int_as_float(0x40000000 | (p * 4 + 2)), __int_as_float(0x40000000 | (p * 4 + 3)));
}

// writer_may_key under phase A's own lane layout (k_phase_a: tile_pixel, xcd_tile, the ballots
// taken by the lanes with x < W && y < nrows only): one byte a writer, 1 = it stores its carry
__global__ void __launch_bounds__(kBlock) k_wkey(const uint8_t* __restrict__ cls, int W, int nrows,
                                                 uint8_t* __restrict__ out) {
  int lx, ly;
  tile_pixel(lx, ly);
  int bx, by;
  xcd_tile(bx, by);
  const int x = bx * kTileW + lx, y = by * kTileH + ly;
  if (x < W && y < nrows) {
    const size_t p = (size_t)y * W + x;
    const uint8_t c = cls[p];
    const unsigned long long mw = __ballot(c == kClsWriter);
    const unsigned long long md = __ballot(c == kClsDep);
    if (c == kClsWriter) out[p] = writer_may_key(mw, md) ? 1 : 0;
  }
}

// phase A's stores of a rank, with tags for records and carries: k_phase_a's addressing (local
// pixel for the class map, row pitch rpitch for the lines and carries) and its key-writer filter
__global__ void __launch_bounds__(kBlock) k_tag_phase_a(const uint8_t* __restrict__ cls, int W,
                                                        int row0, int row_step, int nrows,
                                                        float4* __restrict__ wcarry,
                                                        DepLine* __restrict__ deprec, int rpitch,
                                                        uint8_t* __restrict__ stored) {
  int lx, ly;
  tile_pixel(lx, ly);
  int bx, by;
  xcd_tile(bx, by);
  const int x = bx * kTileW + lx, y = by * kTileH + ly;
  if (x < W && y < nrows) {
    const size_t p = (size_t)y * W + x;
    const uint8_t c = cls[p];
    const size_t pr = (size_t)y * rpitch + x;
    const int img = (row0 + y * row_step) * W + x;
    if (c == kClsDep) deprec[pr] = tag_line(img);
    const unsigned long long mw = __ballot(c == kClsWriter);
    const unsigned long long md = __ballot(c == kClsDep);
    if (c == kClsWriter) {
      const bool k = writer_may_key(mw, md);
      stored[img] = k ? 1 : 0;
      if (k) wcarry[pr] = tag_carry(img);
    }
  }
}

dim3 tile_grid(int W, int nrows) {
  return dim3((W + kTileW - 1) / kTileW, (nrows + kTileH - 1) / kTileH);
}

}  // namespace

extern "C" {

int cv_wrong(void) { return CV_WRONG; }
int cv_fill(void) { return kFill; }
int cv_poison(void) { return kPoison; }
int cv_scan_chunk(void) { return kScanBlock * kScanRows; }
int cv_row_chunk(void) { return kRowChunk; }
int cv_seg_order_max(void) { return kSegOrderMax; }

// Lone compaction: B class maps of W x H through k_row_stats, k_row_scan, k_row_compact and
// k_seg_order as launch_parity strings them, one sync after the last.  Map b lies at a 16-byte
// aligned device address, plus one byte when odd.  zero_words < 0: k_row_stats gets no `zero`
// (launch_shard_local's form) and k_seg_order clears the batch arrays; else it clears zero_words
// 16-byte words, zero2_ints ints and counters[0..16), and k_seg_order leaves the batch arrays.
// Out, per map (P = W * H): rs [H] RowStats, row_off / row_soff / prevw / prevd [H], dep_pix /
// seg_start / seg_key / seg_order [P + 1], counters [17], zero [4 * (max(zero_words, 0) + 1)]
// words, zero2 [max(zero2_ints, 0) + 1], batch [3][(P + 63) / 64 + 1].
int cv_lone(const uint8_t* cls, int B, int W, int H, int odd, int zero_words, int zero2_ints,
            int block_min, int block_cap, void* rs, int* row_off, int* row_soff, long long* prevw,
            long long* prevd, long long* dep_pix, int* seg_start, long long* seg_key,
            int* seg_order, int* counters, unsigned* zero, int* zero2, int* batch) {
  if (B < 1 || W < 1 || H < 1 || (long long)W * H > (1ll << 27) || zero2_ints < 0) return -2;
  const size_t P = (size_t)W * H, P1 = P + 1, mstride = (P + 15) / 16 * 16 + 16;
  const bool zr = zero_words >= 0;
  const size_t zw = (size_t)(zr ? zero_words : 0) + 1, z2 = (size_t)zero2_ints + 1;
  const size_t nb1 = (P + 63) / 64 + 1;
  Dev dC, dRs, dOff, dSoff, dPw, dPd, dDep, dSs, dSk, dOrd, dCnt, dZ, dZ2, dBt;
  CV_TRY(dC.alloc(B * mstride, kFill, odd ? 1 : 0));
  for (int b = 0; b < B; ++b) CV_TRY(dC.put(cls + b * P, P, b * mstride));
  CV_TRY(dRs.alloc(B * H * sizeof(RowStats)));
  CV_TRY(dOff.alloc(B * (size_t)H * 4));
  CV_TRY(dSoff.alloc(B * (size_t)H * 4));
  CV_TRY(dPw.alloc(B * (size_t)H * 8));
  CV_TRY(dPd.alloc(B * (size_t)H * 8));
  CV_TRY(dDep.alloc(B * P1 * 8));
  CV_TRY(dSs.alloc(B * P1 * 4));
  CV_TRY(dSk.alloc(B * P1 * 8));
  CV_TRY(dOrd.alloc(B * P1 * 4));
  CV_TRY(dCnt.alloc(B * 17 * 4));
  CV_TRY(dZ.alloc(B * zw * 16));
  CV_TRY(dZ2.alloc(B * z2 * 4));
  CV_TRY(dBt.alloc(B * 3 * nb1 * 4));
  const int row_blocks = (H + kRowWaves - 1) / kRowWaves;
  for (int b = 0; b < B; ++b) {
    const uint8_t* c = dC.p<uint8_t>(b * mstride);
    int* cn = dCnt.p<int>((size_t)b * 17);
    int* bt = dBt.p<int>(b * 3 * nb1);
    hipLaunchKernelGGL(k_row_stats, dim3(row_blocks), dim3(256), 0, 0, c, W, H,
                       dRs.p<RowStats>((size_t)b * H), zr ? cn : nullptr,
                       zr ? dZ.p<uint4>(b * zw) : nullptr, zr ? zero_words : 0,
                       zr ? dZ2.p<int>(b * z2) : nullptr, zr ? zero2_ints : 0);
    hipLaunchKernelGGL(k_row_scan, dim3(1), dim3(kScanBlock), 0, 0, H,
                       (const RowStats*)dRs.p<RowStats>((size_t)b * H), dOff.p<int>((size_t)b * H),
                       dSoff.p<int>((size_t)b * H), dPw.p<long long>((size_t)b * H),
                       dPd.p<long long>((size_t)b * H), cn);
    hipLaunchKernelGGL(k_row_compact, dim3(row_blocks), dim3(256), 0, 0, c, W, H,
                       (const int*)dOff.p<int>((size_t)b * H), (const int*)dSoff.p<int>((size_t)b * H),
                       (const long long*)dPw.p<long long>((size_t)b * H),
                       (const long long*)dPd.p<long long>((size_t)b * H), dDep.p<long long>(b * P1),
                       dSs.p<int>(b * P1), dSk.p<long long>(b * P1));
    hipLaunchKernelGGL(k_seg_order, dim3(1), dim3(kScanBlock), 0, 0, (const int*)dSs.p<int>(b * P1),
                       cn, dOrd.p<int>(b * P1), bt, bt + nb1, bt + 2 * nb1, block_min, block_cap,
                       zr ? 0 : 1);
  }
  CV_TRY(hipGetLastError());
  CV_TRY(hipDeviceSynchronize());
  CV_TRY(dRs.get(rs));
  CV_TRY(dOff.get(row_off));
  CV_TRY(dSoff.get(row_soff));
  CV_TRY(dPw.get(prevw));
  CV_TRY(dPd.get(prevd));
  CV_TRY(dDep.get(dep_pix));
  CV_TRY(dSs.get(seg_start));
  CV_TRY(dSk.get(seg_key));
  CV_TRY(dOrd.get(seg_order));
  CV_TRY(dCnt.get(counters));
  CV_TRY(dZ.get(zero));
  CV_TRY(dZ2.get(zero2));
  CV_TRY(dBt.get(batch));
  return guards_of({&dC, &dRs, &dOff, &dSoff, &dPw, &dPd, &dDep, &dSs, &dSk, &dOrd, &dCnt, &dZ,
                    &dZ2, &dBt});
}

// k_seg_order alone on a segment table: seg_start [nseg], counters[0] = nseg, counters[2] =
// ndep, the other counters the sentinel.  Out: order [cap], counters [17], batch [3][(ndep + 63)
// / 64 + 1].  The kernel writes order[0 .. nseg) when nseg <= kSegOrderMax: cap >= that.
int cv_order(const int* seg_start, int nseg, int ndep, int block_min, int block_cap,
             int zero_batches, int cap, int* order, int* counters, int* batch) {
  if (nseg < 0 || ndep < 0 || cap < 1 || (nseg <= kSegOrderMax && cap < nseg)) return -2;
  const size_t nb1 = ((size_t)ndep + 63) / 64 + 1;
  Dev dSs, dOrd, dCnt, dBt;
  CV_TRY(dSs.alloc((size_t)(nseg > 0 ? nseg : 1) * 4));
  CV_TRY(dSs.put(seg_start, (size_t)nseg * 4));
  CV_TRY(dOrd.alloc((size_t)cap * 4));
  CV_TRY(dCnt.alloc(17 * 4));
  const int head[3] = {nseg, (int)(0x01010101u * kFill), ndep};
  CV_TRY(dCnt.put(head, sizeof head));
  CV_TRY(dBt.alloc(3 * nb1 * 4));
  int* bt = dBt.p<int>();
  hipLaunchKernelGGL(k_seg_order, dim3(1), dim3(kScanBlock), 0, 0, (const int*)dSs.p<int>(),
                     dCnt.p<int>(), dOrd.p<int>(), bt, bt + nb1, bt + 2 * nb1, block_min, block_cap,
                     zero_batches);
  CV_TRY(hipGetLastError());
  CV_TRY(hipDeviceSynchronize());
  CV_TRY(dOrd.get(order));
  CV_TRY(dCnt.get(counters));
  CV_TRY(dBt.get(batch));
  return guards_of({&dSs, &dOrd, &dCnt, &dBt});
}

// writer_may_key over a W x nrows class map under phase A's lane layout.  Out: one byte a pixel,
// 1 / 0 for a writer that stores / does not store its carry, the sentinel elsewhere.
int cv_wkey(const uint8_t* cls, int W, int nrows, uint8_t* out) {
  if (W < 1 || nrows < 1) return -2;
  const size_t P = (size_t)W * nrows;
  Dev dC, dO;
  CV_TRY(dC.alloc(P));
  CV_TRY(dC.put(cls, P));
  CV_TRY(dO.alloc(P));
  hipLaunchKernelGGL(k_wkey, tile_grid(W, nrows), dim3(kBlock), 0, 0, (const uint8_t*)dC.p<uint8_t>(),
                     W, nrows, dO.p<uint8_t>());
  CV_TRY(hipGetLastError());
  CV_TRY(hipDeviceSynchronize());
  CV_TRY(dO.get(out));
  return guards_of({&dC, &dO});
}

// Row shards: the W x H class map split over G ranks (row y -> rank y % G).  Per rank
// launch_shard_local's sequence (the harness's tagging phase A, k_row_stats, k_row_scan,
// k_shard_pack; thin: rank 0 writes its lines and carries at their image pixels and packs thin
// entries), the gather as rc_shard.hip lays it out (rows [G][rmax]; entries concatenated at
// ShardOffs, exact counts when bound < 0, else every rank's first `bound` entries at g * bound),
// then launch_shard_resolve's k_shard_rows, k_row_scan, k_shard_unpack and k_seg_order at the
// root.  Out (P = W * H): the root's
// rs / row_off / row_soff / prevw / prevd [H], dep_pix / seg_start / seg_key / seg_order [P + 1],
// counters [17], deprec [P + 1][16] words, wcarry [P + 1][4] words, stored [P] (phase A's
// key-writer filter by image pixel), nloc [G] (each rank's DEP count).
int cv_shard(const uint8_t* cls, int W, int H, int G, int thin, int bound, int block_min,
             int block_cap, void* rs, int* row_off, int* row_soff, long long* prevw,
             long long* prevd, long long* dep_pix, int* seg_start, long long* seg_key,
             int* seg_order, int* counters, int* deprec, int* wcarry, uint8_t* stored, int* nloc) {
  if (W < 1 || H < 1 || G < 1 || G > kMaxShards || (long long)W * H > (1 << 22)) return -2;
  const size_t P = (size_t)W * H, P1 = P + 1;
  const int rmax = (H + G - 1) / G;
  struct Rank {
    int nrows = 0;
    Dev cls, wc, rec, rs, off, soff, pw, pd, cnt, dep, ent, rows;
  };
  std::vector<Rank> rk(G);
  Dev dWc, dRec, dStored;
  CV_TRY(dWc.alloc(P1 * sizeof(float4), kPoison));
  CV_TRY(dRec.alloc(P1 * sizeof(DepLine)));
  CV_TRY(dStored.alloc(P));
  std::vector<uint8_t> loc;
  for (int g = 0; g < G; ++g) {
    Rank& r = rk[g];
    r.nrows = g < H ? (H - g + G - 1) / G : 0;
    const size_t n = (size_t)r.nrows * W;
    loc.resize(n);
    for (int y = 0; y < r.nrows; ++y) memcpy(loc.data() + (size_t)y * W, cls + (size_t)(g + y * G) * W, W);
    CV_TRY(r.cls.alloc(n));
    CV_TRY(r.cls.put(loc.data(), n));
    CV_TRY(r.wc.alloc(n * sizeof(float4), kPoison));
    CV_TRY(r.rec.alloc(n * sizeof(DepLine)));
    CV_TRY(r.rs.alloc(r.nrows * sizeof(RowStats)));
    CV_TRY(r.off.alloc((size_t)r.nrows * 4));
    CV_TRY(r.soff.alloc((size_t)r.nrows * 4));
    CV_TRY(r.pw.alloc((size_t)r.nrows * 8));
    CV_TRY(r.pd.alloc((size_t)r.nrows * 8));
    CV_TRY(r.cnt.alloc(17 * 4));
    CV_TRY(hipMemset(r.cnt.p<int>(), 0, 16 * 4));
    CV_TRY(r.dep.alloc((n + 1) * 8));
    CV_TRY(r.ent.alloc((n + 1) * sizeof(ShardEntry)));
    CV_TRY(r.rows.alloc((size_t)r.nrows * sizeof(RowShard)));
    if (r.nrows <= 0) continue;
    const bool th = thin && g == 0;
    hipLaunchKernelGGL(k_tag_phase_a, tile_grid(W, r.nrows), dim3(kBlock), 0, 0,
                       (const uint8_t*)r.cls.p<uint8_t>(), W, g, G, r.nrows,
                       th ? dWc.p<float4>((size_t)g * W) : r.wc.p<float4>(),
                       th ? dRec.p<DepLine>((size_t)g * W) : r.rec.p<DepLine>(), th ? G * W : W,
                       dStored.p<uint8_t>());
    const int row_blocks = (r.nrows + kRowWaves - 1) / kRowWaves;
    hipLaunchKernelGGL(k_row_stats, dim3(row_blocks), dim3(256), 0, 0, (const uint8_t*)r.cls.p<uint8_t>(),
                       W, r.nrows, r.rs.p<RowStats>(), nullptr, nullptr, 0, nullptr, 0);
    hipLaunchKernelGGL(k_row_scan, dim3(1), dim3(kScanBlock), 0, 0, r.nrows,
                       (const RowStats*)r.rs.p<RowStats>(), r.off.p<int>(), r.soff.p<int>(),
                       r.pw.p<long long>(), r.pd.p<long long>(), r.cnt.p<int>());
    hipLaunchKernelGGL(k_shard_pack, dim3(row_blocks), dim3(256), 0, 0, (const uint8_t*)r.cls.p<uint8_t>(),
                       (const float4*)(th ? dWc.p<float4>() : r.wc.p<float4>()),
                       (const DepLine*)r.rec.p<DepLine>(), W, g, G, r.nrows, (const int*)r.off.p<int>(),
                       r.dep.p<long long>(), r.ent.p<ShardEntry>(), r.rows.p<RowShard>(), th ? 1 : 0);
  }
  CV_TRY(hipGetLastError());
  CV_TRY(hipDeviceSynchronize());   // the counts, as the exact exchange waits for them
  std::vector<size_t> cnt(G, 0);
  ShardOffs o{};
  size_t total = 0;
  for (int g = 0; g < G; ++g) {
    int c[3];
    CV_TRY(hipMemcpy(c, rk[g].cnt.p<int>(), sizeof c, hipMemcpyDeviceToHost));
    nloc[g] = c[2];
    if (c[2] < 0 || (size_t)c[2] > (size_t)rk[g].nrows * W) return -4;
    cnt[g] = bound >= 0 ? (size_t)bound : (size_t)c[2];
    if (cnt[g] > (size_t)rmax * W) cnt[g] = (size_t)rmax * W;
    o.off[g] = (long long)total;
    total += cnt[g];
  }
  const size_t cap = total > (size_t)G * rmax * W ? total : (size_t)G * rmax * W;
  Dev dEnt, dRows, dRs, dOff, dSoff, dPw, dPd, dDep, dSs, dSk, dOrd, dCnt, dBt;
  CV_TRY(dEnt.alloc((cap + 1) * sizeof(ShardEntry)));
  CV_TRY(dRows.alloc((size_t)G * rmax * sizeof(RowShard)));
  for (int g = 0; g < G; ++g) {
    CV_TRY(hipMemcpy(dRows.p<RowShard>((size_t)g * rmax), rk[g].rows.p<RowShard>(),
                     (size_t)rk[g].nrows * sizeof(RowShard), hipMemcpyDeviceToDevice));
    if (thin && g == 0) continue;   // the root's own list is read in place
    const size_t take = (size_t)nloc[g] < cnt[g] ? (size_t)nloc[g] : cnt[g];
    CV_TRY(hipMemcpy(dEnt.p<ShardEntry>((size_t)o.off[g]), rk[g].ent.p<ShardEntry>(),
                     take * sizeof(ShardEntry), hipMemcpyDeviceToDevice));
  }
  const size_t nb1 = (P + 63) / 64 + 1;
  CV_TRY(dRs.alloc(H * sizeof(RowStats)));
  CV_TRY(dOff.alloc((size_t)H * 4));
  CV_TRY(dSoff.alloc((size_t)H * 4));
  CV_TRY(dPw.alloc((size_t)H * 8));
  CV_TRY(dPd.alloc((size_t)H * 8));
  CV_TRY(dDep.alloc(P1 * 8));
  CV_TRY(dSs.alloc(P1 * 4));
  CV_TRY(dSk.alloc(P1 * 8));
  CV_TRY(dOrd.alloc(P1 * 4));
  CV_TRY(dCnt.alloc(17 * 4));
  CV_TRY(hipMemset(dCnt.p<int>(), 0, 16 * 4));
  CV_TRY(dBt.alloc(3 * nb1 * 4));
  int* bt = dBt.p<int>();
  const RowShard* rsall = dRows.p<RowShard>();
  hipLaunchKernelGGL(k_shard_rows, dim3((H + 255) / 256), dim3(256), 0, 0, rsall, G, rmax, H,
                     dRs.p<RowStats>());
  hipLaunchKernelGGL(k_row_scan, dim3(1), dim3(kScanBlock), 0, 0, H, (const RowStats*)dRs.p<RowStats>(),
                     dOff.p<int>(), dSoff.p<int>(), dPw.p<long long>(), dPd.p<long long>(),
                     dCnt.p<int>());
  const int row_blocks = (H + kRowWaves - 1) / kRowWaves;
  hipLaunchKernelGGL(k_shard_unpack, dim3(row_blocks), dim3(256), 0, 0, rsall,
                     (const ShardEntry*)dEnt.p<ShardEntry>(),
                     (const ShardEntry*)(thin ? rk[0].ent.p<ShardEntry>() : nullptr), o, G, rmax, W, H,
                     (const int*)dOff.p<int>(), (const int*)dSoff.p<int>(),
                     (const long long*)dPw.p<long long>(), (const long long*)dPd.p<long long>(),
                     dRec.p<DepLine>(), dDep.p<long long>(), dSs.p<int>(), dSk.p<long long>(),
                     dWc.p<float4>(), bound >= 0 ? bound : 0x7fffffff, thin ? 1 : 0);
  // (after a truncated exchange the segment table has slots nobody wrote, which k_seg_order reads
  // as the product's does: any length lands in a bucket, so the order is still a permutation)
  hipLaunchKernelGGL(k_seg_order, dim3(1), dim3(kScanBlock), 0, 0, (const int*)dSs.p<int>(),
                     dCnt.p<int>(), dOrd.p<int>(), bt, bt + nb1, bt + 2 * nb1, block_min, block_cap, 1);
  CV_TRY(hipGetLastError());
  CV_TRY(hipDeviceSynchronize());
  CV_TRY(dRs.get(rs));
  CV_TRY(dOff.get(row_off));
  CV_TRY(dSoff.get(row_soff));
  CV_TRY(dPw.get(prevw));
  CV_TRY(dPd.get(prevd));
  CV_TRY(dDep.get(dep_pix));
  CV_TRY(dSs.get(seg_start));
  CV_TRY(dSk.get(seg_key));
  CV_TRY(dOrd.get(seg_order));
  CV_TRY(dCnt.get(counters));
  CV_TRY(dRec.get(deprec));
  CV_TRY(dWc.get(wcarry));
  CV_TRY(dStored.get(stored));
  for (int g = 0; g < G; ++g) {
    Rank& r = rk[g];
    const int e = guards_of({&r.cls, &r.wc, &r.rec, &r.rs, &r.off, &r.soff, &r.pw, &r.pd, &r.cnt,
                             &r.dep, &r.ent, &r.rows});
    if (e) return e;
  }
  return guards_of({&dWc, &dRec, &dStored, &dEnt, &dRows, &dRs, &dOff, &dSoff, &dPw, &dPd, &dDep,
                    &dSs, &dSk, &dOrd, &dCnt, &dBt});
}

// k_deinterleave as launch_deinterleave launches it: gathered [G][rmax][W * 3] row blocks; with
// block0, rank 0's block is handed over apart and its place in `gathered` holds the sentinel.
int cv_deinterleave(const uint8_t* gathered, int G, int rmax, int W, int H, int block0,
                    uint8_t* img) {
  if (G < 1 || W < 1 || H < 1 || rmax < (H + G - 1) / G) return -2;
  const size_t rb = (size_t)W * 3, blk = (size_t)rmax * rb;
  Dev dG, dB, dI;
  CV_TRY(dG.alloc((size_t)G * blk));
  CV_TRY(dG.put(gathered + (block0 ? blk : 0), (size_t)G * blk - (block0 ? blk : 0), block0 ? blk : 0));
  CV_TRY(dB.alloc(blk));
  if (block0) CV_TRY(dB.put(gathered, blk));
  CV_TRY(dI.alloc((size_t)H * rb));
  hipLaunchKernelGGL(k_deinterleave, dim3(H), dim3(256), 0, 0, (const uint8_t*)dG.p<uint8_t>(),
                     (const uint8_t*)(block0 ? dB.p<uint8_t>() : nullptr), G, rmax, W, H,
                     dI.p<uint8_t>());
  CV_TRY(hipGetLastError());
  CV_TRY(hipDeviceSynchronize());
  CV_TRY(dI.get(img));
  return guards_of({&dG, &dB, &dI});
}

}  // extern "C"
