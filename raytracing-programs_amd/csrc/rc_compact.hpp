// rc_compact.hpp — between phase A and the resolver: phase A's key-writer filter,
// the scan-order DEP compaction (class map -> DEP list, segment table, segment order) and the row
// shards' twins of it.  rc_kernels.hip's launchers string these kernels together; the class-map
// test harness (tests/tools/compact_check.hip) includes them too, so both run the same text.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rc_device.hpp"
#include "rc_kernels.h"

namespace rc {

// Five places of the text below, by role.  Only the test harness's wrong variants
// (compact_check.hip, CV_WRONG) define them otherwise, before this header; the product never does.
#ifndef RC_WKEY_FRAG
#define RC_WKEY_FRAG 7                 // writer_may_key: the lane's row fragment is lanes l .. l | 7
#endif
#ifndef RC_GROUP_CARRY_W
#define RC_GROUP_CARRY_W(lw) lw        // no writer before the lane in its 64-lane group: the carried one
#endif
#ifndef RC_CHUNK_CARRY_W
#define RC_CHUNK_CARRY_W(w) w          // k_row_scan: the last writer of the chunks so far
#endif
#ifndef RC_ROW_CHUNK_END
#define RC_ROW_CHUNK_END(ld) __syncthreads()   // k_row_compact: the last DEP pixel crosses an LDS chunk as it is
#endif
#ifndef RC_SEG_BUCKET
#define RC_SEG_BUCKET(len) len >> 5    // k_seg_order: 32-entry length buckets
#endif

// ---------------------------------------------------------- phase A's key writers --
// A writer's carry-out is read only as a segment key: the last writer before a DEP pixel in
// scan order (seg_init_carry), and by the row shards the last writer before a DEP pixel in its
// row or the last writer of a row (k_shard_pack).  Inside the lane's 8-pixel row fragment of
// the wave tile (lane = 8 * row + x), a writer followed by another writer with no DEP pixel
// between them is neither, so phase A stores only the others: a writer with no later writer
// in its fragment, or with a DEP pixel before the next one.  At quadric 4096^2 that drops most
// of the 1.8 M sparse 16-byte stores (a few thousand keys are ever read).
#ifndef RC_WKEY
#define RC_WKEY 1   // 0: every writer stores its carry-out (round 3)
#endif
__device__ __forceinline__ bool writer_may_key(unsigned long long mw, unsigned long long md) {
  if (!RC_WKEY) return true;
  const int l = threadIdx.x & 63, fe = l | RC_WKEY_FRAG;
  const unsigned long long upto = fe == 63 ? ~0ull : ((1ull << (fe + 1)) - 1ull);
  const unsigned long long above = upto & ~((2ull << l) - 1ull);   // lanes l+1 .. fe (l = 63: none)
  const unsigned long long nwm = mw & above;
  if (!nwm) return true;
  const int nw = __ffsll((long long)nwm) - 1;
  return (md & above & ((1ull << nw) - 1ull)) != 0ull;
}

// ------------------------------------------------------- scan-order DEP compaction --
// The DEP pixels in scan order (dep_pix, the resolver's and phase C's index), the segment
// table (seg_start: first DEP index of every segment, seg_key: the writer pixel before it,
// -1 = none) and the totals (counters[0] = segments, counters[2] = DEP pixels).  A segment
// starts at a DEP pixel with no DEP pixel before it, or with a writer between it and the
// previous DEP pixel.  One wave per row, ballot scans (no LDS, no barriers); the DEP records
// stay where phase A wrote them (pixel-indexed) and the resolver gathers them by dep_pix.
//   k_row_stats  per row: DEP count, segment starts decided inside the row, last writer,
//                last DEP, the writer before the row's first DEP
//   k_row_scan   one workgroup: exclusive scans over the rows (DEP offsets, last writer /
//                last DEP before each row), the first DEP's start decision, segment offsets
//   k_row_compact per row: dep_pix, seg_start, seg_key
constexpr int kRowWaves = 4;   // rows per 256-thread workgroup

__device__ __forceinline__ unsigned long long lanemask_lt() {
  const int lane = threadIdx.x & 63;
  return lane ? (~0ull >> (64 - lane)) : 0ull;
}
__device__ __forceinline__ int hi_bit(unsigned long long m) { return 63 - __clzll((long long)m); }

struct RowStats {
  int ndep, nstart;        // DEP pixels; segment starts other than the row's first DEP
  long long lastw, lastd;  // last writer / DEP pixel of the row (-1: none)
  long long wfirst;        // last writer before the row's first DEP pixel (-1: none)
};

// A row's class bytes reach LDS in 4 KiB chunks, 16 bytes per lane per load (a wave's 64
// one-byte loads per chunk of 64 pixels were a chain of dependent round trips: k_row_stats
// 39 us, k_row_compact 29 us at 4096^2); the ballot scans then read LDS.
constexpr int kRowChunk = 4096;
__device__ __forceinline__ void stage_row_chunk(const uint8_t* __restrict__ src, int n,
                                                uint8_t* __restrict__ buf, int lane) {
  if ((((size_t)src) & 15) == 0) {
    for (int o = lane * 16; o < n; o += 64 * 16) {
      if (o + 16 <= n) {
        *(uint4*)(buf + o) = *(const uint4*)(src + o);
      } else {
        for (int i = o; i < n; ++i) buf[i] = src[i];
      }
    }
  } else {
    for (int i = lane; i < n; i += 64) buf[i] = src[i];
  }
}

// The one-workgroup kernels of the compaction (k_row_scan, k_seg_order) run as
// kScanBlock threads.  With frames in flight they are dispatched beside the next frame's
// phase A, whose workgroups (4 waves of 128 VGPRs) refill every CU slot they free: a
// 1024-thread workgroup needs a whole CU's wave slots at once and waited 0.05-1.2 ms for one
// (k_row_scan 0.164 ms mean in flight against 13 us alone, profiles/r05_rocprof_headline_...),
// holding the frame's resolver back; 256 threads fit the slot one phase A workgroup frees.
// k_row_scan: chunks of kScanBlock * kScanRows rows, kScanRows consecutive rows per thread
// (their loads issued together), a thread-level pass, block scans of the thread totals + a
// chunk carry.  (One row per thread took four dependent load/scan/store rounds at 4096 rows:
// 16 us.)
#ifndef RC_SCAN_BLOCK
#define RC_SCAN_BLOCK 256
#endif
constexpr int kScanBlock = RC_SCAN_BLOCK;
constexpr int kScanRows = kScanBlock >= 1024 ? 4 : 8;
static_assert(kScanBlock % 64 == 0 && kScanBlock <= 1024, "whole waves, at most 16");

// block-wide exclusive scan of (sum, max, max) over the workgroup; returns the block
// totals in t_cnt / t_w / t_d
__device__ __forceinline__ void block_scan3(int& cnt, long long& lw, long long& ld, int* w_cnt,
                                            long long* w_w, long long* w_d, int& t_cnt,
                                            long long& t_w, long long& t_d) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
  int c = cnt;
  long long a = lw, d = ld;
  for (int o = 1; o < 64; o <<= 1) {   // inclusive wave scans
    const int c2 = __shfl_up(c, o, 64);
    const long long a2 = __shfl_up(a, o, 64), d2 = __shfl_up(d, o, 64);
    if (lane >= o) {
      c += c2;
      a = a2 > a ? a2 : a;
      d = d2 > d ? d2 : d;
    }
  }
  if (lane == 63) {
    w_cnt[wave] = c;
    w_w[wave] = a;
    w_d[wave] = d;
  }
  __syncthreads();
  int pc = 0;
  long long pw = -1, pd = -1;
  for (int q = 0; q < wave; ++q) {
    pc += w_cnt[q];
    pw = w_w[q] > pw ? w_w[q] : pw;
    pd = w_d[q] > pd ? w_d[q] : pd;
  }
  t_cnt = 0;
  t_w = -1;
  t_d = -1;
  for (int q = 0; q < nw; ++q) {
    t_cnt += w_cnt[q];
    t_w = w_w[q] > t_w ? w_w[q] : t_w;
    t_d = w_d[q] > t_d ? w_d[q] : t_d;
  }
  // exclusive: the wave prefix combined with the lanes before this one
  int ec = __shfl_up(c, 1, 64);
  long long ea = __shfl_up(a, 1, 64), ed = __shfl_up(d, 1, 64);
  if (lane == 0) {
    ec = 0;
    ea = -1;
    ed = -1;
  }
  cnt = pc + ec;
  lw = ea > pw ? ea : pw;
  ld = ed > pd ? ed : pd;
  __syncthreads();   // the wave totals are rewritten by the next scan
}

// the scan over the rows by one workgroup (any multiple of 64 threads up to 1024)
__device__ __forceinline__ void row_scan_body(int H, const RowStats* __restrict__ rs,
                                              int* __restrict__ row_off,
                                              int* __restrict__ row_soff,
                                              long long* __restrict__ row_prevw,
                                              long long* __restrict__ row_prevd,
                                              int* __restrict__ counters) {
  __shared__ int w_cnt[16];
  __shared__ long long w_w[16], w_d[16];
  int c_cnt = 0, c_seg = 0;           // chunk carries (every thread holds the same values)
  long long c_w = -1, c_d = -1;
  for (int y0 = 0; y0 < H; y0 += (int)blockDim.x * kScanRows) {
    const int yb = y0 + threadIdx.x * kScanRows;
    RowStats r[kScanRows];
#pragma unroll
    for (int k = 0; k < kScanRows; ++k)
      r[k] = yb + k < H ? rs[yb + k] : RowStats{0, 0, -1, -1, -1};
    // thread totals over its rows
    int cnt = 0;
    long long lw = -1, ld = -1;
#pragma unroll
    for (int k = 0; k < kScanRows; ++k) {
      cnt += r[k].ndep;
      lw = r[k].lastw > lw ? r[k].lastw : lw;
      ld = r[k].lastd > ld ? r[k].lastd : ld;
    }
    int t_cnt;
    long long t_w, t_d;
    block_scan3(cnt, lw, ld, w_cnt, w_w, w_d, t_cnt, t_w, t_d);
    // this thread's exclusive prefix, with the chunk carry
    int pc = c_cnt + cnt;
    long long pw = lw > c_w ? lw : c_w, pdd = ld > c_d ? ld : c_d;
    // per row: exclusive values, the first DEP's start decision, segment counts
    int nseg[kScanRows];
    int segsum = 0;
#pragma unroll
    for (int k = 0; k < kScanRows; ++k) {
      nseg[k] = r[k].nstart;
      if (r[k].ndep > 0) {
        const long long key = r[k].wfirst > pw ? r[k].wfirst : pw;
        if (pdd < 0 || key > pdd) nseg[k] += 1;
      }
      if (yb + k < H) {
        row_off[yb + k] = pc;
        row_prevw[yb + k] = pw;
        row_prevd[yb + k] = pdd;
      }
      pc += r[k].ndep;
      pw = r[k].lastw > pw ? r[k].lastw : pw;
      pdd = r[k].lastd > pdd ? r[k].lastd : pdd;
      segsum += nseg[k];
    }
    // segment offsets: a second block scan (sum)
    int sc = segsum;
    long long dw = -1, dd = -1;
    int t_seg;
    long long u1, u2;
    block_scan3(sc, dw, dd, w_cnt, w_w, w_d, t_seg, u1, u2);
    int ps = c_seg + sc;
#pragma unroll
    for (int k = 0; k < kScanRows; ++k) {
      if (yb + k < H) row_soff[yb + k] = ps;
      ps += nseg[k];
    }
    c_cnt += t_cnt;
    c_seg += t_seg;
    c_w = RC_CHUNK_CARRY_W(t_w > c_w ? t_w : c_w);
    c_d = t_d > c_d ? t_d : c_d;
  }
  if (threadIdx.x == 0) {
    counters[0] = c_seg;
    counters[2] = c_cnt;
  }
}

__global__ void __launch_bounds__(kScanBlock) k_row_scan(int H, const RowStats* __restrict__ rs,
                                                   int* __restrict__ row_off,
                                                   int* __restrict__ row_soff,
                                                   long long* __restrict__ row_prevw,
                                                   long long* __restrict__ row_prevd,
                                                   int* __restrict__ counters) {
  row_scan_body(H, rs, row_off, row_soff, row_prevw, row_prevd, counters);
}

// zero (optional): the frame's counters and TeamState words, cleared here instead of by two
// fill launches before this kernel (every workgroup clears a slice)
__global__ void __launch_bounds__(256) k_row_stats(const uint8_t* __restrict__ cls, int W, int H,
                                                   RowStats* __restrict__ rs,
                                                   int* __restrict__ counters,
                                                   uint4* __restrict__ zero, int zero_words,
                                                   int* __restrict__ zero2, int zero2_ints) {
  __shared__ __attribute__((aligned(16))) uint8_t s_row[kRowWaves][kRowChunk];
  if (zero) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    for (int i = g; i < zero_words; i += gridDim.x * 256) zero[i] = make_uint4(0, 0, 0, 0);
    for (int i = g; i < zero2_ints; i += gridDim.x * 256) zero2[i] = 0;
    if (g < 16) counters[g] = 0;
  }
  const int wave = threadIdx.x >> 6;
  const int y = blockIdx.x * kRowWaves + wave;
  const bool on = y < H;
  const int lane = threadIdx.x & 63;
  const long long base = (long long)y * W;
  const unsigned long long lt = lanemask_lt();
  int nd = 0, ns = 0;
  long long lw = -1, ld = -1, wf = -1;
  for (int xc = 0; xc < W; xc += kRowChunk) {
    const int n = W - xc < kRowChunk ? W - xc : kRowChunk;
    if (on) stage_row_chunk(cls + base + xc, n, s_row[wave], lane);
    __syncthreads();
    // unrolled so that the next sub-chunks' LDS reads issue before this one's ballots
#pragma unroll 8
    for (int x0 = xc; x0 < (on ? xc + n : xc); x0 += 64) {
      const int x = x0 + lane;
      const uint8_t c = x < W ? s_row[wave][x - xc] : kClsIdent;
      const unsigned long long md = __ballot(c == kClsDep), mw = __ballot(c == kClsWriter);
      if (md) {   // (half the image's rows hold no DEP pixel: their chunks skip this part)
        // a DEP lane (not the row's first DEP) starts a segment when a writer lies between it
        // and the previous DEP: last writer before it > previous DEP before it
        const long long kw = (mw & lt) ? base + x0 + hi_bit(mw & lt) : RC_GROUP_CARRY_W(lw);
        const long long pd = (md & lt) ? base + x0 + hi_bit(md & lt) : ld;
        const bool st = c == kClsDep && pd >= 0 && kw > pd;
        ns += __popcll(__ballot(st));
        if (wf < 0 && ld < 0) {   // first DEP of the row is in this chunk
          const int f = __ffsll((long long)md) - 1;
          const unsigned long long wb = mw & ((f ? (~0ull >> (64 - f)) : 0ull));
          wf = wb ? base + x0 + hi_bit(wb) : lw;
        }
        nd += __popcll(md);
        ld = base + x0 + hi_bit(md);
      }
      if (mw) lw = base + x0 + hi_bit(mw);
    }
    __syncthreads();   // the chunk buffer is refilled
  }
  if (on && lane == 0) rs[y] = RowStats{nd, ns, lw, ld, wf};
}

// the segment order by one workgroup of kScanBlock threads
__device__ __forceinline__ void seg_order_body(const int* __restrict__ seg_start,
                                               int* __restrict__ counters,
                                               int* __restrict__ order,
                                               int* __restrict__ batch_state,
                                               int* __restrict__ batch_cnt,
                                               int* __restrict__ batch_rq,
                                               int block_min, int block_cap,
                                               int zero_batches) {
  const int nseg = counters[0], ndep = counters[2];
  // phase C's per-batch claim words (64 DEP entries per batch), completion counts and ready
  // queue are zeroed for this frame: by k_row_stats (launch_parity, batch_ints > 0), else here
  if (zero_batches) {
    for (int b = threadIdx.x; b < (ndep + 63) / 64; b += blockDim.x) {
      batch_state[b] = 0;
      batch_cnt[b] = 0;
      batch_rq[b] = 0;
    }
  }
  if (nseg > kSegOrderMax) {
    if (threadIdx.x == 0) {
      counters[3] = 0;
      counters[14] = 0;
      counters[15] = 0;
    }
    return;
  }
  // A stable counting sort: wave w owns the w-th contiguous part of the segments.  A histogram a
  // wave gives every wave its own slots in every bucket, behind the waves before it; a wave then
  // walks its part 64 consecutive segments a step and the lanes of one bucket take consecutive
  // slots in lane order (ballot), the bucket's next slot advancing step by step.  So inside a
  // bucket the order is the segment order whatever the waves' timing.  (The scatter used to take
  // its slots with one LDS atomic a segment from every wave at once: inside a bucket the waves'
  // chunks then interleaved as they happened to run.)
  constexpr int kOrderWaves = kScanBlock / 64;
  __shared__ int hist[kOrderWaves][256];
  __shared__ int off[kOrderWaves][256];
  __shared__ int tot[256];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nw = (int)blockDim.x >> 6;
  for (int i = t; i < kOrderWaves * 256; i += blockDim.x) (&hist[0][0])[i] = 0;
  __syncthreads();
  auto bucket = [&](int s) {
    const int len = (s + 1 < nseg ? seg_start[s + 1] : ndep) - seg_start[s];
    const int b = RC_SEG_BUCKET(len);
    // (b < 0: after a truncated shard exchange the table holds slots nobody wrote and a length can
    // be negative; the frame is rendered again, but every index here stays in range)
    return 255 - (b < 0 ? 0 : b < 255 ? b : 255);
  };
  const int per = (nseg + nw - 1) / nw;
  const int s0 = wave * per, s1 = s0 + per < nseg ? s0 + per : nseg;
  for (int s = s0 + lane; s < s1; s += 64) atomicAdd(&hist[wave][bucket(s)], 1);
  __syncthreads();
  for (int b = t; b < 256; b += blockDim.x) {   // the waves' offsets inside the bucket
    int acc = 0;
    for (int w = 0; w < nw; ++w) {
      off[w][b] = acc;
      acc += hist[w][b];
    }
    tot[b] = acc;
  }
  __syncthreads();
  if (t == 0) {
    int acc = 0, nlong = 0;
    int bmin = (block_min + 31) >> 5;   // smallest length bucket taken by workgroups
    if (bmin > 255) bmin = 255;
    for (int b = 0; b < 256; ++b) {
      const int n = tot[b];
      tot[b] = acc;   // the bucket's first slot
      acc += n;
      if (block_min > 0 && 255 - b >= bmin) nlong = acc;
    }
    // whole workgroups for the long regular segments only when the regular workgroups can
    // take them in at most two turns: a workgroup resolves a 3 856-entry segment in ~0.55x a
    // lone wave's time at worst and most of them much faster (quadric 4096^2: 154 such
    // segments on 120 workgroups, all done by 2.5 ms); with more the turns queue up and it
    // loses (8192^2 lone 12.9 -> 14.4 ms, frames in flight at 4096^2 5.5e9 vs 6.3e9 rays/s)
    if (nlong > 2 * block_cap) nlong = 0;
    counters[14] = nlong;
    counters[15] = nlong;
  }
  __syncthreads();
  const unsigned long long lt = lanemask_lt();
  for (int sb = s0; sb < s1; sb += 64) {   // (wave-uniform bounds)
    const int s = sb + lane;
    const int b = s < s1 ? bucket(s) : -1;
    unsigned long long todo = __ballot(b >= 0);
    while (todo) {
      const int bb = __shfl(b, __ffsll((long long)todo) - 1, 64);
      const unsigned long long m = __ballot(b == bb);
      const int slot = tot[bb] + off[wave][bb];   // only this wave writes off[wave][.]
      if (b == bb) order[slot + __popcll(m & lt)] = s;
      if (b == bb && !(m & lt)) off[wave][bb] += __popcll(m);   // its first lane: the next step's slot
      __builtin_amdgcn_wave_barrier();   // (no instruction) the wave's later reads see that word
      todo &= ~m;
    }
  }
  if (t == 0) counters[3] = 1;
}

__global__ void __launch_bounds__(256) k_row_compact(
    const uint8_t* __restrict__ cls, int W, int H, const int* __restrict__ row_off,
    const int* __restrict__ row_soff, const long long* __restrict__ row_prevw,
    const long long* __restrict__ row_prevd, long long* __restrict__ dep_pix,
    int* __restrict__ seg_start, long long* __restrict__ seg_key) {
  __shared__ __attribute__((aligned(16))) uint8_t s_row[kRowWaves][kRowChunk];
  const int wave = threadIdx.x >> 6;
  const int y = blockIdx.x * kRowWaves + wave;
  const bool on = y < H;
  const int lane = threadIdx.x & 63;
  const long long base = (long long)y * W;
  const unsigned long long lt = lanemask_lt();
  int idx0 = on ? row_off[y] : 0, s0 = on ? row_soff[y] : 0;
  long long lw = on ? row_prevw[y] : -1, ld = on ? row_prevd[y] : -1;
  for (int xc = 0; xc < W; xc += kRowChunk) {
    const int n = W - xc < kRowChunk ? W - xc : kRowChunk;
    if (on) stage_row_chunk(cls + base + xc, n, s_row[wave], lane);
    __syncthreads();
#pragma unroll 8
    for (int x0 = xc; x0 < (on ? xc + n : xc); x0 += 64) {
      const int x = x0 + lane;
      const uint8_t c = x < W ? s_row[wave][x - xc] : kClsIdent;
      const unsigned long long md = __ballot(c == kClsDep), mw = __ballot(c == kClsWriter);
      if (md) {
        const long long kw = (mw & lt) ? base + x0 + hi_bit(mw & lt) : RC_GROUP_CARRY_W(lw);
        const long long pd = (md & lt) ? base + x0 + hi_bit(md & lt) : ld;
        const bool dep = c == kClsDep;
        const bool st = dep && (pd < 0 || kw > pd);
        const unsigned long long ms = __ballot(st);
        if (dep) {
          const int idx = idx0 + __popcll(md & lt);
          dep_pix[idx] = base + x;
          if (st) {
            const int si = s0 + __popcll(ms & lt);
            seg_start[si] = idx;
            seg_key[si] = kw;
          }
        }
        idx0 += __popcll(md);
        s0 += __popcll(ms);
        ld = base + x0 + hi_bit(md);
      }
      if (mw) lw = base + x0 + hi_bit(mw);
    }
    RC_ROW_CHUNK_END(ld);   // the chunk buffer is refilled
  }
}
// Resolver queue order: segments longest first (LPT), so the chains that take longest start
// at once instead of after the queue reaches them.  One block: a counting sort into 256
// length buckets of 32 entries (>= 8160 share the top bucket), stable within a bucket.
// Above kSegOrderMax segments the queue stays in segment order (counters[3] = 0).
// The order's first counters[14] segments have >= block_min entries (rounded up to the
// bucket width): k_resolve's workgroups take them from head A (counters[1]) while its waves
// start on the rest from head B (counters[15]).
__global__ void __launch_bounds__(kScanBlock) k_seg_order(const int* __restrict__ seg_start,
                                                     int* __restrict__ counters,
                                                     int* __restrict__ order,
                                                     int* __restrict__ batch_state,
                                                     int* __restrict__ batch_cnt,
                                                     int* __restrict__ batch_rq,
                                                     int block_min, int block_cap,
                                                     int zero_batches) {
  seg_order_body(seg_start, counters, order, batch_state, batch_cnt, batch_rq, block_min,
                 block_cap, zero_batches);
}

// ------------------------------------------------------ row shards (rc_shard.hip) --
// A parity image split over G ranks by rows (row y -> rank y % G, local row y / G; SURVEY.md
// §8e).  Every rank runs phase A on its rows into rank-local buffers and packs its DEP entries
// (k_shard_pack); the root gathers them and the ranks' row blocks (every non-DEP pixel is final
// after phase A), rebuilds the image's scan order in a lone frame's layout (k_shard_rows,
// k_row_scan, k_shard_unpack) and runs a lone frame's resolver with phase C inside it, which
// shades every DEP entry into the root's image.  Entries travel in the rank's local scan order,
// which is the image's scan order restricted to the rank's rows.
//
// A DEP entry on the wire: its record (pad = image pixel, pad2 = the last writer pixel before
// it in the same row, -1 = none), that writer's carry-out and the entry's primary shade.  A row's summary: the RowStats
// fields in image pixel indices, the row's first entry in the rank's list and the carry-out of
// the row's last writer (the key of a segment that starts after this row).
struct ShardEntry {
  DepLine rec;   // with the entry's primary shade (phase A, Scene::dep_fast): phase C runs on the root
  float4 kc;     // carry-out of the last writer before the entry in its row
};
struct RowShard {
  int ndep, nstart, loff, pad;
  long long lastw, lastd, wfirst;
  float4 cw;
};
static_assert(sizeof(ShardEntry) == 80 && sizeof(RowShard) == 64, "wire records");

// One wave per local row: the rank's DEP list (local pixels, phase C's index), its wire
// entries (at the local DEP offsets of k_row_scan) and the row summary.
__global__ void __launch_bounds__(256) k_shard_pack(
    const uint8_t* __restrict__ cls, const float4* __restrict__ wcarry,
    const DepLine* __restrict__ deprec, int W, int row0, int row_step, int nrows,
    const int* __restrict__ row_off, long long* __restrict__ dep_pix,
    ShardEntry* __restrict__ ent, RowShard* __restrict__ rs, int thin) {
  const int y = blockIdx.x * kRowWaves + (int)(threadIdx.x >> 6);
  if (y >= nrows) return;
  const int lane = threadIdx.x & 63;
  const long long lbase = (long long)y * W;
  const long long gbase = (long long)(row0 + (long long)y * row_step) * W;
  // thin (the root): records and writer carries are already at their image pixels (k_phase_a
  // rec_img); an entry is only {image pixel, in-row writer before it} (8 B, read in place)
  const long long wbase = thin ? gbase : lbase;
  const unsigned long long lt = lanemask_lt();
  int l0 = row_off[y], nd = 0, ns = 0;
  int lw = -1, ld = -1, wf = -1;   // x of the row's last writer / last DEP / first DEP's writer
  bool first_seen = false;
  for (int x0 = 0; x0 < W; x0 += 64) {
    const int x = x0 + lane;
    const uint8_t c = x < W ? cls[lbase + x] : kClsIdent;
    const unsigned long long md = __ballot(c == kClsDep), mw = __ballot(c == kClsWriter);
    const int kw = (mw & lt) ? x0 + hi_bit(mw & lt) : lw;   // in-row writer before the lane
    const int pd = (md & lt) ? x0 + hi_bit(md & lt) : ld;   // in-row DEP before the lane
    const bool dep = c == kClsDep;
    ns += __popcll(__ballot(dep && pd >= 0 && kw > pd));
    if (!first_seen && md) {
      const int f = __ffsll((long long)md) - 1;
      const unsigned long long wb = mw & (f ? (~0ull >> (64 - f)) : 0ull);
      wf = wb ? x0 + hi_bit(wb) : lw;
      first_seen = true;
    }
    if (dep) {
      const int l = l0 + __popcll(md & lt);
      dep_pix[l] = lbase + x;
      if (thin) {
        ((int2*)ent)[l] = make_int2((int)(gbase + x), kw >= 0 ? (int)(gbase + kw) : -1);
      } else {
        ShardEntry e;
        e.rec = deprec[lbase + x];
        e.rec.r.pad = (int)(gbase + x);
        e.rec.r.pad2 = kw >= 0 ? (int)(gbase + kw) : -1;
        e.kc = kw >= 0 ? wcarry[lbase + kw] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        ent[l] = e;
      }
    }
    l0 += __popcll(md);
    nd += __popcll(md);
    if (mw) lw = x0 + hi_bit(mw);
    if (md) ld = x0 + hi_bit(md);
  }
  if (lane == 0) {
    RowShard r;
    r.ndep = nd;
    r.nstart = ns;
    r.loff = row_off[y];
    r.pad = 0;
    r.lastw = lw >= 0 ? gbase + lw : -1;
    r.lastd = ld >= 0 ? gbase + ld : -1;
    r.wfirst = wf >= 0 ? gbase + wf : -1;
    r.cw = lw >= 0 ? wcarry[wbase + lw] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    rs[y] = r;
  }
}

struct ShardOffs {
  long long off[kMaxShards];   // first entry of rank g in the gathered entry list
};

// Root: the image's RowStats from the gathered row summaries ([G][rmax], row y at [y%G][y/G]).
__global__ void __launch_bounds__(256) k_shard_rows(const RowShard* __restrict__ rsall, int G,
                                                    int rmax, int H, RowStats* __restrict__ rs) {
  const int y = blockIdx.x * blockDim.x + threadIdx.x;
  if (y >= H) return;
  const RowShard r = rsall[(size_t)(y % G) * rmax + y / G];
  rs[y] = RowStats{r.ndep, r.nstart, r.lastw, r.lastd, r.wfirst};
}

// Root, one wave per image row: the row's entries in scan order -> the resolver's inputs, in a
// lone frame's layout (image pixel indices): the DEP line (record and primary shade) at
// deprec[pixel], dep_pix = the pixels in scan order and every segment's key =
// the image pixel of the writer before it, whose carry-out goes to wcarry[writer] (a DEP
// pixel and a writer are never the same pixel).  The resolver, phase C inside it and its
// framebuffer stores then run exactly as in a lone frame, into the root's image.  A segment
// start is decided exactly as in k_row_compact (writer after the previous DEP).
__global__ void __launch_bounds__(256) k_shard_unpack(
    const RowShard* __restrict__ rsall, const ShardEntry* __restrict__ ent,
    const ShardEntry* __restrict__ ent0, ShardOffs offs,
    int G, int rmax, int W, int H, const int* __restrict__ row_off,
    const int* __restrict__ row_soff, const long long* __restrict__ row_prevw,
    const long long* __restrict__ row_prevd, DepLine* __restrict__ deprec,
    long long* __restrict__ dep_pix, int* __restrict__ seg_start,
    long long* __restrict__ seg_key, float4* __restrict__ wcarry, int bound, int thin0) {
  const int y = blockIdx.x * kRowWaves + (int)(threadIdx.x >> 6);
  if (y >= H) return;
  const int lane = threadIdx.x & 63;
  const long long P = (long long)W * H;
  const int g = y % G;
  const RowShard r = rsall[(size_t)g * rmax + y / G];
  // rank 0's entries are the root's own list (never copied), the others' the gathered blocks;
  // thin0: the root's list is {image pixel, writer} pairs whose records and writer carries its
  // phase A already wrote at their image pixels (k_shard_pack thin)
  const bool th = g == 0 && ent0 && thin0;
  const ShardEntry* e = (g == 0 && ent0 ? ent0 : ent + offs.off[g]) + r.loff;
  const int2* et = (const int2*)ent0 + r.loff;
  const int n = r.ndep;
  const int idx0 = row_off[y];
  int s0 = row_soff[y];
  long long pd = row_prevd[y];
  const long long pw = row_prevw[y];
  float4 pwc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (pw >= 0) {   // the writer before the row is the last writer of its own row
    const int yw = (int)(pw / W);
    pwc = rsall[(size_t)(yw % G) * rmax + yw / G].cw;
  }
  const unsigned long long lt = lanemask_lt();
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const bool valid = i < n;
    ShardEntry q;
    if (valid && !th) q = e[i];
    if (valid && th) {
      const int2 tq = et[i];
      q.rec.r.pad = tq.x;
      q.rec.r.pad2 = tq.y;
    }
    // bound: the fixed-size exchange delivered each rank's first `bound` entries.  A longer
    // list (the frame is then rendered again, rc_shard.hip) reads the next rank's block: such
    // an entry becomes a harmless record (zero directions, shape 0) at the spare pixel P (the
    // root's buffers hold P + 1 pixels), continuing its segment — never an out-of-range shape
    // or pixel index for the resolver and phase C.  The root's own list is read in place: whole.
    const bool spare = valid && ((!th && r.loff + i >= bound) || q.rec.r.pad < 0 ||
                                 q.rec.r.pad >= P);
    if (spare) {
      q.rec = DepLine{DepRec{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0, -1, 0.0f, 0.0f, 0.0f, -1},
                      0.0f, 0.0f, 0.0f, 0};
      q.kc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const long long pix = valid ? (spare ? P : (long long)q.rec.r.pad) : -1;
    const long long kin = valid && !spare && q.rec.r.pad2 >= 0 && q.rec.r.pad2 < P
                              ? (long long)q.rec.r.pad2 : -1;
    long long prev = __shfl_up(pix, 1, 64);
    if (lane == 0) prev = pd;
    const long long kw = kin >= 0 ? kin : pw;
    const bool st = valid && (prev < 0 || kw > prev);
    const unsigned long long ms = __ballot(st);
    if (valid) {
      const int idx = idx0 + i;
      if (!th || spare) deprec[pix] = q.rec;
      dep_pix[idx] = pix;
      if (st) {
        const int s = s0 + __popcll(ms & lt);
        seg_start[s] = idx;
        seg_key[s] = kw;
        // every entry keyed by kw writes the same carry-out; the root's own in-row writers'
        // carries are in place already
        if (kw >= 0 && !(th && kin >= 0)) wcarry[kw] = kin >= 0 ? q.kc : pwc;
      }
    }
    s0 += __popcll(ms);
    const int last = (n - i0 < 64 ? n - i0 : 64) - 1;
    pd = __shfl(pix, last, 64);
  }
}

// Root: image row y <- gathered[y % G][y / G] (the row-cyclic partition undone).
__global__ void __launch_bounds__(256) k_deinterleave(const uint8_t* __restrict__ gathered,
                                                      const uint8_t* __restrict__ block0,
                                                      int G, int rmax, int W, int H,
                                                      uint8_t* __restrict__ img) {
  const int y = blockIdx.x;
  const size_t rb = (size_t)W * 3;
  // rank 0's rows come from the root's own block (not copied into `gathered`)
  const uint8_t* src = (y % G == 0 && block0) ? block0 + (size_t)(y / G) * rb
                                              : gathered + ((size_t)(y % G) * rmax + y / G) * rb;
  uint8_t* dst = img + (size_t)y * rb;
  if ((rb & 3) == 0) {
    for (size_t i = threadIdx.x; i < rb / 4; i += blockDim.x)
      ((uint32_t*)dst)[i] = ((const uint32_t*)src)[i];
  } else {
    for (size_t i = threadIdx.x; i < rb; i += blockDim.x) dst[i] = src[i];
  }
}
}  // namespace rc
