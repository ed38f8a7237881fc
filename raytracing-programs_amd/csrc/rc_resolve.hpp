// rc_resolve.hpp — the carry resolver's window code: the DEP records' gathering,
// the wave's and the workgroup's LANE/COOP window state machines with their carry predictor, and
// the tagged carry-in granules.  k_resolve (rc_kernels.hip) is built from these; the entry-level
// test harness (tests/tools/resolve_check.hip) includes them too, so both run the same text.
#pragma once
#include <hip/hip_runtime.h>

#include "rc_cudasem.hpp"
#include "rc_device.hpp"

namespace rc {

constexpr int kResolveBlock = 256;

// The windows' two bit-for-bit comparisons, by role.  Only the test harness's wrong variants
// (resolve_check.hip, RV_WRONG) define them otherwise, before this header; the product never does.
#ifndef RC_WIN_SAME
#define RC_WIN_SAME(a, b) same_bits(a, b)     // an evaluation left the carry as it was
#endif
#ifndef RC_GUESS_SAME
#define RC_GUESS_SAME(a, b) same_bits(a, b)   // a guessed carry-in is the exact one
#endif

// DEP entry j's record: phase A wrote it at the pixel (dep_pix[j]); gathered, never copied.
__device__ __forceinline__ DepRec rec_at(const DepLine* __restrict__ deprec,
                                         const long long* __restrict__ dep_pix, int j) {
  return deprec[dep_pix[j]].r;   // the first 48 bytes of the line (the shade is phase C's)
}

// Resolve the 64 entries [base, base+64) ∩ [.., end) of one wave at carry `c`, changers
// included.  On return: `mine` = this lane's carry-in, `c` = carry after the window; the
// result counts transfer-function evaluation steps.  The first pass evaluates the 64
// entries one per lane.  After a changer the rest of the window is dense-prone (the carry
// creeps one entry at a time in long runs), so it continues with the cooperative evaluator:
// 64/G entries per step, shapes spread over the G lanes of each group.
__device__ __forceinline__ DepRec shfl_rec(const DepRec& r, int src) {
  DepRec o;
  o.ax = __shfl(r.ax, src, 64);
  o.ay = __shfl(r.ay, src, 64);
  o.az = __shfl(r.az, src, 64);
  o.n0x = __shfl(r.n0x, src, 64);
  o.n0y = __shfl(r.n0y, src, 64);
  o.n0z = __shfl(r.n0z, src, 64);
  o.obj0 = __shfl(r.obj0, src, 64);
  o.pad = 0;
  o.bx = __shfl(r.bx, src, 64);
  o.by = __shfl(r.by, src, 64);
  o.bz = __shfl(r.bz, src, 64);
  o.pad2 = 0;
  return o;
}

// Window state machine.  LANE: one entry per lane at the current carry (64 entries for one
// evaluation's latency: right for clean stretches).  COOP: the cooperative evaluator, 64/GE
// entries per step at a lower latency (right inside dense runs, where every entry may move
// the carry).  A changer found by a LANE pass switches to COOP; two clean COOP steps in a row
// switch back.  `dense` carries the mode into the next window.  Returns the number of
// evaluation steps; *changed tells whether any entry of the window moved the carry.
struct WinStats {
  int lane, coop, changers;
#if RC_STAMPS   // diagnostic build: cycles inside the evaluations / whole steps / waiting at
                // the step's barrier (block_window)
  unsigned long long ce, cs, cw;
#endif
};

// Carry predictor for dense runs.  Inside a run of changers the carry creeps: at quadric
// 4096^2 the seven 1 377-entry all-changer segments move one component by a near-constant
// number of float ulps per entry (9-12, 143-156, -195..-209, ...) and keep the other two.
// The cooperative evaluator then spends its spare lane groups on entry pos+1 at guessed
// carry-ins bits(c) + mean delta of the last few changes (+-1, +-2.. ulps on the moving
// component); when entry pos's exact output equals a guess bit for bit, entry pos+1's
// evaluation at that guess IS its exact evaluation and two entries retire in one step.  The
// guesses only choose what to evaluate, never what is accepted.
struct CarryHist {
  V3 h[4];   // carries after the last changes, h[0] the latest
  int n;
  int run;   // changes in a row (a hand-off to a helper block starts a long run, k_resolve)
};
#ifndef RC_PREDICT
#define RC_PREDICT 1
#endif
constexpr bool kPredict = RC_PREDICT != 0;
// Helper blocks' predictive step: 0 = its 15 guesses all for entry pos+1; k = groups 1..k guess
// pos+1 and groups k+1..15 guess pos+2 (oracle simulation of the seven dense 1 377-entry
// segments at quadric 4096^2, scripts/pred_sim.py: 1.65-1.99 entries per step with 15/0,
// 1.54-2.95 with 7/8, 1.60-2.91 with 9/6)
#ifndef RC_PRED_SPLIT
#define RC_PRED_SPLIT 0
#endif
constexpr int kPredSplit = RC_PRED_SPLIT;
__device__ __forceinline__ void hist_push(CarryHist& hs, V3 c) {
  hs.run = hs.n == 0 ? 0 : hs.run + 1;
  hs.h[3] = hs.h[2];
  hs.h[2] = hs.h[1];
  hs.h[1] = hs.h[0];
  hs.h[0] = c;
  hs.n = hs.n < 4 ? hs.n + 1 : 4;
}
// guess q (1..) of the carry after c: the mean delta of the history, in float bits, with the
// moving component offset by 0, -1, +1, -2, +2, ...
__device__ __forceinline__ V3 hist_guess(const CarryHist& hs, V3 c, int q, int mult = 1) {
  // no run-time index into h[] (it would put the history in scratch memory, whose reload
  // waits for every store in flight — the carry-in publications) and no run-time divisor
  const int m = hs.n - 1;   // 1..3
  const V3 o = sel(m == 3, hs.h[3], sel(m == 2, hs.h[2], hs.h[1]));   // not a struct ?:
  auto md = [&](float a, float b) {
    const int d = (int)(__float_as_uint(a) - __float_as_uint(b));
    const int r = d >= 0 ? 1 : -1;   // m / 2 rounded away from zero, for m = 2, 3
    return m == 1 ? d : (m == 2 ? (d + r) / 2 : (d + r) / 3);
  };
  int dx = md(hs.h[0].x, o.x), dy = md(hs.h[0].y, o.y), dz = md(hs.h[0].z, o.z);
  if (mult != 1) dx *= mult, dy *= mult, dz *= mult;
  const int j = q - 1;
  const int off = (j & 1) ? -((j + 1) >> 1) : (j >> 1);   // q = 1, 2, 3, 4.. -> 0, -1, +1, -2..
  const int ax = abs(dx), ay = abs(dy), az = abs(dz);
  if (ax >= ay && ax >= az) dx += off;
  else if (ay >= az) dy += off;
  else dz += off;
  return v3(__uint_as_float(__float_as_uint(c.x) + (unsigned)dx),
            __uint_as_float(__float_as_uint(c.y) + (unsigned)dy),
            __uint_as_float(__float_as_uint(c.z) + (unsigned)dz));
}

__device__ __forceinline__ int wave_window(const Scene& sc, int maxrec,
                                           const DepLine* __restrict__ deprec,
                                           const long long* __restrict__ dep_pix, int base,
                                           int end, V3& c, V3& mine, bool& mhit,
                                           const LaneShape& ls,
                                           int G, bool& dense, bool& changed,
                                           WinStats& ws, int K, CarryHist& hs
#if RC_STAMPS
                                           , Stamps* st_
#endif
) {
  const int lane = threadIdx.x & 63;
  const int idx = base + lane;
  const int nvalid = end - base < 64 ? end - base : 64;
  const bool valid = lane < nvalid;
  DepRec r;
  if (valid) r = rec_at(deprec, dep_pix, idx);
  mine = c;
  mhit = false;
  changed = false;
  int zero = 0;
  int evals = 0;
  int pos = 0;                     // lanes < pos are resolved
  bool coop = dense && G > 0;
  int clean_run = 0;
  const bool spec = 2 * G <= 64;
  const int GE = G > 0 ? (spec ? 2 * G : G) : 64;
  const int E = 64 / GE;
  const int e = lane / GE, kself = G > 0 ? lane % G : 0, half = spec ? (lane / G) & 1 : 0;
  while (pos < nvalid) {
    ++evals;
    if (!coop) {
      ++ws.lane;
      const bool act = valid && lane >= pos;
      V3 o = c;
      bool h = false;
#if RC_STAMPS
      const unsigned long long tl0_ = stamp_now();
#endif
      if (act) o = carry_path(sc, r, maxrec, c, zero, h);
      const unsigned long long m = __ballot(act && !RC_WIN_SAME(o, c));
#if RC_STAMPS
      st_->acc[0] += stamp_now() - tl0_;
#endif
      if (m == 0) {
        if (act) {
          mine = c;
          mhit = h;
        }
        hs.n = 0;
        pos = nvalid;
        break;
      }
      const int k = __ffsll((long long)m) - 1;
      if (act && lane <= k) {
        mine = c;
        mhit = h;
      }
      if (k > 0 || hs.n == 0) hs.n = 0, hist_push(hs, c);   // the run starts at this change
      c = v3(__shfl(o.x, k, 64), __shfl(o.y, k, 64), __shfl(o.z, k, 64));
      hist_push(hs, c);
      pos = k + 1;
      changed = true;
      ++ws.changers;
      coop = G > 0;
      clean_run = 0;
      continue;
    }
    ++ws.coop;
#if RC_STAMPS == 2   // coarse: acc[1] = evaluations, acc[2] = whole cooperative steps
    const unsigned long long cs0_ = __builtin_amdgcn_s_memtime();
#endif
    // predictive step (CarryHist): group 0 takes entry pos at c, the others entry pos+1 at
    // guessed carry-ins; otherwise groups take entries pos, pos+1, .. all at c
    const bool predict = hs.n >= 2 && E >= 2 && pos + 1 < nvalid && kPredict;
    const int i = predict ? pos + (e > 0 ? 1 : 0) : pos + e;
    const V3 ce = sel(predict && e > 0 && e < E, hist_guess(hs, c, e), c);
    const bool act = e < E && i < nvalid;
    const DepRec ri = shfl_rec(r, i < 64 ? i : 63);
    V3 oc = ce;
    bool hg = false;
#if RC_STAMPS
#define RC_SPEC1(GT, Q) carry_path_spec<GT, Q>(sc, ls, kself, G, half, ri, maxrec, ce, zero, hg, st_)
#else
#define RC_SPEC1(GT, Q) carry_path_spec<GT, Q>(sc, ls, kself, G, half, ri, maxrec, ce, zero, hg)
#endif
#define RC_SPEC(GT) \
  (sc.has_quadric ? (quad_x0(sc) ? RC_SPEC1(GT, 2) : RC_SPEC1(GT, 1)) : RC_SPEC1(GT, 0))
    if (act) {
      if (G == 8) oc = RC_SPEC(8);
      else if (G == 4) oc = RC_SPEC(4);
      else if (G == 16) oc = RC_SPEC(16);
      else if (spec) oc = RC_SPEC(0);
      else oc = carry_path_coop(sc, ls, kself, G, ri, maxrec, ce, zero, hg);
    }
#undef RC_SPEC
#undef RC_SPEC1
#if RC_STAMPS == 2
    st_->acc[1] += __builtin_amdgcn_s_memtime() - cs0_;
    struct StepEnd_ {
      Stamps* s;
      unsigned long long t;
      __device__ ~StepEnd_() { s->acc[2] += __builtin_amdgcn_s_memtime() - t; }
    } step_end_{st_, cs0_};
#endif
    if (predict) {
      const V3 o0 = v3(__shfl(oc.x, 0, 64), __shfl(oc.y, 0, 64), __shfl(oc.z, 0, 64));
      const bool h0 = __shfl((int)hg, 0, 64) != 0;
      if (lane == pos) {
        mine = c;
        mhit = h0;
      }
      if (RC_WIN_SAME(o0, c)) {   // entry pos leaves the carry: the run is over
        hs.n = 0;
        pos += 1;
        if (++clean_run >= K) coop = false;
        continue;
      }
      changed = true;
      ++ws.changers;
      clean_run = 0;
      hist_push(hs, o0);
      const unsigned long long mm =
          __ballot(act && e > 0 && (lane % GE) == 0 && RC_GUESS_SAME(ce, o0));
      if (mm == 0) {
        c = o0;
        pos += 1;
        continue;
      }
      const int gl = __ffsll((long long)mm) - 1;   // leader lane of the matching group
      const V3 o1 = v3(__shfl(oc.x, gl, 64), __shfl(oc.y, gl, 64), __shfl(oc.z, gl, 64));
      const bool h1 = __shfl((int)hg, gl, 64) != 0;
      if (lane == pos + 1) {
        mine = o0;
        mhit = h1;
      }
      pos += 2;
      if (RC_WIN_SAME(o1, o0)) {
        hs.n = 0;
        c = o0;
        if (++clean_run >= K) coop = false;
      } else {
        ++ws.changers;
        hist_push(hs, o1);
        c = o1;
      }
      continue;
    }
    const unsigned long long mc = __ballot(act && (lane % GE) == 0 && !RC_WIN_SAME(oc, c));
    // entry pos+q's hit flag sits in its group's first lane, q*GE
    const int q = lane - pos;
    const bool hq = __shfl((int)hg, (q >= 0 && q < E ? q : 0) * GE, 64) != 0;
    if (mc == 0) {
      hs.n = 0;
      const int lim = pos + E < nvalid ? pos + E : nvalid;
      if (lane >= pos && lane < lim) {
        mine = c;
        mhit = hq;
      }
      pos = lim;
      if (++clean_run >= K) coop = false;
      continue;
    }
    const int g = (__ffsll((long long)mc) - 1) / GE;
    if (lane >= pos && lane <= pos + g) {
      mine = c;
      mhit = hq;
    }
    if (g > 0 || hs.n == 0) hs.n = 0, hist_push(hs, c);
    c = v3(__shfl(oc.x, g * GE, 64), __shfl(oc.y, g * GE, 64), __shfl(oc.z, g * GE, 64));
    hist_push(hs, c);
    pos += g + 1;
    changed = true;
    ++ws.changers;
    clean_run = 0;
  }
  dense = coop;
  return evals;
}

__device__ __forceinline__ unsigned long long pack2(unsigned lo, unsigned hi) {
  return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

// Carry-in hand-off (MI355X_MICROARCH.md / cdna_hip_programming.md Guideline 16, R2): each
// entry's carry-in is three naturally aligned 8-byte granules {value, tag}, each written by ONE
// agent-scope (sc1) store, tag = this frame's epoch.  The phase-C tail (other waves of the same
// launch, any XCD) reads them with sc1 loads and accepts an entry only when all three tags
// match, so no flag, fence or ordering is involved; a stale or torn entry is simply retried.
struct CinG {
  unsigned long long g[3];
};
// The tag's top bit carries the entry's hit flag (some bounce level hit at this carry-in:
// not clean, Scene::dep_fast); epochs stay below 2^31.
constexpr unsigned kCinHit = 0x80000000u;
__device__ __forceinline__ void cin_put(CinG* cin, int j, V3 c, unsigned tag, bool hit) {
  const unsigned tg = tag | (hit ? kCinHit : 0u);
  __hip_atomic_store(&cin[j].g[0], pack2(__float_as_uint(c.x), tg), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&cin[j].g[1], pack2(__float_as_uint(c.y), tg), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&cin[j].g[2], pack2(__float_as_uint(c.z), tg), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
// A whole wave publishes the entries j0+lo .. j0+hi-1 (lanes lo..hi-1 of the wave's 64-entry
// slice) together: store instruction i writes granule 64*i + lane of the slice, so each
// instruction covers 512 contiguous bytes instead of 64 granules at a 24-byte stride (the
// agent-scope stores write through to memory: strided granules cost ~3x their bytes in HBM
// writes, rocprofv3 WRITE_SIZE).  Every granule is still one 8-byte atomic store with its own
// tag, so readers are unchanged.  The carry is either the wave's own per-lane value
// (cin_put_wave) or one carry for the whole range (cin_put_wave_uniform); hitmask bit e is
// entry lane e's hit flag.  Every lane of the wave must call these.
__device__ __forceinline__ void cin_put_granules(CinG* cin, int j0, int lo, int hi, V3 c_lane,
                                                 bool uniform, unsigned tag,
                                                 unsigned long long hitmask) {
  const int lane = threadIdx.x & 63;
  unsigned long long* g = &cin[j0].g[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int q = 64 * i + lane;
    const int e = q / 3, comp = q - 3 * e;
    float x = c_lane.x, y = c_lane.y, z = c_lane.z;
    if (!uniform) {
      x = __shfl(x, e, 64);
      y = __shfl(y, e, 64);
      z = __shfl(z, e, 64);
    }
    const float v = comp == 0 ? x : (comp == 1 ? y : z);
    const unsigned tg = tag | (((hitmask >> e) & 1ull) ? kCinHit : 0u);
    if (e >= lo && e < hi)
      __hip_atomic_store(&g[q], pack2(__float_as_uint(v), tg), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
}
// Per-lane carries staged through the wave's own 768 bytes of LDS (entry-major x, y, z: float
// q of the stage is granule q's value) instead of cross-lane shuffles.
__device__ __forceinline__ void cin_put_wave(CinG* cin, int j0, int lo, int hi, V3 c_lane,
                                             unsigned tag, unsigned long long hitmask,
                                             float* stage) {
  const int lane = threadIdx.x & 63;
  stage[3 * lane] = c_lane.x;
  stage[3 * lane + 1] = c_lane.y;
  stage[3 * lane + 2] = c_lane.z;
  __builtin_amdgcn_wave_barrier();   // one wave's LDS accesses complete in order
  unsigned long long* g = &cin[j0].g[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int q = 64 * i + lane;
    const int e = q / 3;
    const unsigned tg = tag | (((hitmask >> e) & 1ull) ? kCinHit : 0u);
    const float v = stage[q];
    if (e >= lo && e < hi)
      __hip_atomic_store(&g[q], pack2(__float_as_uint(v), tg), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
  __builtin_amdgcn_wave_barrier();   // the stage is rewritten by the next window
}
__device__ __forceinline__ void cin_put_wave_uniform(CinG* cin, int j0, int lo, int hi, V3 c,
                                                     unsigned tag, unsigned long long hitmask) {
  cin_put_granules(cin, j0, lo, hi, c, true, tag, hitmask);
}

__device__ __forceinline__ bool cin_get(CinG* cin, int j, unsigned tag, V3& c, bool& hit) {
  const unsigned long long a =
      __hip_atomic_load(&cin[j].g[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long b =
      __hip_atomic_load(&cin[j].g[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long d =
      __hip_atomic_load(&cin[j].g[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  c = v3(__uint_as_float((unsigned)a), __uint_as_float((unsigned)b),
         __uint_as_float((unsigned)d));
  const unsigned ta = (unsigned)(a >> 32);
  hit = (ta & kCinHit) != 0u;
  return (ta & ~kCinHit) == tag && (unsigned)(b >> 32) == ta && (unsigned)(d >> 32) == ta;
}

// Block-level window for the team's RESOLVE leader: the 4 waves of one block resolve up to
// 256 entries at the block-uniform carry c with the same LANE/COOP state machine as
// wave_window, at 4x the width — COOP steps take 4*E entries (E per wave) and LANE passes
// 256 — so clusters with short clean gaps cost one cooperative evaluation per changer.
// The window's records sit in LDS (`rec`, loaded by the caller); per-step results meet in
// double-buffered per-wave slots behind one barrier.  Entries are written to cin as they
// resolve.  Every thread of the block must call this.
struct BlockWinShared {
  DepRec rec[kResolveBlock];
  uint8_t hit[kResolveBlock];   // per entry: some level hit at the window's carry
  int wpos[2][4];
  float wout[2][4][3];
  // predictive steps (helper blocks): per group its output, hit flag and guess, double-
  // buffered by step parity like wpos / wout (one barrier per step)
  float pout[2][16][3];
  float pce[2][16][3];
  int phit[2][16];
};

// hp (helper blocks): carry predictor; the cooperative step then takes entry pos at c in
// group 0 and entry pos+1 at Eb-1 guessed carry-ins in the other groups (wave_window's
// predictive step with the whole block: 15 guesses instead of 3).
// stop (the team leader): instead of a LANE pass after K clean cooperative steps, return at
// once with the number of entries resolved so far (the team's cooperative SCAN takes the
// rest, k_resolve).  Returns -1 when the window was resolved to its end.
__device__ __forceinline__ int block_window(const Scene& sc, int maxrec, BlockWinShared& bw,
                                            int base, int nvalid, V3& c, const LaneShape& ls,
                                            int G, bool& dense, bool& changed, int K,
                                            CinG* __restrict__ cin, unsigned tag,
                                            WinStats& ws, CarryHist* hp = nullptr,
                                            bool stop = false) {
  int stopped = -1;
  constexpr int kNo = 0x7fffffff;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  changed = false;
  int zero = 0;
  int pos = 0;
  int par = 0;
  bool coop = dense && G > 0;
  int clean_run = 0;
  const bool spec = 2 * G <= 64;
  const int GE = G > 0 ? (spec ? 2 * G : G) : 64;
  const int E = 64 / GE;
  const int Eb = 4 * E;
  const int e = lane / GE, kself = G > 0 ? lane % G : 0, half = spec ? (lane / G) & 1 : 0;
#if RC_STAMPS
  unsigned long long top_ = 0;
#endif
  while (pos < nvalid) {
#if RC_STAMPS
    {
      const unsigned long long n_ = __builtin_amdgcn_s_memtime();
      if (top_) ws.cs += n_ - top_;
      top_ = n_;
    }
#endif
    int last;      // entries [pos, last] resolve with carry c
    V3 cn = c;
    bool hit;
    // (spec: the step below evaluates through carry_path_spec, which needs an entry's two groups,
    // 2 G lanes.  With G = 64 — scenes of 33 to 64 shapes — there is no second group: its lanes
    // read their own group's result as the speculated level's, so a level after a missed one was
    // skipped unevaluated.  Such a scene's helpers take the plain cooperative steps below.)
    if (coop && hp && kPredict && spec && hp->n >= 2 && pos + 1 < nvalid && Eb <= 16 && Eb >= 2) {
      ++ws.coop;
      const int gi = wave * E + e;
      // groups 1..k1 guess entry pos+1's carry-in; with RC_PRED_SPLIT the groups above k1 guess
      // entry pos+2's (twice the history's mean step: a hit retires three entries)
      const bool three = kPredSplit > 0 && kPredSplit < Eb - 1 && pos + 2 < nvalid;
      const int k1 = three ? kPredSplit : Eb - 1;
      const bool g2 = gi > k1;
      const int i = pos + (gi > 0 ? 1 : 0) + (g2 ? 1 : 0);
      const V3 ce = sel(gi > 0, hist_guess(*hp, c, g2 ? gi - k1 : gi, g2 ? 2 : 1), c);
      const DepRec ri = bw.rec[i < nvalid ? i : pos];
      V3 oc = ce;
      bool hg = false;
#if RC_STAMPS
      Stamps stp = {{0, 0, 0, 0}, 0};
#define RC_SPEC1(GT, Q) carry_path_spec<GT, Q>(sc, ls, kself, G, half, ri, maxrec, ce, zero, hg, &stp)
#else
#define RC_SPEC1(GT, Q) carry_path_spec<GT, Q>(sc, ls, kself, G, half, ri, maxrec, ce, zero, hg)
#endif
#define RC_SPEC(GT) \
  (sc.has_quadric ? (quad_x0(sc) ? RC_SPEC1(GT, 2) : RC_SPEC1(GT, 1)) : RC_SPEC1(GT, 0))
      if (G == 8) oc = RC_SPEC(8);
      else if (G == 4) oc = RC_SPEC(4);
      else if (G == 16) oc = RC_SPEC(16);
      else oc = RC_SPEC(0);
#undef RC_SPEC
#undef RC_SPEC1
#if RC_STAMPS
      ws.ce += __builtin_amdgcn_s_memtime() - top_;
#endif
      if ((lane % GE) == 0) {
        bw.pout[par][gi][0] = oc.x;
        bw.pout[par][gi][1] = oc.y;
        bw.pout[par][gi][2] = oc.z;
        bw.pce[par][gi][0] = ce.x;
        bw.pce[par][gi][1] = ce.y;
        bw.pce[par][gi][2] = ce.z;
        bw.phit[par][gi] = hg ? 1 : 0;
      }
      // one barrier per step: every wave finds the matching guess itself (the same ballot
      // over the same slots), and the slots are double-buffered by step parity — a wave
      // writes parity p again only after every wave has passed the barrier of the step
      // in between, i.e. has read these
#if RC_STAMPS
      const unsigned long long bw0_ = __builtin_amdgcn_s_memtime();
#endif
      __syncthreads();
#if RC_STAMPS
      ws.cw += __builtin_amdgcn_s_memtime() - bw0_;
#endif
      const V3 o0 = v3(bw.pout[par][0][0], bw.pout[par][0][1], bw.pout[par][0][2]);
      const V3 pl = v3(bw.pce[par][lane < Eb ? lane : 0][0], bw.pce[par][lane < Eb ? lane : 0][1],
                       bw.pce[par][lane < Eb ? lane : 0][2]);
      const bool mt = lane > 0 && lane <= k1 && RC_GUESS_SAME(pl, o0);
      const unsigned long long mm = __ballot(mt);
      const int mi = mm ? __ffsll((long long)mm) - 1 : 0;
      if (t == pos) cin_put(cin, base + pos, c, tag, bw.phit[par][0] != 0);
      if (RC_WIN_SAME(o0, c)) {   // entry pos leaves the carry: the run is over
        hp->n = 0;
        pos += 1;
        if (++clean_run >= K) coop = false;
      } else {
        changed = true;
        ++ws.changers;
        clean_run = 0;
        hist_push(*hp, o0);
        if (mi > 0) {
          const V3 o1 = v3(bw.pout[par][mi][0], bw.pout[par][mi][1], bw.pout[par][mi][2]);
          if (t == pos + 1) cin_put(cin, base + pos + 1, o0, tag, bw.phit[par][mi] != 0);
          pos += 2;
          if (RC_WIN_SAME(o1, o0)) {
            hp->n = 0;
            c = o0;
          } else {
            ++ws.changers;
            hist_push(*hp, o1);
            c = o1;
            // entry pos+2 (now pos) evaluated at a guess equal to o1: its exact evaluation
            const unsigned long long m2 = three ? __ballot(lane > k1 && lane < Eb && RC_GUESS_SAME(pl, o1)) : 0ull;
            if (m2) {
              const int mj = __ffsll((long long)m2) - 1;
              const V3 o2 = v3(bw.pout[par][mj][0], bw.pout[par][mj][1], bw.pout[par][mj][2]);
              if (t == pos) cin_put(cin, base + pos, o1, tag, bw.phit[par][mj] != 0);
              pos += 1;
              if (RC_WIN_SAME(o2, o1)) {
                hp->n = 0;
              } else {
                ++ws.changers;
                hist_push(*hp, o2);
                c = o2;
              }
            }
          }
        } else {
          c = o0;
          pos += 1;
        }
      }
      par ^= 1;
      continue;
    }
    if (!coop) {
      ++ws.lane;
      const bool act = t >= pos && t < nvalid;
      V3 o = c;
      bool h = false;
      if (act) o = carry_path(sc, bw.rec[t], maxrec, c, zero, h);
#if RC_STAMPS
      ws.ce += __builtin_amdgcn_s_memtime() - top_;
#endif
      bw.hit[t] = h ? 1 : 0;
      const unsigned long long m = __ballot(act && !RC_WIN_SAME(o, c));
      const int k = m ? __ffsll((long long)m) - 1 : -1;
      if (lane == 0) bw.wpos[par][wave] = k >= 0 ? wave * 64 + k : kNo;
      if (k >= 0 && lane == k) {
        bw.wout[par][wave][0] = o.x;
        bw.wout[par][wave][1] = o.y;
        bw.wout[par][wave][2] = o.z;
      }
    } else {
      ++ws.coop;
      const int i = pos + wave * E + e;
      const bool act = e < E && i < nvalid;
      const DepRec ri = bw.rec[i < nvalid ? i : pos];
      V3 oc = c;
      bool hg = false;
#if RC_STAMPS
      Stamps stq = {{0, 0, 0, 0}, 0};
#define RC_SPEC1(GT, Q) carry_path_spec<GT, Q>(sc, ls, kself, G, half, ri, maxrec, c, zero, hg, &stq)
#else
#define RC_SPEC1(GT, Q) carry_path_spec<GT, Q>(sc, ls, kself, G, half, ri, maxrec, c, zero, hg)
#endif
#define RC_SPEC(GT) \
  (sc.has_quadric ? (quad_x0(sc) ? RC_SPEC1(GT, 2) : RC_SPEC1(GT, 1)) : RC_SPEC1(GT, 0))
      if (act) {
        if (G == 8) oc = RC_SPEC(8);
        else if (G == 4) oc = RC_SPEC(4);
        else if (G == 16) oc = RC_SPEC(16);
        else if (spec) oc = RC_SPEC(0);
        else oc = carry_path_coop(sc, ls, kself, G, ri, maxrec, c, zero, hg);
      }
#undef RC_SPEC
#undef RC_SPEC1
#if RC_STAMPS
      ws.ce += __builtin_amdgcn_s_memtime() - top_;
#endif
      if (act && (lane % GE) == 0) bw.hit[i] = hg ? 1 : 0;
      const unsigned long long mc = __ballot(act && (lane % GE) == 0 && !RC_WIN_SAME(oc, c));
      const int g = mc ? (__ffsll((long long)mc) - 1) / GE : -1;
      if (lane == 0) bw.wpos[par][wave] = g >= 0 ? pos + wave * E + g : kNo;
      if (g >= 0 && lane == g * GE) {
        bw.wout[par][wave][0] = oc.x;
        bw.wout[par][wave][1] = oc.y;
        bw.wout[par][wave][2] = oc.z;
      }
    }
#if RC_STAMPS
    const unsigned long long bw1_ = __builtin_amdgcn_s_memtime();
#endif
    __syncthreads();
#if RC_STAMPS
    ws.cw += __builtin_amdgcn_s_memtime() - bw1_;
#endif
    int wb = 0;
    int best = bw.wpos[par][0];
    for (int q = 1; q < 4; ++q) {
      const int v = bw.wpos[par][q];
      if (v < best) {
        best = v;
        wb = q;
      }
    }
    hit = best != kNo;
    if (hit) {
      last = best;
      cn = v3(bw.wout[par][wb][0], bw.wout[par][wb][1], bw.wout[par][wb][2]);
    } else {
      last = coop ? (pos + Eb < nvalid ? pos + Eb : nvalid) - 1 : nvalid - 1;
    }
    {   // entries pos..last of this window read carry c: each wave publishes its 64-entry slice
      const int w0 = wave * 64;
      const int lo = pos - w0 > 0 ? pos - w0 : 0;
      const int hi = last + 1 - w0 < 64 ? last + 1 - w0 : 64;
      const unsigned long long hm = __ballot(bw.hit[t] != 0);
      if (lo < hi) cin_put_wave_uniform(cin, base + w0, lo, hi, c, tag, hm);
    }
    if (hp) {   // keep the predictor's history across the non-predictive steps
      if (!hit || last > pos) hp->n = 0;
      if (hit) {
        if (hp->n == 0) hist_push(*hp, c);
        hist_push(*hp, cn);
      }
    }
    pos = last + 1;
    c = cn;
    par ^= 1;
    if (hit) {
      changed = true;
      ++ws.changers;
      coop = G > 0;
      clean_run = 0;
    } else if (coop) {
      if (++clean_run >= K) {
        coop = false;
        if (stop) {   // the cluster is over: the team scans on from pos
          stopped = pos;
          break;
        }
      }
    }
  }
#if RC_STAMPS
  if (top_) ws.cs += __builtin_amdgcn_s_memtime() - top_;
#endif
  dense = coop;
  return stopped;
}

}  // namespace rc
