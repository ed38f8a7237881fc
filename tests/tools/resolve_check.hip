// resolve_check.hip — test-only device harness of the carry resolver (rc_device.hpp: carry_path,
// carry_path_coop, carry_path_spec; rc_resolve.hpp: wave_window, block_window, the carry-in
// granules), for tests/test_gpu_resolve.py.  Three entries, one kernel launch each:
//   rv_eval         n cases (primary direction, carry-in) through one form of the evaluator, the
//                   lanes laid out as the windows lay them out;
//   rv_wave_chain   chains of entries through the product's wave_window, one wave a chain, stepped
//                   from window to window as k_resolve's regular waves step;
//   rv_block_chain  the same through block_window, one 256-thread workgroup a chain, in its three
//                   uses (whole-workgroup regular segments, the helpers' predictive step, the team
//                   leader's early stop).
// Every lane first runs phase A's shoot<kModeParityA> on its primary direction, which leaves the
// DEP record exactly as k_phase_a leaves it.  Compiled with the product's HIPFLAGS; the product
// library never links it.
//
// RV_WRONG = 1..4 builds a wrong variant (tests/build/libresolvecheck_w<k>.so), which the suite
// must catch: 1 the windows compare carries with == instead of bit for bit; 2 the speculative
// evaluator's arg-min lets the highest index win among equal t; 3 it keeps the skipped shape
// after a missed level; 4 the predictive step accepts a guess one ulp from the exact carry.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#ifndef RV_WRONG
#define RV_WRONG 0
#endif
#if RV_WRONG == 2
#define RC_ARGMIN_KEY(k) ((k) == 0x7fffffff ? 0x7fffffffu : 1023u - (unsigned)(k))
#define RC_ARGMIN_UNKEY(kb) ((kb) == 0x7fffffffu ? 0x7fffffff : 1023 - (int)(kb))
#endif
#if RV_WRONG == 3
#define RC_SKIP_AFTER_MISS S
#endif

#include "raycast_hip.h"
#include "rc_device.hpp"
#include "rc_kernels.h"
#include "rc_scene.h"

#if RV_WRONG == 1
namespace rc {
__device__ __forceinline__ bool rv_same_eq(V3 a, V3 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
}
#define RC_WIN_SAME(a, b) rv_same_eq(a, b)
#endif
#if RV_WRONG == 4
namespace rc {
__device__ __forceinline__ bool rv_near1(float a, float b) {
  const int d = (int)(__float_as_uint(a) - __float_as_uint(b));
  return d >= -1 && d <= 1;
}
__device__ __forceinline__ bool rv_same_ulp(V3 a, V3 b) {
  return rv_near1(a.x, b.x) && rv_near1(a.y, b.y) && rv_near1(a.z, b.z);
}
}
#define RC_GUESS_SAME(a, b) rv_same_ulp(a, b)
#endif

#include "rc_resolve.hpp"

using namespace rc;

namespace {

constexpr unsigned kTag = 0x2468aceu;   // the harness's carry-in tag (an epoch: below 2^31)
constexpr int kStopMax = 63;            // stop positions reported per chain

struct Staged {
  rc_shape s[kLdsShapesMax + 1];
};

// k_resolve<true>'s staging: n <= kLdsShapesMax shapes in LDS, every record read goes there
__device__ __forceinline__ void stage_shapes(Scene& sc, Staged& st) {
  if (sc.n <= kLdsShapesMax) {
    const int words = (int)(sizeof(rc_shape) / 4) * (sc.n + 1);
    for (int i = threadIdx.x; i < words; i += blockDim.x)
      ((unsigned*)st.s)[i] = ((const unsigned*)sc.shapes)[i];
    __syncthreads();
    sc.shapes = st.s;
    sc.lshapes = st.s;
  }
}

__device__ __forceinline__ LaneShape lane_shape(const Scene& sc, int G) {
  LaneShape ls;
  ls.has = false;
  if (G > 0) {
    const int kself = (threadIdx.x & 63) % G;
    ls.has = kself < sc.n;
    if (ls.has) ls.s = sc.shapes[kself];
  }
  return ls;
}

// phase A on one primary direction: the class and, for a DEP pixel, its record
__device__ __forceinline__ DepRec phase_a(Scene sc, int kq, bool in, const float* d, int i,
                                          int maxrec, int& cls) {
  DepRec r;
  memset(&r, 0, sizeof r);
  cls = -1;
  if (in) {
    sc.has_quadric = kq != 0;   // the record does not depend on the quadric form
    PixelOut po;
    po.cls = kClsIdent;
    po.rgb = v3(0.0f, 0.0f, 0.0f);
    int ze = 0;
    shoot<kModeParityA>(sc, v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]), maxrec, v3(0.0f, 0.0f, 0.0f),
                        po, ze);
    cls = po.cls;
    if (po.cls == kClsDep) r = po.dep;
  }
  return r;
}

// FORM 0: carry_path, one entry a lane.  1: carry_path_coop, G lanes an entry.  2:
// carry_path_spec<GT, kQ>, 2G lanes an entry (GT = 0: the runtime G).  A wave takes 64 cases at a
// time: every lane shoots its own, then the groups take entries s * E + e in GE steps.
template <int FORM, int GT, int kQ>
__global__ void __launch_bounds__(256) k_eval(Scene sc, int kq, int n, int maxrec, const float* d,
                                              const float* cin, int G, float* out, int* hit,
                                              int* cls) {
  __shared__ Staged st;
  stage_shapes(sc, st);
  sc.has_quadric = kq;
  const LaneShape ls = lane_shape(sc, G);
  const int lane = threadIdx.x & 63;
  const int nw = (int)gridDim.x * 4;
  int zero = 0;
  for (int ch = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6); ch * 64 < n; ch += nw) {
    const int i = ch * 64 + lane;
    const bool in = i < n;
    int cl;
    const DepRec r = phase_a(sc, kq, in, d, i, maxrec, cl);
    if (in) cls[i] = cl;
    const bool dep = in && cl == kClsDep;
    const V3 c = in ? v3(cin[3 * i], cin[3 * i + 1], cin[3 * i + 2]) : v3(0.0f, 0.0f, 0.0f);
    if (FORM == 0) {
      if (dep) {
        bool h = false;
        const V3 o = carry_path(sc, r, maxrec, c, zero, h);
        out[3 * i] = o.x; out[3 * i + 1] = o.y; out[3 * i + 2] = o.z;
        hit[i] = h ? 1 : 0;
      }
      continue;
    }
    const int GE = FORM == 2 ? 2 * G : G, E = 64 / GE;
    const int e = lane / GE, kself = lane % G, half = FORM == 2 ? (lane / G) & 1 : 0;
    for (int s = 0; s < GE; ++s) {
      const int idx = s * E + e;
      const DepRec ri = shfl_rec(r, idx);
      const V3 ce = v3(__shfl(c.x, idx, 64), __shfl(c.y, idx, 64), __shfl(c.z, idx, 64));
      const bool act = __shfl((int)dep, idx, 64) != 0;
      V3 oc = ce;
      bool hg = false;
      if (act) {
        if (FORM == 1) oc = carry_path_coop(sc, ls, kself, G, ri, maxrec, ce, zero, hg);
        else oc = carry_path_spec<GT, kQ>(sc, ls, kself, G, half, ri, maxrec, ce, zero, hg);
      }
      if (act && lane % GE == 0) {
        const int o = ch * 64 + idx;
        out[3 * o] = oc.x; out[3 * o + 1] = oc.y; out[3 * o + 2] = oc.z;
        hit[o] = hg ? 1 : 0;
      }
    }
  }
}

// The chains' records: entry j of the launch at line j (dep_pix is the identity), written by the
// chain's own threads before its first window.
__device__ __forceinline__ void chain_records(const Scene& sc, int kq, int j0, int j1,
                                              const float* d, int maxrec, DepLine* line,
                                              long long* dep_pix, int* cls) {
  for (int j = j0 + (int)threadIdx.x; j < j1; j += (int)blockDim.x) {
    int cl;
    DepLine l;
    memset(&l, 0, sizeof l);
    l.r = phase_a(sc, kq, true, d, j, maxrec, cl);
    line[j] = l;
    dep_pix[j] = j;
    cls[j] = cl;
  }
  __threadfence();
  __syncthreads();
}

// One wave a chain: k_resolve's regular-wave loop over a segment, without the hand-off to a helper.
// stats: lane passes, cooperative steps, changers, evaluation steps.
__global__ void __launch_bounds__(64) k_wave_chain(Scene sc, int kq, const int* offs, int maxrec,
                                                   const float* d, const float* init, int G, int K,
                                                   DepLine* line, long long* dep_pix, CinG* cin,
                                                   float* mine_out, int* mhit_out, float* fin,
                                                   int* stats, int* cls) {
  __shared__ Staged st;
  __shared__ float s_stage[192];
  stage_shapes(sc, st);
  const int q = (int)blockIdx.x, start = offs[q], end = offs[q + 1];
  chain_records(sc, kq, start, end, d, maxrec, line, dep_pix, cls);
  sc.has_quadric = kq;
  const LaneShape ls = lane_shape(sc, G);
  const int lane = threadIdx.x & 63;
  int iters = 0;
  V3 c = v3(init[3 * q], init[3 * q + 1], init[3 * q + 2]);
  bool dense = false;
  WinStats ws = {0, 0, 0};
  CarryHist hs;
  hs.n = 0;
  hs.run = 0;
#if RC_STAMPS
  Stamps stp = {{0, 0, 0, 0}, 0};
#endif
  for (int j = start; j < end; j += 64) {
    V3 mine;
    bool mhit, changed;
    iters += wave_window(sc, maxrec, line, dep_pix, j, end, c, mine, mhit, ls, G, dense, changed,
                         ws, K, hs
#if RC_STAMPS
                         , &stp
#endif
                         );
    const unsigned long long hm = __ballot(j + lane < end && mhit);
    cin_put_wave(cin, j, 0, end - j < 64 ? end - j : 64, mine, kTag, hm, s_stage);
    if (j + lane < end) {
      mine_out[3 * (j + lane)] = mine.x;
      mine_out[3 * (j + lane) + 1] = mine.y;
      mine_out[3 * (j + lane) + 2] = mine.z;
      mhit_out[j + lane] = mhit ? 1 : 0;
    }
  }
  if (lane == 0) {
    fin[3 * q] = c.x; fin[3 * q + 1] = c.y; fin[3 * q + 2] = c.z;
    stats[4 * q] = ws.lane; stats[4 * q + 1] = ws.coop; stats[4 * q + 2] = ws.changers;
    stats[4 * q + 3] = iters;
  }
}

// One workgroup a chain through block_window over 256-entry windows.  mode 0: a whole-workgroup
// regular segment (starts in LANE mode, no predictor).  1: a helper's item (starts dense, with
// the CarryHist hn / hist of the hand-off).  2: the team leader (starts dense, stop = true); a
// stopped window's rest and what follows it up to 256 entries go through one plain call, then the
// leader's way goes on; stops[0] counts the stops, stops[1..] are the entries they stopped at.
__global__ void __launch_bounds__(kResolveBlock) k_block_chain(
    Scene sc, int kq, const int* offs, int maxrec, const float* d, const float* init, int G, int K,
    int mode, const int* hn, const float* hist, DepLine* line, long long* dep_pix, CinG* cin,
    float* fin, int* stats, int* stops, int* cls) {
  __shared__ Staged st;
  __shared__ BlockWinShared s_bw;
  stage_shapes(sc, st);
  const int q = (int)blockIdx.x, start = offs[q], end = offs[q + 1];
  chain_records(sc, kq, start, end, d, maxrec, line, dep_pix, cls);
  sc.has_quadric = kq;
  const LaneShape ls = lane_shape(sc, G);
  const int t = threadIdx.x;
  V3 c = v3(init[3 * q], init[3 * q + 1], init[3 * q + 2]);
  bool dense = mode != 0;
  WinStats ws = {0, 0, 0};
  CarryHist hs;
  hs.n = mode == 1 ? hn[q] : 0;
  hs.run = 0;
  for (int k = 0; k < 4; ++k)
    hs.h[k] = mode == 1 ? v3(hist[12 * q + 3 * k], hist[12 * q + 3 * k + 1], hist[12 * q + 3 * k + 2])
                        : v3(0.0f, 0.0f, 0.0f);
  int nstop = 0;
  bool plain = false;   // mode 2: the window after a stop
  int j = start;
  while (j < end) {
    const int nv = end - j < kResolveBlock ? end - j : kResolveBlock;
    __syncthreads();   // everyone is done reading the window before
    if (t < nv) s_bw.rec[t] = rec_at(line, dep_pix, j + t);
    __syncthreads();
    bool changed;
    const int stop = block_window(sc, maxrec, s_bw, j, nv, c, ls, G, dense, changed, K, cin, kTag,
                                  ws, mode == 1 ? &hs : nullptr, mode == 2 && !plain);
    plain = false;
    if (stop >= 0) {
      if (t == 0 && nstop < kStopMax) stops[(kStopMax + 1) * q + 1 + nstop] = j + stop;
      ++nstop;
      j += stop;
      plain = true;
    } else {
      j += nv;
    }
  }
  if (t == 0) {
    fin[3 * q] = c.x; fin[3 * q + 1] = c.y; fin[3 * q + 2] = c.z;
    stats[4 * q] = ws.lane; stats[4 * q + 1] = ws.coop; stats[4 * q + 2] = ws.changers;
    stats[4 * q + 3] = ws.lane + ws.coop;
    stops[(kStopMax + 1) * q] = nstop;
  }
}

struct RvScene {
  rc_packed_header* host;
  char* dev;
  int hasq, cross;
};

#define RV_TRY(x)                         \
  do {                                    \
    const hipError_t e_ = (x);            \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

struct Bufs {
  void* p[20];
  int n = 0;
  ~Bufs() {
    for (int k = 0; k < n; ++k) (void)hipFree(p[k]);
  }
  hipError_t get(void** out, const void* src, size_t bytes) {
    *out = nullptr;
    if (n >= 20) return hipErrorOutOfMemory;
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, bytes ? bytes : 4);
    if (e != hipSuccess) return e;
    p[n++] = d;
    *out = d;
    if (src) return hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
    return hipMemset(d, 0, bytes ? bytes : 4);
  }
};

// the resolver's Scene: as launch_parity's make_scene, has_quadric set by the kernels
Scene device_scene(const RvScene* s) {
  const rc_packed_header* h = s->host;
  const rc_shape* hs = (const rc_shape*)((const char*)h + h->off_shapes);
  Scene sc;
  memset(&sc, 0, sizeof sc);
  sc.shapes = (const rc_shape*)(s->dev + h->off_shapes);
  sc.lights = (const rc_light*)(s->dev + h->off_lights);
  sc.pairs = (const rc_shade_pair*)(s->dev + h->off_pairs);
  sc.lshapes = sc.shapes;
  sc.lpairs = sc.pairs;
  sc.n = h->n;
  sc.m = h->m;
  for (int k = 0; k < h->n && k < 64; ++k)
    if (hs[k].refl > 0.0f) sc.refl_mask |= 1ull << k;
  sc.has_quadric = s->hasq;
  sc.o0_ok = h->o0_ok;
  sc.dep_fast = !(hs[h->n].opacity > 0.0f);
  for (int k = 0; k < h->n; ++k)
    if (!(fabsf(hs[k].refl) < 1.0e5f)) sc.dep_fast = 0;
  sc.pin = 0;
  return sc;
}

// kq: 0 = the scene has no quadric, 1 = it has, 2 = the cross-term-free form (no cross terms)
bool kq_ok(const RvScene* s, int kq) {
  if (!s->hasq) return kq == 0;
  return kq == 1 || (kq == 2 && !s->cross);
}
// G: 0 (no cooperative evaluator) or a power of two in 2..64 that holds the scene's shapes
bool group_ok(const RvScene* s, int G) {
  if (G == 0) return true;
  return G >= 2 && G <= 64 && (G & (G - 1)) == 0 && G >= s->host->n;
}

template <int FORM, int GT>
void launch_eval(int kq, int blocks, Scene sc, int n, int maxrec, const float* d, const float* c,
                 int G, float* o, int* h, int* cl) {
  if (FORM != 2) k_eval<FORM, 0, 0><<<blocks, 256>>>(sc, kq, n, maxrec, d, c, G, o, h, cl);
  else if (kq == 0) k_eval<2, GT, 0><<<blocks, 256>>>(sc, kq, n, maxrec, d, c, G, o, h, cl);
  else if (kq == 1) k_eval<2, GT, 1><<<blocks, 256>>>(sc, kq, n, maxrec, d, c, G, o, h, cl);
  else k_eval<2, GT, 2><<<blocks, 256>>>(sc, kq, n, maxrec, d, c, G, o, h, cl);
}

}  // namespace

extern "C" {

int rv_wrong(void) { return RV_WRONG; }

void* rv_scene_create(const json_data_t* js) {
  rc_packed_header* h = rc_pack_scene(js);
  if (!h) return nullptr;
  RvScene* s = (RvScene*)calloc(1, sizeof *s);
  if (!s) { free(h); return nullptr; }
  s->host = h;
  const rc_shape* hs = (const rc_shape*)((const char*)h + h->off_shapes);
  for (int k = 0; k < h->n; ++k)
    if (hs[k].type == RC_SHAPE_QUADRIC) {
      s->hasq = 1;
      if (hs[k].qd != 0.0f || hs[k].qe != 0.0f || hs[k].qf != 0.0f) s->cross = 1;
    }
  if (hipMalloc((void**)&s->dev, (size_t)h->bytes) != hipSuccess ||
      hipMemcpy(s->dev, h, (size_t)h->bytes, hipMemcpyHostToDevice) != hipSuccess) {
    if (s->dev) (void)hipFree(s->dev);
    free(h);
    free(s);
    return nullptr;
  }
  return s;
}

void rv_scene_destroy(void* sp) {
  RvScene* s = (RvScene*)sp;
  if (!s) return;
  (void)hipFree(s->dev);
  free(s->host);
  free(s);
}

// shapes, whether one is a quadric, whether a quadric has cross terms
void rv_scene_info(const void* sp, int* n, int* has_quadric, int* cross) {
  const RvScene* s = (const RvScene*)sp;
  *n = s->host->n;
  *has_quadric = s->hasq;
  *cross = s->cross;
}

// n cases (primary direction d, carry-in c: 3 floats each) through one form of the evaluator:
// form 0 carry_path; 1 carry_path_coop with groups of G lanes; 2 carry_path_spec with two groups
// of G lanes an entry, G = 4, 8, 16 as the template constant and 32 as the runtime value.  Out:
// cls (phase A's class of the primary ray), and where it is DEP (2) the carry-out and the hit
// flag.  -2: arguments the library's dispatch could not produce.
int rv_eval(const void* sp, int form, int G, int kq, int n, int maxrec, const float* d,
            const float* carry_in, float* carry_out, int* hit, int* cls) {
  const RvScene* s = (const RvScene*)sp;
  if (!s || n < 0 || maxrec < 1 || maxrec > 64 || form < 0 || form > 2 || !kq_ok(s, kq)) return -2;
  if (form == 0 ? G != 0 : (G == 0 || !group_ok(s, G))) return -2;
  if (form == 2 && !(G == 4 || G == 8 || G == 16 || G == 32)) return -2;
  if (n == 0) return 0;
  Bufs bf;
  void *dD, *dI, *dO, *dH, *dC;
  RV_TRY(bf.get(&dD, d, (size_t)n * 12));
  RV_TRY(bf.get(&dI, carry_in, (size_t)n * 12));
  RV_TRY(bf.get(&dO, nullptr, (size_t)n * 12));
  RV_TRY(bf.get(&dH, nullptr, (size_t)n * 4));
  RV_TRY(bf.get(&dC, nullptr, (size_t)n * 4));
  const Scene sc = device_scene(s);
  const int chunks = (n + 63) / 64;
  const int blocks = chunks < 128 ? (chunks + 3) / 4 : 32;   // at most 8192 threads a launch
  const float *pd = (const float*)dD, *pi = (const float*)dI;
  float* po = (float*)dO;
  int *ph = (int*)dH, *pc = (int*)dC;
  if (form == 0) launch_eval<0, 0>(kq, blocks, sc, n, maxrec, pd, pi, G, po, ph, pc);
  else if (form == 1) launch_eval<1, 0>(kq, blocks, sc, n, maxrec, pd, pi, G, po, ph, pc);
  else if (G == 4) launch_eval<2, 4>(kq, blocks, sc, n, maxrec, pd, pi, G, po, ph, pc);
  else if (G == 8) launch_eval<2, 8>(kq, blocks, sc, n, maxrec, pd, pi, G, po, ph, pc);
  else if (G == 16) launch_eval<2, 16>(kq, blocks, sc, n, maxrec, pd, pi, G, po, ph, pc);
  else launch_eval<2, 0>(kq, blocks, sc, n, maxrec, pd, pi, G, po, ph, pc);
  RV_TRY(hipGetLastError());
  RV_TRY(hipDeviceSynchronize());
  RV_TRY(hipMemcpy(carry_out, dO, (size_t)n * 12, hipMemcpyDeviceToHost));
  RV_TRY(hipMemcpy(hit, dH, (size_t)n * 4, hipMemcpyDeviceToHost));
  RV_TRY(hipMemcpy(cls, dC, (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
}

// nch chains: chain q holds the entries offs[q] .. offs[q + 1] - 1 of d (offs[0] = 0) and starts
// from the carry init[3 q ..].  mode -1: one wave a chain through wave_window (G lanes a group, 0 =
// LANE passes only; K = rc_tuning.wave_k).  mode 0, 1, 2: one workgroup a chain through
// block_window (k_block_chain; hn / hist: the helpers' CarryHist, mode 1 only).  Out, per entry:
// cls, the raw carry-in granules (cin: 3 x 8 bytes, tag rv_tag()), for mode -1 also the window's
// own `mine` and `mhit`; per chain: the final carry, stats (LANE passes, cooperative steps,
// changers, evaluation steps) and for mode 2 stops (64 ints: the count, then the entries).
unsigned rv_tag(void) { return kTag; }

int rv_chain(const void* sp, int mode, int G, int K, int kq, int nch, const int* offs, int maxrec,
             const float* d, const float* init, const int* hn, const float* hist,
             unsigned long long* cin, float* mine, int* mhit, float* fin, int* stats, int* stops,
             int* cls) {
  const RvScene* s = (const RvScene*)sp;
  if (!s || nch < 1 || nch > 64 || maxrec < 1 || maxrec > 64 || mode < -1 || mode > 2 || K < 1 ||
      K > 64 || !kq_ok(s, kq) || !group_ok(s, G) || offs[0] != 0)
    return -2;
  for (int q = 0; q < nch; ++q)
    if (offs[q + 1] < offs[q]) return -2;
  if (mode == 1 && (!hn || !hist)) return -2;
  for (int q = 0; mode == 1 && q < nch; ++q)
    if (hn[q] < 0 || hn[q] > 4) return -2;
  const int n = offs[nch];
  if (n == 0) return -2;
  Bufs bf;
  void *dOf, *dD, *dI, *dHn, *dHi, *dL, *dP, *dG, *dM, *dMh, *dF, *dS, *dSt, *dC;
  RV_TRY(bf.get(&dOf, offs, (size_t)(nch + 1) * 4));
  RV_TRY(bf.get(&dD, d, (size_t)n * 12));
  RV_TRY(bf.get(&dI, init, (size_t)nch * 12));
  RV_TRY(bf.get(&dHn, mode == 1 ? hn : nullptr, (size_t)nch * 4));
  RV_TRY(bf.get(&dHi, mode == 1 ? hist : nullptr, (size_t)nch * 48));
  RV_TRY(bf.get(&dL, nullptr, (size_t)n * sizeof(DepLine)));
  RV_TRY(bf.get(&dP, nullptr, (size_t)n * 8));
  RV_TRY(bf.get(&dG, nullptr, ((size_t)n + 64) * sizeof(CinG)));
  RV_TRY(bf.get(&dM, nullptr, (size_t)n * 12));
  RV_TRY(bf.get(&dMh, nullptr, (size_t)n * 4));
  RV_TRY(bf.get(&dF, nullptr, (size_t)nch * 12));
  RV_TRY(bf.get(&dS, nullptr, (size_t)nch * 16));
  RV_TRY(bf.get(&dSt, nullptr, (size_t)nch * (kStopMax + 1) * 4));
  RV_TRY(bf.get(&dC, nullptr, (size_t)n * 4));
  const Scene sc = device_scene(s);
  if (mode < 0)
    k_wave_chain<<<nch, 64>>>(sc, kq, (const int*)dOf, maxrec, (const float*)dD, (const float*)dI, G,
                              K, (DepLine*)dL, (long long*)dP, (CinG*)dG, (float*)dM, (int*)dMh,
                              (float*)dF, (int*)dS, (int*)dC);
  else
    k_block_chain<<<nch, kResolveBlock>>>(sc, kq, (const int*)dOf, maxrec, (const float*)dD,
                                          (const float*)dI, G, K, mode, (const int*)dHn,
                                          (const float*)dHi, (DepLine*)dL, (long long*)dP,
                                          (CinG*)dG, (float*)dF, (int*)dS, (int*)dSt, (int*)dC);
  RV_TRY(hipGetLastError());
  RV_TRY(hipDeviceSynchronize());
  RV_TRY(hipMemcpy(cin, dG, (size_t)n * sizeof(CinG), hipMemcpyDeviceToHost));
  RV_TRY(hipMemcpy(mine, dM, (size_t)n * 12, hipMemcpyDeviceToHost));
  RV_TRY(hipMemcpy(mhit, dMh, (size_t)n * 4, hipMemcpyDeviceToHost));
  RV_TRY(hipMemcpy(fin, dF, (size_t)nch * 12, hipMemcpyDeviceToHost));
  RV_TRY(hipMemcpy(stats, dS, (size_t)nch * 16, hipMemcpyDeviceToHost));
  RV_TRY(hipMemcpy(stops, dSt, (size_t)nch * (kStopMax + 1) * 4, hipMemcpyDeviceToHost));
  RV_TRY(hipMemcpy(cls, dC, (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
