// prim_check.hip — TEST INFRASTRUCTURE ONLY (tests/test_gpu_prims.py, `make primcheck`).
//
// Runs the product's own device routines (rc_device.hpp, rc_cudasem.hpp: the very functions the
// kernels inline, compiled with the product's flags) one thread per case, so the tests can
// compare them ray by ray with the CPU oracle and with numpy.  The shape records come from
// rc_pack_scene (rc_scene.o), which computes o0, r2 and inv_r.  Every entry copies its host
// arrays to the device, makes ONE launch and copies the results back; it returns 0, a HIP
// error code, or -2 for an argument it refuses (a shape index outside the scene).
//
// The three *_mut routines below are deliberately wrong copies of product routines:
// the tests require the case lists to tell each of them from the reference.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "raycast_hip.h"
#include "rc_cudasem.hpp"
#include "rc_device.hpp"
#include "rc_scene.h"

using namespace rc;

namespace {

// --------------------------------------------------------------------- mutants --
// div_nr's reciprocal with ONE Newton step
__device__ __forceinline__ double recip_nr_mut(double d) {
  double y = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, y, 1.0);
  return __builtin_fma(y, e, y);
}
// sqrt_ns without its second correction step
__device__ __forceinline__ double sqrt_ns_mut(double s) {
  const double y = __builtin_amdgcn_rsq(s);
  double g = s * y, h = y * 0.5;
  const double r = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, r, g);
  h = __builtin_fma(h, r, h);
  double d = __builtin_fma(-g, g, s);
  g = __builtin_fma(d, h, g);
  return (s == 0.0 || s == __builtin_inf()) ? s : g;
}
// quot_class with the upper exponent bound 127 in place of 126
__device__ __forceinline__ int quot_class_mut(double num, double den) {
  const unsigned hn = (unsigned)__double2hiint(num), hd = (unsigned)__double2hiint(den);
  const int en = (int)((hn >> 20) & 0x7ffu), ed = (int)((hd >> 20) & 0x7ffu);
  const int e = en - ed;
  if (en != 0 && en != 0x7ff && ed != 0 && ed != 0x7ff && e >= -148 && e <= 127)
    return ((hn ^ hd) >> 31) ? kQNeg : kQPos;
  const float t = (float)(num / den);
  if (t < 0.0f) return kQNeg;
  if (t == 0.0f) return kQZero;
  return t < __builtin_inff() ? kQPos : kQOther;
}

// --------------------------------------------------------------------- scalars --
enum {
  kOpDiv = 0,      // a = num, b = den (f64 bits) -> o0 = div_nr(n, d, recip_nr(d)), o1 = tquot (f32)
  kOpDivMut,       //   the same through recip_nr_mut
  kOpSqrt,         // a = s -> o0 = sqrt_ns(s)
  kOpSqrtMut,
  kOpLength,       // a = xyz (3 f32) -> o1 = length
  kOpDiv3,         // a = xyz (3 f32), b = len (f32) -> o1 = 3 f32
  kOpPow20,        // a = x (f64) -> o0
  kOpPown,         // a = x (f64), b = n (i32) -> o0
  kOpQuotClass,    // a = num, b = den (f64) -> o1 = class (i32)
  kOpQuotClassMut,
  kOpX0Reject,     // a = O (3 f32), b = D (3 f32) -> o1 = 0/1 (i32)
  kOpCount
};

__global__ void k_scalar(int op, int n, const void* a, const void* b, void* o0, void* o1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* ad = (const double*)a;
  const double* bd = (const double*)b;
  const float* af = (const float*)a;
  const float* bf = (const float*)b;
  double* od = (double*)o0;
  float* of = (float*)o1;
  int* oi = (int*)o1;
  switch (op) {
    case kOpDiv: {
      const double y = recip_nr(bd[i]);
      od[i] = div_nr(ad[i], bd[i], y);
      of[i] = tquot(ad[i], bd[i], y);
      break;
    }
    case kOpDivMut: {
      const double y = recip_nr_mut(bd[i]);
      od[i] = div_nr(ad[i], bd[i], y);
      of[i] = (float)div_nr(ad[i], bd[i], y);
      break;
    }
    case kOpSqrt: od[i] = sqrt_ns(ad[i]); break;
    case kOpSqrtMut: od[i] = sqrt_ns_mut(ad[i]); break;
    case kOpLength: of[i] = length(v3(af[3 * i], af[3 * i + 1], af[3 * i + 2])); break;
    case kOpDiv3: {
      const V3 q = div3(v3(af[3 * i], af[3 * i + 1], af[3 * i + 2]), bf[i]);
      of[3 * i] = q.x;
      of[3 * i + 1] = q.y;
      of[3 * i + 2] = q.z;
      break;
    }
    case kOpPow20: od[i] = pow20(ad[i]); break;
    case kOpPown: od[i] = pown_dd(ad[i], ((const int*)b)[i]); break;
    case kOpQuotClass: oi[i] = quot_class(ad[i], bd[i]); break;
    case kOpQuotClassMut: oi[i] = quot_class_mut(ad[i], bd[i]); break;
    case kOpX0Reject:
      oi[i] = x0_reject(v3(af[3 * i], af[3 * i + 1], af[3 * i + 2]),
                        v3(bf[3 * i], bf[3 * i + 1], bf[3 * i + 2])) ? 1 : 0;
      break;
    default: break;
  }
}

// ---------------------------------------------------------------------- shapes --
enum {
  kFormTest = 0,      // test_shape, cross terms as written
  kFormTestX0,        // test_shape in the cross-term-free form (quad_x0) with x0_reject
  kFormO0,            // hit_*_o0 (O = 0 is implied; the O array is not read)
  kFormO0X0,
  kFormShadow,        // shadow_sphere / the plane's shadow rule / shadow_quadric
  kFormShadowX0,
  kFormUniNoQuad,     // test_unified<false>
  kFormUniQuad,       // test_unified<true, false>
  kFormUniQuadX0,     // test_unified<true, true> with x0_reject, as carry_path_spec calls it
  kFormCuda,          // cusem::cu_test
  kFormCount
};

__device__ __forceinline__ V3 ld3(const float* p, int i) {
  return v3(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
}

__global__ void k_shape(const rc_shape* shapes, int form, int n, const float* Oa, const float* Da,
                        const int* shape, const int* skipa, int* hit, float* tout) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const rc_shape& s = shapes[shape[i]];
  const V3 O = form == kFormO0 || form == kFormO0X0 ? v3(0.0f, 0.0f, 0.0f) : ld3(Oa, i);
  const V3 D = ld3(Da, i);
  const int skip = skipa[i];
  const RayK rk = ray_consts(D);
  float t = 0.0f;
  bool h = false;
  switch (form) {
    case kFormTest: h = test_shape(s, O, D, rk, skip, t); break;
    case kFormTestX0: h = test_shape(s, O, D, rk, skip, t, true, x0_reject(O, D)); break;
    case kFormO0:
    case kFormO0X0: {
      const bool x0 = form == kFormO0X0;
      if (s.type == RC_SHAPE_SPHERE) h = hit_sphere_o0(D, s, rk, t);
      else if (s.type == RC_SHAPE_PLANE) h = hit_plane_o0(D, s, t);
      else if (s.type == RC_SHAPE_QUADRIC)
        h = hit_quadric_o0(D, s, t, x0) && !(x0 && x0_reject(O, D));
      break;
    }
    case kFormShadow:
    case kFormShadowX0: {
      const bool x0 = form == kFormShadowX0;
      if (s.type == RC_SHAPE_SPHERE) h = shadow_sphere(O, D, s, rk);
      else if (s.type == RC_SHAPE_PLANE)
        h = hit_plane(O, D, s, t) && __builtin_inff() > t && t > 0.0f;
      else if (s.type == RC_SHAPE_QUADRIC)
        h = shadow_quadric(O, D, s, skip, x0, x0 && x0_reject(O, D));
      t = 0.0f;   // a shadow form has no distance
      break;
    }
    case kFormUniNoQuad: h = test_unified<false>(s, O, D, rk, skip, t); break;
    case kFormUniQuad: h = test_unified<true, false>(s, O, D, rk, skip, t); break;
    case kFormUniQuadX0: {
      const bool rejq = (s.type == RC_SHAPE_QUADRIC) & x0_reject(O, D);
      h = test_unified<true, true>(s, O, D, rk, skip, t) & !rejq;
      break;
    }
    case kFormCuda: h = cusem::cu_test(s, O, D, cusem::ray_a(D), skip, t); break;
    default: break;
  }
  hit[i] = h ? 1 : 0;
  tout[i] = t;
}

// ----------------------------------------------------------------------- lists --
enum { kListNearest = 0, kListPrimary, kListShadowed, kListCuNearest, kListCuShadowed, kListCount };

__global__ void k_list(Scene sc, int form, int n, const float* Oa, const float* Da,
                       const int* skipa, int* idx, float* tout) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 O = form == kListPrimary ? v3(0.0f, 0.0f, 0.0f) : ld3(Oa, i);
  const V3 D = ld3(Da, i);
  const int skip = skipa[i];
  float t = 0.0f;
  int k = -1;
  switch (form) {
    case kListNearest: k = nearest(sc, O, D, skip, t); break;
    case kListPrimary: k = nearest_primary(sc, D, t); break;
    case kListShadowed: k = shadowed(sc, O, D, skip) ? 1 : 0; break;
    case kListCuNearest: k = cusem::cu_nearest(sc, O, D, skip, t); break;
    case kListCuShadowed: k = cusem::cu_shadowed(sc, O, D, skip) ? 1 : 0; break;
    default: break;
  }
  idx[i] = k;
  tout[i] = t;
}

// ---------------------------------------------------------------------- frames --
enum { kFrameHit = 0, kFrameSelNoQuad, kFrameSelQuad, kFrameCount };

__global__ void k_frame(Scene sc, int form, int n, const int* shape, const float* Oa,
                        const float* Da, const float* ta, float* Pa, float* Na, int* zero) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 O = ld3(Oa, i), D = ld3(Da, i);
  V3 P = v3(0.0f, 0.0f, 0.0f), N = v3(0.0f, 0.0f, 0.0f);
  int ze = 0;
  if (form == kFrameHit) hit_frame(sc, shape[i], O, D, ta[i], P, N, ze);
  else if (form == kFrameSelNoQuad) hit_frame_sel<false>(sc.lshapes[shape[i]], O, D, ta[i], P, N);
  else if (form == kFrameSelQuad) hit_frame_sel<true>(sc.lshapes[shape[i]], O, D, ta[i], P, N);
  Pa[3 * i] = P.x; Pa[3 * i + 1] = P.y; Pa[3 * i + 2] = P.z;
  Na[3 * i] = N.x; Na[3 * i + 1] = N.y; Na[3 * i + 2] = N.z;
  zero[i] = ze;
}

// ------------------------------------------------------------------- host side --
struct PcScene {
  rc_packed_header* host;
  char* dev;
  int natural_hq;   // 0: no quadric, 1: some quadric has cross terms, 2: none has
};

// device buffers of one call: freed together whatever path leaves the entry
struct Bufs {
  void* p[12];
  int n = 0;
  ~Bufs() {
    for (int k = 0; k < n; ++k) (void)hipFree(p[k]);
  }
  // a device copy of `bytes` bytes of `src` (src NULL: uninitialised-but-zeroed output buffer)
  hipError_t get(void** out, const void* src, size_t bytes) {
    *out = nullptr;
    if (n >= 12) return hipErrorOutOfMemory;
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, bytes ? bytes : 4);
    if (e != hipSuccess) return e;
    p[n++] = d;
    *out = d;
    if (src) return hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
    return hipMemset(d, 0, bytes ? bytes : 4);
  }
};

#define PC_TRY(x)                      \
  do {                                 \
    const hipError_t e_ = (x);         \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

constexpr int kBlock = 256;
inline int grid_of(int n) { return (n + kBlock - 1) / kBlock; }

int finish() {
  PC_TRY(hipGetLastError());
  PC_TRY(hipDeviceSynchronize());
  return 0;
}

bool indices_ok(const PcScene* s, int n, const int* shape) {
  for (int i = 0; i < n; ++i)
    if (shape[i] < 0 || shape[i] >= s->host->n) return false;
  return true;
}

Scene scene_of(const PcScene* s, int hq, int o0) {
  Scene sc;
  memset(&sc, 0, sizeof sc);
  sc.shapes = (const rc_shape*)(s->dev + s->host->off_shapes);
  sc.lshapes = sc.shapes;
  sc.n = s->host->n;
  sc.m = 0;   // nothing here shades: lights and pairs stay null
  sc.has_quadric = hq < 0 ? s->natural_hq : hq;
  sc.o0_ok = o0 < 0 ? s->host->o0_ok : o0;
  return sc;
}

}  // namespace

extern "C" {

// Pack (rc_pack_scene) and upload a scene.  NULL on failure.
void* pc_scene_create(const json_data_t* js) {
  rc_packed_header* h = rc_pack_scene(js);
  if (!h) return nullptr;
  PcScene* s = (PcScene*)calloc(1, sizeof *s);
  if (!s) { free(h); return nullptr; }
  s->host = h;
  if (hipMalloc((void**)&s->dev, (size_t)h->bytes) != hipSuccess ||
      hipMemcpy(s->dev, h, (size_t)h->bytes, hipMemcpyHostToDevice) != hipSuccess) {
    if (s->dev) (void)hipFree(s->dev);
    free(h);
    free(s);
    return nullptr;
  }
  const rc_shape* hs = (const rc_shape*)((const char*)h + h->off_shapes);
  bool cross = false;
  for (int k = 0; k < h->n; ++k)
    if (hs[k].type == RC_SHAPE_QUADRIC) {
      s->natural_hq = 1;
      if (hs[k].qd != 0.0f || hs[k].qe != 0.0f || hs[k].qf != 0.0f) cross = true;
    }
  if (s->natural_hq && !cross) s->natural_hq = 2;
  return s;
}

void pc_scene_destroy(void* sp) {
  PcScene* s = (PcScene*)sp;
  if (!s) return;
  (void)hipFree(s->dev);
  free(s->host);
  free(s);
}

// n shapes, the library's has_quadric value (0, 1, 2) and o0_ok for this scene
void pc_scene_info(const void* sp, int* n, int* has_quadric, int* o0_ok) {
  const PcScene* s = (const PcScene*)sp;
  *n = s->host->n;
  *has_quadric = s->natural_hq;
  *o0_ok = s->host->o0_ok;
}

// One scalar primitive (kOp*) over n cases; the arrays' per-case layouts are listed at the enum
// (an array the operation does not use may be NULL).
int pc_scalar(int op, int n, const void* a, const void* b, void* o0, void* o1) {
  // bytes per case of a, b, o0, o1
  static const int kBytes[kOpCount][4] = {
      {8, 8, 8, 4}, {8, 8, 8, 4}, {8, 0, 8, 0}, {8, 0, 8, 0},  {12, 0, 0, 4}, {12, 4, 0, 12},
      {8, 0, 8, 0}, {8, 4, 8, 0}, {8, 8, 0, 4}, {8, 8, 0, 4}, {12, 12, 0, 4}};
  if (op < 0 || op >= kOpCount || n < 0) return -2;
  if (n == 0) return 0;
  const int a_bytes = kBytes[op][0], b_bytes = kBytes[op][1], o0_bytes = kBytes[op][2],
            o1_bytes = kBytes[op][3];
  if (!a || (b_bytes && !b) || (o0_bytes && !o0) || (o1_bytes && !o1)) return -2;
  Bufs bf;
  void *da, *db, *d0, *d1;
  PC_TRY(bf.get(&da, a, (size_t)n * a_bytes));
  PC_TRY(bf.get(&db, b_bytes ? b : nullptr, (size_t)n * b_bytes));
  PC_TRY(bf.get(&d0, nullptr, (size_t)n * o0_bytes));
  PC_TRY(bf.get(&d1, nullptr, (size_t)n * o1_bytes));
  k_scalar<<<grid_of(n), kBlock>>>(op, n, da, db, d0, d1);
  if (int r = finish()) return r;
  if (o0_bytes) PC_TRY(hipMemcpy(o0, d0, (size_t)n * o0_bytes, hipMemcpyDeviceToHost));
  if (o1_bytes) PC_TRY(hipMemcpy(o1, d1, (size_t)n * o1_bytes, hipMemcpyDeviceToHost));
  return 0;
}

// One shape test form (kForm*) for n cases (O, D: 3 floats each; shape index; skip).
int pc_shape(const void* sp, int form, int n, const float* O, const float* D, const int* shape,
             const int* skip, int* hit, float* t) {
  const PcScene* s = (const PcScene*)sp;
  if (!s || form < 0 || form >= kFormCount || n < 0 || !indices_ok(s, n, shape)) return -2;
  if (n == 0) return 0;
  Bufs bf;
  void *dO, *dD, *dS, *dK, *dH, *dT;
  PC_TRY(bf.get(&dO, O, (size_t)n * 12));
  PC_TRY(bf.get(&dD, D, (size_t)n * 12));
  PC_TRY(bf.get(&dS, shape, (size_t)n * 4));
  PC_TRY(bf.get(&dK, skip, (size_t)n * 4));
  PC_TRY(bf.get(&dH, nullptr, (size_t)n * 4));
  PC_TRY(bf.get(&dT, nullptr, (size_t)n * 4));
  k_shape<<<grid_of(n), kBlock>>>((const rc_shape*)(s->dev + s->host->off_shapes), form, n,
                                  (const float*)dO, (const float*)dD, (const int*)dS,
                                  (const int*)dK, (int*)dH, (float*)dT);
  if (int r = finish()) return r;
  PC_TRY(hipMemcpy(hit, dH, (size_t)n * 4, hipMemcpyDeviceToHost));
  PC_TRY(hipMemcpy(t, dT, (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
}

// One whole-list routine (kList*) for n rays.  has_quadric / o0_ok: -1 = the scene's own value,
// else the value to run with (1 forces the cross-term form, 0 forces nearest_primary's fallback).
int pc_list(const void* sp, int form, int has_quadric, int o0_ok, int n, const float* O,
            const float* D, const int* skip, int* idx, float* t) {
  const PcScene* s = (const PcScene*)sp;
  if (!s || form < 0 || form >= kListCount || n < 0) return -2;
  if (has_quadric == 2 && s->natural_hq != 2) return -2;   // quad_x0 needs zero cross terms
  if (n == 0) return 0;
  Bufs bf;
  void *dO, *dD, *dK, *dI, *dT;
  PC_TRY(bf.get(&dO, O, (size_t)n * 12));
  PC_TRY(bf.get(&dD, D, (size_t)n * 12));
  PC_TRY(bf.get(&dK, skip, (size_t)n * 4));
  PC_TRY(bf.get(&dI, nullptr, (size_t)n * 4));
  PC_TRY(bf.get(&dT, nullptr, (size_t)n * 4));
  k_list<<<grid_of(n), kBlock>>>(scene_of(s, has_quadric, o0_ok), form, n, (const float*)dO,
                                 (const float*)dD, (const int*)dK, (int*)dI, (float*)dT);
  if (int r = finish()) return r;
  PC_TRY(hipMemcpy(idx, dI, (size_t)n * 4, hipMemcpyDeviceToHost));
  PC_TRY(hipMemcpy(t, dT, (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
}

// Hit point, normal and zero-normalize count of (shape, O, D, t) through one frame form (kFrame*).
int pc_frame(const void* sp, int form, int n, const int* shape, const float* O, const float* D,
             const float* t, float* P, float* N, int* zero) {
  const PcScene* s = (const PcScene*)sp;
  if (!s || form < 0 || form >= kFrameCount || n < 0 || !indices_ok(s, n, shape)) return -2;
  if (n == 0) return 0;
  Bufs bf;
  void *dS, *dO, *dD, *dT, *dP, *dN, *dZ;
  PC_TRY(bf.get(&dS, shape, (size_t)n * 4));
  PC_TRY(bf.get(&dO, O, (size_t)n * 12));
  PC_TRY(bf.get(&dD, D, (size_t)n * 12));
  PC_TRY(bf.get(&dT, t, (size_t)n * 4));
  PC_TRY(bf.get(&dP, nullptr, (size_t)n * 12));
  PC_TRY(bf.get(&dN, nullptr, (size_t)n * 12));
  PC_TRY(bf.get(&dZ, nullptr, (size_t)n * 4));
  k_frame<<<grid_of(n), kBlock>>>(scene_of(s, -1, -1), form, n, (const int*)dS, (const float*)dO,
                                  (const float*)dD, (const float*)dT, (float*)dP, (float*)dN,
                                  (int*)dZ);
  if (int r = finish()) return r;
  PC_TRY(hipMemcpy(P, dP, (size_t)n * 12, hipMemcpyDeviceToHost));
  PC_TRY(hipMemcpy(N, dN, (size_t)n * 12, hipMemcpyDeviceToHost));
  PC_TRY(hipMemcpy(zero, dZ, (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
