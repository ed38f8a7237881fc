// prim_check.hip — TEST INFRASTRUCTURE ONLY (tests/test_gpu_prims.py, `make primcheck`).
//
// Runs the product's own device routines (rc_device.hpp, rc_cudasem.hpp: the very functions the
// kernels inline, compiled with the product's flags) one thread per case, so the tests can
// compare them ray by ray with the CPU oracle and with numpy.  The shape records come from
// rc_pack_scene (rc_scene.o), which computes o0, r2 and inv_r.  Every entry copies its host
// arrays to the device, makes ONE launch and copies the results back; it returns 0, a HIP
// error code, or -2 for an argument it refuses (a shape index outside the scene).
//
// The *_mut routines below are deliberately wrong copies of product routines:
// the tests require the case lists to tell each of them from the reference.
//
// The hit-level entries (pc_shade, pc_shoot; tests/test_gpu_shading.py) run shade, cu_shade, the
// bounce loops shoot<MODE> and shade_dep_cont the same way, with the scene's lights and colour
// pairs set up as the library's upload_scene sets them up.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "raycast_hip.h"
#include "rc_cudasem.hpp"
#include "rc_device.hpp"
#include "rc_pixel.hpp"
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
  kOpQuant,        // a = c (f32) -> o1 = quant(c) (i32)
  kOpPrimaryDir,   // a = hx, hy (2 f64), b = pw, ph (2 f32), x, y (2 i32) -> o0 = zero events (i32),
                   //   o1 = primary_dir (3 f32)
  kOpPowGeneral,   // a = alpha (f32), b = a0 (f32) -> o1 = (float)pow((double)alpha, (double)a0),
                   //   the expression shade evaluates for a spot exponent that is no small integer
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
    case kOpQuant: oi[i] = (int)quant(af[i]); break;
    case kOpPrimaryDir: {
      Cam cam;
      cam.hx = ad[2 * i];
      cam.hy = ad[2 * i + 1];
      cam.pw = bf[4 * i];
      cam.ph = bf[4 * i + 1];
      const int* bi = (const int*)b;
      int ze = 0;
      const V3 d = primary_dir(cam, bi[4 * i + 2], bi[4 * i + 3], ze);
      ((int*)o0)[i] = ze;
      of[3 * i] = d.x;
      of[3 * i + 1] = d.y;
      of[3 * i + 2] = d.z;
      break;
    }
    case kOpPowGeneral: of[i] = (float)pow((double)af[i], (double)bf[i]); break;
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

// --------------------------------------------------------------------- shading --
// shade with one of three deliberate mistakes (kMut: 1, 2, 3) — the arguments the product's
// comments make, undone one at a time:
//   1  `inert` without its two finiteness tests (an infinite or NaN attenuation times +-0 is NaN,
//      and only the shadow ray decides whether the reference adds it)
//   2  alpha = -dot(ld, dir): the dot product negated as a whole, zero components and all
//   3  no second zero-normalize event for an unshadowed spot light with P on it
template <int kMut>
__device__ __forceinline__ V3 shade_mut(const Scene& sc, int idx, V3 P, V3 N, V3 D, int& zero_events) {
  const rc_shape& o = sc.lshapes[idx];
  const float opacity = o.opacity;
  V3 out = v3(0.0f, 0.0f, 0.0f);
  if (!(opacity > 0.0f)) return out;
  const int skip = (idx == sc.n) ? -1 : idx;
  const rc_shade_pair* pr = sc.lpairs + (size_t)idx * sc.m;
  for (int l = 0; l < sc.m; ++l) {
    const rc_light& L = sc.lights[l];
    V3 ld = v3(L.pos[0] - P.x, L.pos[1] - P.y, L.pos[2] - P.z);
    const float dist = length(ld);
    if (dist == 0.0f) zero_events++;
    else ld = div3(ld, dist);
    const float lin = L.r0 + L.r1 * dist;
    const float rad =
        (float)(1.0 / ((double)lin + (double)L.r2 * ((double)dist * (double)dist)));
    float ang = 1.0f;
    const bool z = dist == 0.0f;
    if (L.type == RC_LIGHT_SPOT) {
      const V3 vr = v3(P.x - L.pos[0], P.y - L.pos[1], P.z - L.pos[2]);
      const V3 v = v3(vr.x == 0.0f ? vr.x : -ld.x, vr.y == 0.0f ? vr.y : -ld.y,
                      vr.z == 0.0f ? vr.z : -ld.z);
      const V3 dir = v3(L.dir[0], L.dir[1], L.dir[2]);
      const float alpha = kMut == 2 ? -dot(ld, dir) : dot(v, dir);
      if (alpha < L.cos_theta) ang = 0.0f;
      else if (L.a0_kind == RC_A0_INT) ang = (float)pown_dd((double)alpha, L.a0_int);
      else ang = (float)pow((double)alpha, (double)L.a0);
    }
    const float th = dot(N, ld);
    const bool fin = kMut == 1 || (__builtin_isfinite(rad) && __builtin_isfinite(ang));
    const bool inert = th <= 0.0f && fin && !(z && L.type == RC_LIGHT_SPOT);
    if (inert) continue;
    if (shadowed(sc, P, ld, skip)) continue;
    if (L.type == RC_LIGHT_SPOT && kMut != 3) zero_events += z ? 1 : 0;
    float dr = 0.0f, dg = 0.0f, db = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
    if (!(th <= 0.0f)) {
      const rc_shade_pair& p = pr[l];
      dr = p.dl[0] * th;
      dg = p.dl[1] * th;
      db = p.dl[2] * th;
      const V3 view = v3(D.x * -1.0f, D.y * -1.0f, D.z * -1.0f);
      const double angle = (double)dot(view, reflect(ld, N));
      if (!(angle > 0.0)) {
        const double p20 = pow20(angle);
        sr = (float)((double)p.sl[0] * p20);
        sg = (float)((double)p.sl[1] * p20);
        sb = (float)((double)p.sl[2] * p20);
      }
    }
    out.x = out.x + ((dr + sr) * rad) * ang;
    out.y = out.y + ((dg + sg) * rad) * ang;
    out.z = out.z + ((db + sb) * rad) * ang;
  }
  return v3(out.x * opacity, out.y * opacity, out.z * opacity);
}

enum {
  kShade = 0,        // shade, records read from global memory
  kShadeStaged,      // shade after stage_scene<true>: lshapes / lpairs in LDS, as the pixel kernels
  kShadeCuda,        // cusem::cu_shade (no phantom, no events)
  kShadeMutInert,    // shade_mut<1>
  kShadeMutAlpha,    // shade_mut<2>
  kShadeMutZero,     // shade_mut<3>
  kShadeCount
};

// idx[i] == -1 is the phantom (record sc.n)
template <bool kStage>
__global__ void k_shade(Scene sc, int form, int n, const int* idx, const float* Pa, const float* Na,
                        const float* Da, float* rgb, int* zero) {
  __shared__ StageBuf<kStage> buf;
  stage_scene<kStage>(sc, buf);   // every thread: it has a barrier
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int k = idx[i] < 0 ? sc.n : idx[i];
  const V3 P = ld3(Pa, i), N = ld3(Na, i), D = ld3(Da, i);
  int ze = 0;
  V3 c = v3(0.0f, 0.0f, 0.0f);
  switch (form) {
    case kShade:
    case kShadeStaged: c = shade(sc, k, P, N, D, ze); break;
    case kShadeCuda: c = cusem::cu_shade(sc, k, P, N, D); break;
    case kShadeMutInert: c = shade_mut<1>(sc, k, P, N, D, ze); break;
    case kShadeMutAlpha: c = shade_mut<2>(sc, k, P, N, D, ze); break;
    case kShadeMutZero: c = shade_mut<3>(sc, k, P, N, D, ze); break;
    default: break;
  }
  rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
  zero[i] = ze;
}

enum {
  kShootFast = 0,    // shoot<kModeFast>
  kShootParityA,     // shoot<kModeParityA>: class; rgb and carry where the class is not DEP
  kShootParityC,     // shoot<kModeParityC> from the case's carry-in
  kShootClassify,    // shoot<kModeClassify>: class and carry only
  kShootDepCont,     // shoot<kModeParityA>, then for a DEP pixel under dep_fast shade_dep_cont on
                     //   the line phase A would have written, from the case's carry-in
  kShootCount
};

// cls: the device's class (kClsIdent / kClsWriter / kClsDep); flag: 1 where kShootDepCont ran
// shade_dep_cont.  carry_out: po.carry where the pixel wrote it, else the carry-in.
__global__ void k_shoot(Scene sc, int form, int n, int maxrec, const float* da, const float* cin,
                        float* rgb, int* cls, float* cout, int* zero, int* flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 d = ld3(da, i), c = ld3(cin, i);
  PixelOut po;
  po.carry = c;
  int ze = 0, fl = 0;
  switch (form) {
    case kShootFast: shoot<kModeFast>(sc, d, maxrec, v3(0.0f, 0.0f, 0.0f), po, ze); break;
    case kShootParityA: shoot<kModeParityA>(sc, d, maxrec, v3(0.0f, 0.0f, 0.0f), po, ze); break;
    case kShootParityC: shoot<kModeParityC>(sc, d, maxrec, c, po, ze); break;
    case kShootClassify: shoot<kModeClassify>(sc, d, maxrec, v3(0.0f, 0.0f, 0.0f), po, ze); break;
    case kShootDepCont: {
      shoot<kModeParityA>(sc, d, maxrec, v3(0.0f, 0.0f, 0.0f), po, ze);
      if (po.cls == kClsDep && sc.dep_fast) {
        DepLine line;
        line.r = po.dep;
        line.px = po.pcol.x; line.py = po.pcol.y; line.pz = po.pcol.z;
        line.pad3 = 0;
        po.rgb = shade_dep_cont(sc, &line, maxrec, c, ze);
        fl = 1;
      }
      break;
    }
    default: break;
  }
  const V3 co = po.cls == kClsWriter ? po.carry : c;
  rgb[3 * i] = po.rgb.x; rgb[3 * i + 1] = po.rgb.y; rgb[3 * i + 2] = po.rgb.z;
  cout[3 * i] = co.x; cout[3 * i + 1] = co.y; cout[3 * i + 2] = co.z;
  cls[i] = po.cls;
  zero[i] = ze;
  flag[i] = fl;
}

// cusem::render_pixel takes a camera and a pixel, not a direction: pixel i = (xy[2i], xy[2i+1])
__global__ void k_render_pixel(Scene sc, Cam cam, int n, int max_iter, const int* xy, float* rgb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 c = cusem::render_pixel(sc, cam, xy[2 * i], xy[2 * i + 1], max_iter);
  rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
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

constexpr int kPcBlock = 256;
inline int grid_of(int n) { return (n + kPcBlock - 1) / kPcBlock; }

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
  sc.m = 0;   // the intersection entries shade nothing: lights and pairs stay null
  sc.has_quadric = hq < 0 ? s->natural_hq : hq;
  sc.o0_ok = o0 < 0 ? s->host->o0_ok : o0;
  return sc;
}

// The scene of the shading entries: lights, colour pairs, the reflectivity mask and dep_fast from
// the packed image, restated here as upload_scene (rc_api.hip) states them.
Scene lit_scene_of(const PcScene* s) {
  Scene sc = scene_of(s, -1, -1);
  const rc_packed_header* h = s->host;
  sc.lights = (const rc_light*)(s->dev + h->off_lights);
  sc.pairs = (const rc_shade_pair*)(s->dev + h->off_pairs);
  sc.lpairs = sc.pairs;
  sc.m = h->m;
  const rc_shape* hs = (const rc_shape*)((const char*)h + h->off_shapes);
  for (int k = 0; k < h->n && k < 64; ++k)
    if (hs[k].refl > 0.0f) sc.refl_mask |= 1ull << k;
  sc.dep_fast = !(hs[h->n].opacity > 0.0f);
  for (int k = 0; k < h->n; ++k)
    if (!(fabsf(hs[k].refl) < 1.0e5f)) sc.dep_fast = 0;
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
      {8, 0, 8, 0}, {8, 4, 8, 0}, {8, 8, 0, 4}, {8, 8, 0, 4}, {12, 12, 0, 4},
      {4, 0, 0, 4}, {16, 16, 4, 12}, {4, 4, 0, 4}};
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
  k_scalar<<<grid_of(n), kPcBlock>>>(op, n, da, db, d0, d1);
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
  k_shape<<<grid_of(n), kPcBlock>>>((const rc_shape*)(s->dev + s->host->off_shapes), form, n,
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
  k_list<<<grid_of(n), kPcBlock>>>(scene_of(s, has_quadric, o0_ok), form, n, (const float*)dO,
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
  k_frame<<<grid_of(n), kPcBlock>>>(scene_of(s, -1, -1), form, n, (const int*)dS, (const float*)dO,
                                  (const float*)dD, (const float*)dT, (float*)dP, (float*)dN,
                                  (int*)dZ);
  if (int r = finish()) return r;
  PC_TRY(hipMemcpy(P, dP, (size_t)n * 12, hipMemcpyDeviceToHost));
  PC_TRY(hipMemcpy(N, dN, (size_t)n * 12, hipMemcpyDeviceToHost));
  PC_TRY(hipMemcpy(zero, dZ, (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
}

// One shading form (kShade*) for n hits: shape index (-1: the phantom), hit point, normal and ray
// direction (3 floats each) -> the colour (3 floats) and the zero-normalize events.  -2: an index
// outside the scene, the phantom under kShadeCuda, or kShadeStaged for a scene the pixel kernels
// would not stage (stage_fits).
int pc_shade(const void* sp, int form, int n, const int* idx, const float* P, const float* N,
             const float* D, float* rgb, int* zero) {
  const PcScene* s = (const PcScene*)sp;
  if (!s || form < 0 || form >= kShadeCount || n < 0) return -2;
  for (int i = 0; i < n; ++i)
    if (idx[i] < (form == kShadeCuda ? 0 : -1) || idx[i] >= s->host->n) return -2;
  const rc_packed_header* h = s->host;
  if (form == kShadeStaged && !(h->n + 1 <= kStageShapes && (h->n + 1) * h->m <= kStagePairs))
    return -2;
  if (n == 0) return 0;
  Bufs bf;
  void *dI, *dP, *dN, *dD, *dC, *dZ;
  PC_TRY(bf.get(&dI, idx, (size_t)n * 4));
  PC_TRY(bf.get(&dP, P, (size_t)n * 12));
  PC_TRY(bf.get(&dN, N, (size_t)n * 12));
  PC_TRY(bf.get(&dD, D, (size_t)n * 12));
  PC_TRY(bf.get(&dC, nullptr, (size_t)n * 12));
  PC_TRY(bf.get(&dZ, nullptr, (size_t)n * 4));
  if (form == kShadeStaged)
    k_shade<true><<<grid_of(n), kPcBlock>>>(lit_scene_of(s), form, n, (const int*)dI, (const float*)dP,
                                          (const float*)dN, (const float*)dD, (float*)dC, (int*)dZ);
  else
    k_shade<false><<<grid_of(n), kPcBlock>>>(lit_scene_of(s), form, n, (const int*)dI,
                                           (const float*)dP, (const float*)dN, (const float*)dD,
                                           (float*)dC, (int*)dZ);
  if (int r = finish()) return r;
  PC_TRY(hipMemcpy(rgb, dC, (size_t)n * 12, hipMemcpyDeviceToHost));
  PC_TRY(hipMemcpy(zero, dZ, (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
}

// One bounce-loop form (kShoot*) for n primary directions d (3 floats) with carry-ins (3 floats):
// the colour before quantisation, the device's class, the carry after the pixel, the
// zero-normalize events and kShootDepCont's flag.  dep_fast: -1 = as the library derives it from
// the scene, 0 = off.  maxrec: 1 .. 64.
int pc_shoot(const void* sp, int form, int dep_fast, int n, int maxrec, const float* d,
             const float* carry_in, float* rgb, int* cls, float* carry_out, int* zero, int* flag) {
  const PcScene* s = (const PcScene*)sp;
  if (!s || form < 0 || form >= kShootCount || n < 0 || maxrec < 1 || maxrec > 64 ||
      dep_fast < -1 || dep_fast > 0)
    return -2;
  if (n == 0) return 0;
  Scene sc = lit_scene_of(s);
  if (dep_fast == 0) sc.dep_fast = 0;
  Bufs bf;
  void *dD, *dI, *dC, *dK, *dO, *dZ, *dF;
  PC_TRY(bf.get(&dD, d, (size_t)n * 12));
  PC_TRY(bf.get(&dI, carry_in, (size_t)n * 12));
  PC_TRY(bf.get(&dC, nullptr, (size_t)n * 12));
  PC_TRY(bf.get(&dK, nullptr, (size_t)n * 4));
  PC_TRY(bf.get(&dO, nullptr, (size_t)n * 12));
  PC_TRY(bf.get(&dZ, nullptr, (size_t)n * 4));
  PC_TRY(bf.get(&dF, nullptr, (size_t)n * 4));
  k_shoot<<<grid_of(n), kPcBlock>>>(sc, form, n, maxrec, (const float*)dD, (const float*)dI,
                                  (float*)dC, (int*)dK, (float*)dO, (int*)dZ, (int*)dF);
  if (int r = finish()) return r;
  PC_TRY(hipMemcpy(rgb, dC, (size_t)n * 12, hipMemcpyDeviceToHost));
  PC_TRY(hipMemcpy(cls, dK, (size_t)n * 4, hipMemcpyDeviceToHost));
  PC_TRY(hipMemcpy(carry_out, dO, (size_t)n * 12, hipMemcpyDeviceToHost));
  PC_TRY(hipMemcpy(zero, dZ, (size_t)n * 4, hipMemcpyDeviceToHost));
  PC_TRY(hipMemcpy(flag, dF, (size_t)n * 4, hipMemcpyDeviceToHost));
  return 0;
}

// cusem::render_pixel for n pixels (x, y) of the scene's W x H camera (the launchers' make_cam):
// the colour before quantisation.  max_iter: 0 .. 64.
int pc_render_pixel(const void* sp, int W, int H, int max_iter, int n, const int* xy, float* rgb) {
  const PcScene* s = (const PcScene*)sp;
  if (!s || W < 1 || H < 1 || max_iter < 0 || max_iter > 64 || n < 0) return -2;
  if (n == 0) return 0;
  Cam cam;
  cam.hx = 0.0 - (double)s->host->cam_w / 2.0;
  cam.hy = 0.0 + (double)s->host->cam_h / 2.0;
  cam.pw = s->host->cam_w / (float)W;
  cam.ph = s->host->cam_h / (float)H;
  Bufs bf;
  void *dX, *dC;
  PC_TRY(bf.get(&dX, xy, (size_t)n * 8));
  PC_TRY(bf.get(&dC, nullptr, (size_t)n * 12));
  k_render_pixel<<<grid_of(n), kPcBlock>>>(lit_scene_of(s), cam, n, max_iter, (const int*)dX,
                                           (float*)dC);
  if (int r = finish()) return r;
  PC_TRY(hipMemcpy(rgb, dC, (size_t)n * 12, hipMemcpyDeviceToHost));
  return 0;
}

// m lights, dep_fast as lit_scene_of derives it, and whether the pixel kernels would stage the scene
void pc_scene_lit_info(const void* sp, int* m, int* dep_fast, int* staged) {
  const PcScene* s = (const PcScene*)sp;
  const rc_packed_header* h = s->host;
  *m = h->m;
  *dep_fast = lit_scene_of(s).dep_fast;
  *staged = h->n + 1 <= kStageShapes && (h->n + 1) * h->m <= kStagePairs;
}

}  // extern "C"
