// pin_check.hip — test-only device harness of phase C's carry-point table (rc_device.hpp:
// pin_build, shade_dep_cont_pin, shade_dep_wave), for tests/test_gpu_pinned.py.  One wave per
// group of 64 entries, as k_dep_chunks' second pass runs them: every lane first runs phase A's
// shoot<kModeParityA> on its primary direction (which leaves the DEP line and counts the primary
// part's events, as k_phase_a does), then the wave shades its DEP entries from the given
// carry-ins with the product's own shade_dep_wave (Scene::pin set) or shade_dep_cont (pin 0).
// Compiled with the product's HIPFLAGS; the product library never links it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "raycast_hip.h"
#include "rc_device.hpp"
#include "rc_scene.h"

using namespace rc;

namespace {

// cnt[0]: waves that took the table, cnt[1]: waves that had DEP entries and did not
__global__ void __launch_bounds__(64) k_pin_wave(Scene sc, int n, int maxrec, const float* da,
                                                 const float* cin, float* rgb, int* zero,
                                                 int* flag, int* cnt) {
  __shared__ PinTable tb;
  const int lane = (int)threadIdx.x, i = (int)blockIdx.x * 64 + lane;
  const bool in = i < n;
  PixelOut po;
  po.cls = kClsIdent;
  po.rgb = v3(0.0f, 0.0f, 0.0f);
  int ze = 0;
  V3 c = v3(0.0f, 0.0f, 0.0f);
  if (in) {
    c = v3(cin[3 * i], cin[3 * i + 1], cin[3 * i + 2]);
    shoot<kModeParityA>(sc, v3(da[3 * i], da[3 * i + 1], da[3 * i + 2]), maxrec,
                        v3(0.0f, 0.0f, 0.0f), po, ze);
  }
  const bool dep = in && po.cls == kClsDep && sc.dep_fast;
  DepLine line;
  line.r = po.dep;
  line.px = po.pcol.x; line.py = po.pcol.y; line.pz = po.pcol.z;
  line.pad3 = 0;
  // pass 1 of k_dep_chunks compacts the entries: the DEP lanes move to the front of the wave
  const unsigned long long m = __ballot(dep);
  const int slot = __popcll(m & ((1ull << lane) - 1ull)), ndep = __popcll(m);
  __shared__ DepLine s_line[64];
  __shared__ float s_c[64][3];
  __shared__ int s_src[64];
  if (dep) {
    s_line[slot] = line;
    s_c[slot][0] = c.x; s_c[slot][1] = c.y; s_c[slot][2] = c.z;
    s_src[slot] = lane;
  }
  __syncthreads();
  const bool act = lane < ndep;
  V3 out = v3(0.0f, 0.0f, 0.0f);
  int zc = 0;
  bool took = false;
  if (ndep > 0) {   // wave-uniform
    const V3 cc = act ? v3(s_c[lane][0], s_c[lane][1], s_c[lane][2]) : v3(0.0f, 0.0f, 0.0f);
    if (sc.pin) {
      out = shade_dep_wave(sc, &s_line[lane & 63], maxrec, cc, act, tb, zc, took);
    } else if (act) {
      out = shade_dep_cont(sc, &s_line[lane], maxrec, cc, zc);
    }
    if (lane == 0) atomicAdd(&cnt[took ? 0 : 1], 1);
  }
  // back to the entries' own places
  __shared__ float s_o[64][3];
  __shared__ int s_z[64];
  if (act) {
    const int src = s_src[lane];
    s_o[src][0] = out.x; s_o[src][1] = out.y; s_o[src][2] = out.z;
    s_z[src] = zc;
  }
  __syncthreads();
  if (!in) return;
  V3 o = po.rgb;
  if (dep) {
    o = v3(s_o[lane][0], s_o[lane][1], s_o[lane][2]);
    ze += s_z[lane];
  }
  rgb[3 * i] = o.x; rgb[3 * i + 1] = o.y; rgb[3 * i + 2] = o.z;
  zero[i] = ze;
  flag[i] = dep ? 1 : 0;
}

struct PnScene {
  rc_packed_header* host;
  char* dev;
};

#define PN_TRY(x)                         \
  do {                                    \
    const hipError_t e_ = (x);            \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

struct Bufs {
  void* p[8];
  int n = 0;
  ~Bufs() {
    for (int k = 0; k < n; ++k) (void)hipFree(p[k]);
  }
  hipError_t get(void** out, const void* src, size_t bytes) {
    *out = nullptr;
    if (n >= 8) return hipErrorOutOfMemory;
    void* d = nullptr;
    hipError_t e = hipMalloc(&d, bytes ? bytes : 4);
    if (e != hipSuccess) return e;
    p[n++] = d;
    *out = d;
    if (src) return hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
    return hipMemset(d, 0, bytes ? bytes : 4);
  }
};

}  // namespace

extern "C" {

void* pn_scene_create(const json_data_t* js) {
  rc_packed_header* h = rc_pack_scene(js);
  if (!h) return nullptr;
  PnScene* s = (PnScene*)calloc(1, sizeof *s);
  if (!s) { free(h); return nullptr; }
  s->host = h;
  if (hipMalloc((void**)&s->dev, (size_t)h->bytes) != hipSuccess ||
      hipMemcpy(s->dev, h, (size_t)h->bytes, hipMemcpyHostToDevice) != hipSuccess) {
    if (s->dev) (void)hipFree(s->dev);
    free(h);
    free(s);
    return nullptr;
  }
  return s;
}

void pn_scene_destroy(void* sp) {
  PnScene* s = (PnScene*)sp;
  if (!s) return;
  (void)hipFree(s->dev);
  free(s->host);
  free(s);
}

// n, m, dep_fast, and whether the library would give the scene a table (RC_PIN_FITS)
void pn_scene_info(const void* sp, int* n, int* m, int* dep_fast, int* fits) {
  const rc_packed_header* h = ((const PnScene*)sp)->host;
  const rc_shape* hs = (const rc_shape*)((const char*)h + h->off_shapes);
  int df = !(hs[h->n].opacity > 0.0f);
  for (int k = 0; k < h->n; ++k)
    if (!(fabsf(hs[k].refl) < 1.0e5f)) df = 0;
  *n = h->n;
  *m = h->m;
  *dep_fast = df;
  *fits = RC_PIN_FITS(h->n, h->m) ? 1 : 0;
}

// n entries (primary direction d, carry-in c: 3 floats each), wave w takes entries 64 w .. 64 w +
// 63.  pin: rc_tuning.pin's bit 0 as upload_scene (rc_api.hip) turns it into Scene::pin — it is
// dropped where the scene is not dep_fast or does not fit the table.  Out: the pixel's colour
// before quantisation and its zero-normalize events where flag = 1 (a DEP pixel under dep_fast;
// elsewhere phase A's own), and waves[2] = waves that took the table / that did not.
int pn_dep_wave(const void* sp, int pin, int n, int maxrec, const float* d, const float* carry_in,
                float* rgb, int* zero, int* flag, int* waves) {
  const PnScene* s = (const PnScene*)sp;
  if (!s || n < 0 || maxrec < 1 || maxrec > 64 || pin < 0 || pin > 1) return -2;
  waves[0] = waves[1] = 0;
  if (n == 0) return 0;
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
  for (int k = 0; k < h->n; ++k)
    if (hs[k].type == RC_SHAPE_QUADRIC) sc.has_quadric = 1;   // phase C keeps the cross terms (RC_X0_PHASE_C)
  sc.o0_ok = h->o0_ok;
  sc.dep_fast = !(hs[h->n].opacity > 0.0f);
  for (int k = 0; k < h->n; ++k)
    if (!(fabsf(hs[k].refl) < 1.0e5f)) sc.dep_fast = 0;
  sc.pin = sc.dep_fast && RC_PIN_FITS(h->n, h->m) ? pin : 0;
  Bufs bf;
  void *dD, *dI, *dC, *dZ, *dF, *dW;
  PN_TRY(bf.get(&dD, d, (size_t)n * 12));
  PN_TRY(bf.get(&dI, carry_in, (size_t)n * 12));
  PN_TRY(bf.get(&dC, nullptr, (size_t)n * 12));
  PN_TRY(bf.get(&dZ, nullptr, (size_t)n * 4));
  PN_TRY(bf.get(&dF, nullptr, (size_t)n * 4));
  PN_TRY(bf.get(&dW, nullptr, 8));
  k_pin_wave<<<(n + 63) / 64, 64>>>(sc, n, maxrec, (const float*)dD, (const float*)dI, (float*)dC,
                                    (int*)dZ, (int*)dF, (int*)dW);
  PN_TRY(hipGetLastError());
  PN_TRY(hipDeviceSynchronize());
  PN_TRY(hipMemcpy(rgb, dC, (size_t)n * 12, hipMemcpyDeviceToHost));
  PN_TRY(hipMemcpy(zero, dZ, (size_t)n * 4, hipMemcpyDeviceToHost));
  PN_TRY(hipMemcpy(flag, dF, (size_t)n * 4, hipMemcpyDeviceToHost));
  PN_TRY(hipMemcpy(waves, dW, 8, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
