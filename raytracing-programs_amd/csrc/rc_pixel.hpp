// rc_pixel.hpp — what the two kernel files share (rc_kernels.hip: the renderer and the parity
// pipeline; rc_sample_kernels.hip: the sampling family): the build-time switches both read, the
// pixel kernels' tiles and framebuffer stores, the LDS copy of the scene, and the launchers' host
// helpers (make_scene, stage_fits, make_cam, dispatch).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "rc_device.hpp"
#include "rc_kernels.h"

// Which kernels use the cross-term-free quadric form (quad_x0: Scene::has_quadric == 2,
// rc_device.hpp quad_abc) when the scene allows it.  A kernel with 0 folds has_quadric to 0/1,
// so quad_x0 is a constant false there and the form and its branches are compiled out.
// (RC_X0_PHASE_C and RC_X0_RESOLVE, the parity side's, are in rc_kernels.hip.)
#ifndef RC_X0_PIXEL
#define RC_X0_PIXEL 1     // k_render, k_phase_a, k_classify
#endif
#ifndef RC_PHASE_A_WAVES
#define RC_PHASE_A_WAVES 4   // waves per SIMD the render kernels are compiled for
#endif

namespace rc {

// Pixel kernels: a workgroup renders a 16x16-pixel tile of four 8x8 wave tiles (ray coherence
// inside a wave); each lane stores its own three framebuffer bytes.  The LDS-staged form
// (RC_TILE_STAGE=1, built as libraycast_hip_coalesced.so with 32x8 tiles) writes every tile row
// as one 96-byte run instead: rocprofv3 WRITE_SIZE of k_render at quadric 4096^2 50.6 MB (=
// the 50.3 MB framebuffer) against 64.0 MB for the lane stores, but k_render 0.74-0.76 ms
// against 0.69 ms and phase A 0.93-0.96 against 0.86 ms: these kernels are VALU-
// bound and their stores use < 1 % of HBM bandwidth, so the lane stores are the default.
#ifndef RC_TILE_W
#define RC_TILE_W 16
#endif
#ifndef RC_TILE_STAGE
#define RC_TILE_STAGE 0   // 1: tiles staged in LDS, written as whole rows (variant)
#endif
constexpr int kTileW = RC_TILE_W, kTileH = 256 / RC_TILE_W;
constexpr int kBlock = kTileW * kTileH;
static_assert(kTileW % 8 == 0 && kTileH % 8 == 0, "8x8 wave tiles");

// XCD-aware tile order (MI355X_MICROARCH.md: workgroups are dealt round-robin to the 8 XCDs,
// each with its own L2).  With the grid's own order, horizontally adjacent tiles run on
// different XCDs, so a 128-byte line of class bytes (8 tiles wide) or of framebuffer bytes
// (~3 tiles) is written piecewise from several L2s and reaches HBM as partial-line writes
// (rocprofv3 WRITE_SIZE of k_phase_a 1.26x its bytes).
//   RC_XCD_TILES 1: XCD k takes the k-th contiguous eighth of the tiles — measured: phase A
//                   0.745 -> 0.878 ms (the image's heavy bands land on a few XCDs);
//   RC_XCD_TILES 2: chunks of 8 horizontally adjacent tiles per XCD, chunks dealt round-robin
//                   (a line's tiles share one L2; the load stays interleaved).
#ifndef RC_XCD_TILES
#define RC_XCD_TILES 2   // measured: k_phase_a WRITE_SIZE 312 -> 269 MB in flight, time within noise
#endif
// order: RC_XCD_TILES for k_phase_a; k_render keeps the grid order (its only stores are the
// framebuffer's; fast mode 0.64 ms in round 3 against 0.65-0.66 ms with chunks, r04l)
template <int kOrder = RC_XCD_TILES>
__device__ __forceinline__ void xcd_tile(int& bx, int& by) {
  const int nx = gridDim.x, n = nx * (int)gridDim.y;
  const int lin = (int)blockIdx.y * nx + (int)blockIdx.x;
  int t = lin;
  if (kOrder == 1) {
    const int xcd = lin & 7, k = lin >> 3, q = n >> 3, r = n & 7;
    // XCDs below r take q + 1 tiles, the others q: a bijection of [0, n)
    t = xcd < r ? xcd * (q + 1) + k : r * (q + 1) + (xcd - r) * q + k;
  } else if (kOrder == 2 && lin < (n & ~63)) {
    // the XCD's k-th workgroup -> chunk (k / 8) * 8 + xcd, tile k % 8 of it (a bijection of
    // the first n & ~63 tiles; the rest keep the grid order)
    const int xcd = lin & 7, k = lin >> 3;
    t = ((k >> 3) * 8 + xcd) * 8 + (k & 7);
  }
  bx = t % nx;
  by = t / nx;
}

__device__ __forceinline__ void tile_pixel(int& lx, int& ly) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  lx = (wave % (kTileW / 8)) * 8 + (lane & 7);
  ly = (wave / (kTileW / 8)) * 8 + (lane >> 3);
}

// A tile's framebuffer bytes (and, for phase A, its class bytes) staged in LDS: every lane
// drops its 3 (1) bytes in, then the workgroup writes each row of the tile as one contiguous
// run — dword stores when the run is whole and 4-byte aligned (W % 4 == 0), bytes otherwise —
// instead of three byte stores per lane into 8-pixel row fragments (the store
// north_star names is the coalesced one; C/raycast.c:122-127 is the store replaced).
struct TileBytes {
  uint32_t rgb[kTileH][kTileW * 3 / 4];
  uint32_t cls[kTileH][kTileW / 4];
  int done;   // waves that have staged their pixels
};

// Zeroes the wave counter; the caller's next barrier publishes it.
__device__ __forceinline__ void tile_init(TileBytes& t) {
  if (threadIdx.x == 0) t.done = 0;
}

// No workgroup barrier before the row writes (waiting for the slowest wave of a tile held the
// others' slots: measured +7 % on k_render): each wave releases its staged bytes and counts
// itself in; the LAST wave of the tile writes every row and the others simply end.
__device__ __forceinline__ bool tile_last_wave(TileBytes& t) {
  if (!RC_TILE_STAGE) return false;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  int old = 0;
  if ((threadIdx.x & 63) == 0)
    old = __hip_atomic_fetch_add(&t.done, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
  old = __shfl(old, 0, 64);
  if (old != kBlock / 64 - 1) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  return true;
}

__device__ __forceinline__ void tile_put_rgb(TileBytes& t, int lx, int ly, uint8_t r, uint8_t g,
                                             uint8_t b, uint8_t* direct) {
  if (!RC_TILE_STAGE) {   // the default: the lane's own three byte stores
    direct[0] = r;
    direct[1] = g;
    direct[2] = b;
    return;
  }
  uint8_t* q = (uint8_t*)t.rgb[ly] + lx * 3;
  q[0] = r;
  q[1] = g;
  q[2] = b;
}

// Row ly of the tile goes to dst_row(ly) (nullptr: the row is outside the image), nbytes
// valid bytes per row.  The tile's last wave calls this (tile_last_wave).
template <int kWords, typename RowPtr>
__device__ __forceinline__ void tile_write_rows(const uint32_t (*src)[kWords], RowPtr dst_row,
                                                int nbytes) {
  const int t = threadIdx.x & 63;   // one wave writes the tile (tile_last_wave)
  for (int i = t; i < kTileH * kWords; i += 64) {
    const int ly = i / kWords, k = i % kWords;
    uint8_t* d = dst_row(ly);
    if (!d) continue;
    if (nbytes == kWords * 4 && ((uintptr_t)d & 3u) == 0u) {
      ((uint32_t*)d)[k] = src[ly][k];
    } else {
      const uint8_t* sb = (const uint8_t*)src[ly];
      for (int b = k * 4; b < k * 4 + 4 && b < nbytes; ++b) d[b] = sb[b];
    }
  }
}

__device__ __forceinline__ void store_rgb(uint8_t* __restrict__ p, V3 c) {
  p[0] = quant(c.x);
  p[1] = quant(c.y);
  p[2] = quant(c.z);
}

__device__ __forceinline__ void flush_events(int zero_events, unsigned long long* counter) {
  if (zero_events) atomicAdd(counter, (unsigned long long)zero_events);
}

// The pixel kernels' divergent record reads (the winner's frame, shading record and colour
// pairs: Scene::lshapes / lpairs) come from an LDS copy of the scene when it is small
// enough: an LDS read instead of a vector-memory round trip per lane.  The
// uniform loops over shapes and lights keep their scalar loads.
constexpr int kStageShapes = 32;   // shape records, phantom included
constexpr int kStagePairs = 128;   // (shape, light) colour pairs
struct SceneStage {
  rc_shape shapes[kStageShapes];
  rc_shade_pair pairs[kStagePairs];
};
template <bool kStage>
struct StageBuf {
  SceneStage s;
};
template <>
struct StageBuf<false> {
  int unused;
};

// Every thread of the workgroup must call this (it has a barrier).
template <bool kStage>
__device__ __forceinline__ void stage_scene(Scene& sc, StageBuf<kStage>& buf) {
  if constexpr (kStage) {
    const int ws = (int)(sizeof(rc_shape) / 4) * (sc.n + 1);
    for (int i = threadIdx.x; i < ws; i += blockDim.x)
      ((unsigned*)buf.s.shapes)[i] = ((const unsigned*)sc.shapes)[i];
    const int wp = (int)(sizeof(rc_shade_pair) / 4) * (sc.n + 1) * sc.m;
    for (int i = threadIdx.x; i < wp; i += blockDim.x)
      ((unsigned*)buf.s.pairs)[i] = ((const unsigned*)sc.pairs)[i];
    __syncthreads();
    sc.lshapes = buf.s.shapes;
    sc.lpairs = buf.s.pairs;
  }
}

static Scene make_scene(const LaunchScene& s) {
  Scene sc;
  sc.shapes = s.shapes;
  sc.lights = s.lights;
  sc.pairs = s.pairs;
  sc.lshapes = s.shapes;
  sc.lpairs = s.pairs;
  sc.n = s.n;
  sc.m = s.m;
  sc.refl_mask = s.refl_mask;
  sc.has_quadric = s.has_quadric;
  sc.o0_ok = s.o0_ok;
  sc.dep_fast = s.dep_fast;
  sc.pin = s.pin;
  return sc;
}
static bool stage_fits(const LaunchScene& s) {
  return s.n + 1 <= kStageShapes && (s.n + 1) * s.m <= kStagePairs;
}
static Cam make_cam(const LaunchScene& s, int W, int H) {
  Cam c;
  c.hx = 0.0 - (double)s.cam_w / 2.0;
  c.hy = 0.0 + (double)s.cam_h / 2.0;
  c.pw = s.cam_w / (float)W;
  c.ph = s.cam_h / (float)H;
  return c;
}

// The launchers' runtime flags as the kernels' template flags: fn(st) or fn(cuda, st) with
// std::bool_constant arguments, so a launcher names its kernel once as k<cuda.value, st.value>.
// cuda_sem is the outer branch: kernels are emitted in the order they are instantiated, and
// <true, true>, <true, false>, <false, true>, <false, false> keeps the code object's layout as
// it has been measured.
template <class Fn>
static void dispatch(bool st, Fn fn) {
  st ? fn(std::true_type{}) : fn(std::false_type{});
}
template <class Fn>
static void dispatch(bool cuda_sem, bool st, Fn fn) {
  if (cuda_sem)
    dispatch(st, [&](auto s) { fn(std::true_type{}, s); });
  else
    dispatch(st, [&](auto s) { fn(std::false_type{}, s); });
}

}  // namespace rc
