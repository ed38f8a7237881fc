// rc_guided.hip — the two scene-free kernels behind the ambient-occlusion plane:
// k_ao_filter, the cross-bilateral pooling of the occlusion records guided by the G-buffer
// (rc_ao_filter_device), and k_ao_compose, the ambient term added to a colour image
// (rc_ao_compose_device).  Integer sums and the project's float dot: no new arithmetic.
//
// k_ao_filter.  One workgroup (256 threads, rc_pixel.hpp's lane layout: a wave owns an 8 x 8
// block) per 16 x 16 tile, one lane a pixel.
//   stage   the tile and a halo of `radius` pixels on every side into LDS once, as eight planes
//           of dwords (record, id, P.xyz, N.xyz).  An entry outside the image gets the id
//           INT_MIN, which matches no pixel that enters the loop (id_p >= 0), so the loop has no
//           bounds test.
//   pool    the (2r + 1)^2 taps in a uniform double loop: trip counts and taps are kernel
//           arguments (scalar loads; the taps widened to dwords, AoTaps).  A tap tests the id,
//           then the normal, then the plane distance, each read only when the test before it
//           passed: an interior pixel's lanes do not diverge and an edge pixel reads as little
//           as possible.  The centre's P and N stay in registers.  The sums are 32-bit (rc_ao_filter_check caps the weights at
//           32768 and a record's half at 65535); the one division a pixel is 64-bit.
// The LDS row pitch.  ds_read_b32 conflicts within a 32-lane half on (address / 4) % 32, and a
// half is four rows of eight pixels.  With a pitch of 32 dwords the four rows fall on the same
// eight banks (4-way); with a pitch = 8 or 24 (mod 32) they fall on four disjoint groups of
// eight.  The pitch is 24 dwords up to radius 4 (a region of at most 24 columns) and 40 above
// (at most 32): 13.5 KiB at radius 1, 40 KiB at radius 8.
// RC_AO_FILTER_DIRECT=1 (the Makefile's filter-variants) compiles the measurement variant that
// reads the neighbours from global memory through the caches instead, with a bounds test a tap.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "rc_device.hpp"
#include "rc_kernels.h"

#ifndef RC_AO_FILTER_DIRECT
#define RC_AO_FILTER_DIRECT 0
#endif

namespace rc {
namespace {

constexpr int kGuidedTile = 16;
constexpr int kGuidedThreads = 256;

__device__ __forceinline__ unsigned guided_byte(unsigned open, unsigned rays) {
  return rays ? (510u * open + rays) / (2u * rays) : 255u;   // rc_ao_byte: 510 * 65535 < 2^25
}

// the pooled byte: R ? (510 O + R) / (2 R) : 255 with O, R < 2^31
__device__ __forceinline__ unsigned pooled_byte(unsigned O, unsigned R) {
  if (!R) return 255u;
  return (unsigned)((510ull * O + R) / (2ull * R));
}

__device__ __forceinline__ void guided_pixel(int& lx, int& ly) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  lx = (wave & 1) * 8 + (lane & 7);
  ly = (wave >> 1) * 8 + (lane >> 3);
}

constexpr int ao_filter_pitch(int radius) { return radius <= 4 ? 24 : 40; }

// The filter's taps widened to dwords by the launcher: gfx950 has no 16-bit scalar load, and
// taps[|d|] with a uniform d is then one s_load_dword from the kernel-argument segment.
struct AoTaps {
  uint32_t t[kAoFilterMaxRadius + 1];
};

#if !RC_AO_FILTER_DIRECT
__global__ void __launch_bounds__(kGuidedThreads) k_ao_filter(
    const uint32_t* __restrict__ ao, const int32_t* __restrict__ id, const float* __restrict__ P,
    const float* __restrict__ N, int W, int H, AoFilter f, AoTaps taps, int pitch,
    uint8_t* __restrict__ out) {
  extern __shared__ uint32_t lds[];
  const int r = f.radius, side = kGuidedTile + 2 * r, plane = side * pitch;
  const int x0 = (int)blockIdx.x * kGuidedTile, y0 = (int)blockIdx.y * kGuidedTile;
  for (int i = threadIdx.x; i < side * side; i += kGuidedThreads) {
    const int ty = i / side, tx = i - ty * side;
    const int gx = x0 - r + tx, gy = y0 - r + ty;
    uint32_t w[8] = {0u, (uint32_t)INT_MIN, 0u, 0u, 0u, 0u, 0u, 0u};
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t g = (size_t)gy * (size_t)W + (size_t)gx;
      const uint32_t* p = (const uint32_t*)P + 3 * g;
      const uint32_t* n = (const uint32_t*)N + 3 * g;
      w[0] = ao[g];
      w[1] = (uint32_t)id[g];
      w[2] = p[0], w[3] = p[1], w[4] = p[2];
      w[5] = n[0], w[6] = n[1], w[7] = n[2];
    }
    uint32_t* d = lds + ty * pitch + tx;
    for (int k = 0; k < 8; ++k) d[k * plane] = w[k];
  }
  __syncthreads();
  int lx, ly;
  guided_pixel(lx, ly);
  const int x = x0 + lx, y = y0 + ly;
  if (x >= W || y >= H) return;
  const uint32_t* c = lds + (ly + r) * pitch + (lx + r);
  const uint32_t rec_p = c[0];
  const int id_p = (int)c[plane];
  unsigned byte;
  if (id_p < 0) {
    byte = guided_byte(rec_p & 0xffffu, rec_p >> 16);
  } else {
    const float* cf = (const float*)c;
    const V3 Pp = v3(cf[2 * plane], cf[3 * plane], cf[4 * plane]);
    const V3 Np = v3(cf[5 * plane], cf[6 * plane], cf[7 * plane]);
    unsigned O = 0u, R = 0u;
    for (int dy = -r; dy <= r; ++dy) {                        // uniform
      const unsigned wy = taps.t[dy < 0 ? -dy : dy];
      for (int dx = -r; dx <= r; ++dx) {                      // uniform
        const unsigned w = wy * taps.t[dx < 0 ? -dx : dx];
        const uint32_t* q = c + dy * pitch + dx;
        bool accept = dx == 0 && dy == 0;
        if (!accept && (int)q[plane] == id_p) {
          const float* qf = (const float*)q;
          const V3 Nq = v3(qf[5 * plane], qf[6 * plane], qf[7 * plane]);
          if (dot(Np, Nq) >= f.nmin) {
            const V3 Pq = v3(qf[2 * plane], qf[3 * plane], qf[4 * plane]);
            accept = fabsf(dot(Np, sub(Pq, Pp))) <= f.dplane;
          }
        }
        if (accept) {
          const uint32_t rec = q[0];
          O += w * (rec & 0xffffu);
          R += w * (rec >> 16);
        }
      }
    }
    byte = pooled_byte(O, R);
  }
  out[(size_t)y * (size_t)W + (size_t)x] = (uint8_t)byte;
}
#else
// The measurement variant: the same rule with every neighbour read from global memory.
__global__ void __launch_bounds__(kGuidedThreads) k_ao_filter(
    const uint32_t* __restrict__ ao, const int32_t* __restrict__ id, const float* __restrict__ P,
    const float* __restrict__ N, int W, int H, AoFilter f, AoTaps taps, int /*pitch*/,
    uint8_t* __restrict__ out) {
  int lx, ly;
  guided_pixel(lx, ly);
  const int r = f.radius;
  const int x = (int)blockIdx.x * kGuidedTile + lx, y = (int)blockIdx.y * kGuidedTile + ly;
  if (x >= W || y >= H) return;
  const size_t p = (size_t)y * (size_t)W + (size_t)x;
  const uint32_t rec_p = ao[p];
  const int id_p = id[p];
  unsigned byte;
  if (id_p < 0) {
    byte = guided_byte(rec_p & 0xffffu, rec_p >> 16);
  } else {
    const V3 Pp = v3(P[3 * p], P[3 * p + 1], P[3 * p + 2]);
    const V3 Np = v3(N[3 * p], N[3 * p + 1], N[3 * p + 2]);
    unsigned O = 0u, R = 0u;
    for (int dy = -r; dy <= r; ++dy) {
      const unsigned wy = taps.t[dy < 0 ? -dy : dy];
      for (int dx = -r; dx <= r; ++dx) {
        const unsigned w = wy * taps.t[dx < 0 ? -dx : dx];
        const int qx = x + dx, qy = y + dy;
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
        bool accept = dx == 0 && dy == 0;
        if (!accept && id[q] == id_p) {
          const V3 Nq = v3(N[3 * q], N[3 * q + 1], N[3 * q + 2]);
          if (dot(Np, Nq) >= f.nmin) {
            const V3 Pq = v3(P[3 * q], P[3 * q + 1], P[3 * q + 2]);
            accept = fabsf(dot(Np, sub(Pq, Pp))) <= f.dplane;
          }
        }
        if (accept) {
          const uint32_t rec = ao[q];
          O += w * (rec & 0xffffu);
          R += w * (rec >> 16);
        }
      }
    }
    byte = pooled_byte(O, R);
  }
  out[p] = (uint8_t)byte;
}
#endif

// k_ao_compose: 1 + 4 + 3 bytes in and 3 out a pixel, memory-bound.  Every workgroup builds the
// scene's table a[k][c] = quant(ambient[c] * diffuse[k][c]) in LDS (kComposeTable shapes; a
// larger scene's lanes compute their own entry), then one lane a pixel in row-major order:
// id and ao are read once, out[c] = min(255, in[c] + (a[id][c] * ao + 127) / 255), and an id
// outside [0, n) copies the pixel.  No alignment is assumed of any pointer: byte accesses.
constexpr int kComposeTable = 256;

__global__ void __launch_bounds__(kGuidedThreads) k_ao_compose(
    const float* __restrict__ diffuse, int n, Ambient amb, const int32_t* __restrict__ id,
    const uint8_t* __restrict__ ao, const uint8_t* in, uint8_t* out, unsigned long long pixels) {
  __shared__ uint32_t table[kComposeTable];
  const int staged = n < kComposeTable ? n : kComposeTable;
  for (int k = threadIdx.x; k < staged; k += kGuidedThreads) {
    const float* d = diffuse + 3 * (size_t)k;
    table[k] = (uint32_t)quant(amb.c[0] * d[0]) | ((uint32_t)quant(amb.c[1] * d[1]) << 8) |
               ((uint32_t)quant(amb.c[2] * d[2]) << 16);
  }
  __syncthreads();
  const unsigned long long p = (unsigned long long)blockIdx.x * kGuidedThreads + threadIdx.x;
  if (p >= pixels) return;
  const int k = id[p];
  const uint8_t* src = in + 3 * p;
  unsigned c0 = src[0], c1 = src[1], c2 = src[2];
  if (k >= 0 && k < n) {
    uint32_t a;
    if (k < staged) {
      a = table[k];
    } else {
      const float* d = diffuse + 3 * (size_t)k;
      a = (uint32_t)quant(amb.c[0] * d[0]) | ((uint32_t)quant(amb.c[1] * d[1]) << 8) |
          ((uint32_t)quant(amb.c[2] * d[2]) << 16);
    }
    const unsigned o = ao[p];
    c0 += ((a & 0xffu) * o + 127u) / 255u;
    c1 += (((a >> 8) & 0xffu) * o + 127u) / 255u;
    c2 += ((a >> 16) * o + 127u) / 255u;
    c0 = c0 > 255u ? 255u : c0;
    c1 = c1 > 255u ? 255u : c1;
    c2 = c2 > 255u ? 255u : c2;
  }
  uint8_t* dst = out + 3 * p;
  dst[0] = (uint8_t)c0, dst[1] = (uint8_t)c1, dst[2] = (uint8_t)c2;
}

bool guided_image(int W, int H) {
  return W >= 1 && H >= 1 && W <= kGuidedMaxSide && H <= kGuidedMaxSide;
}

}  // namespace

hipError_t launch_ao_filter(const void* ao, const int32_t* id, const float* P, const float* N,
                            int W, int H, const AoFilter& f, uint8_t* out, hipStream_t stream) {
  if (!ao || ((uintptr_t)ao & 3u) || !id || !P || !N || !out || !guided_image(W, H) ||
      f.radius < 0 || f.radius > kAoFilterMaxRadius)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((W + kGuidedTile - 1) / kGuidedTile),
                  (unsigned)((H + kGuidedTile - 1) / kGuidedTile));
  const int pitch = ao_filter_pitch(f.radius), side = kGuidedTile + 2 * f.radius;
  const size_t lds = RC_AO_FILTER_DIRECT ? 0 : (size_t)side * pitch * 8 * sizeof(uint32_t);
  AoTaps taps;
  for (int d = 0; d <= kAoFilterMaxRadius; ++d) taps.t[d] = d <= f.radius ? f.taps[d] : 0u;
  hipLaunchKernelGGL(k_ao_filter, grid, dim3(kGuidedThreads), lds, stream, (const uint32_t*)ao, id,
                     P, N, W, H, f, taps, pitch, out);
  return hipGetLastError();
}

hipError_t launch_ao_compose(const float* diffuse, int n_shapes, const Ambient& ambient,
                             const int32_t* id, const uint8_t* ao, const uint8_t* in, uint8_t* out,
                             int W, int H, hipStream_t stream) {
  if (!diffuse || n_shapes < 0 || !id || !ao || !in || !out || !guided_image(W, H))
    return hipErrorInvalidValue;
  const unsigned long long pixels = (unsigned long long)W * (unsigned long long)H;
  const unsigned long long blocks = (pixels + kGuidedThreads - 1) / kGuidedThreads;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ao_compose, dim3((unsigned)blocks), dim3(kGuidedThreads), 0, stream, diffuse,
                     n_shapes, ambient, id, ao, in, out, pixels);
  return hipGetLastError();
}

}  // namespace rc
