// rc_sample_kernels.hip — the sampling family of the MI355X raycaster (gfx950): every kernel
// that shoots more than one ray a pixel or fewer pixels than the image, and their launchers.
// They share the renderer's pixel routines (rc_device.hpp, rc_cudasem.hpp) and its tiles
// (rc_pixel.hpp); k_render, k_render_cuda and the parity pipeline are in rc_kernels.hip.  The
// entry points that drive these launchers are in rc_sampling.hip.
//
//   k_render_ssaa fast mode with s x s supersampling: one lane per subsample, the box filter
//                 across the lanes of a wave, one store per output pixel.
//   k_box_down    the box filter of an s*W x s*H image in memory (parity and cuda modes).
//   k_aa_mark / k_aa_refine
//                 adaptive supersampling (fast and cuda modes): the list of the one-ray image's
//                 edge pixels (3x3 contrast >= t), then the s x s subsamples of those pixels only.
//   k_rates_render / k_rates_refine8
//                 supersampling by the caller's per-pixel rate map (fast and cuda modes): the
//                 rate-1 pixels and one list per factor, refined by k_aa_refine (2, 4) and by
//                 k_rates_refine8 (8, whose list grows downwards).
//   k_pattern / k_pattern_list
//                 sparse sample patterns (fast and cuda modes): n samples of a pixel's g x g
//                 lattice, n lanes a pixel; every pixel, or the pixels k_aa_mark listed.
//   k_accum / k_accum_list / k_accum_resolve
//                 progressive supersampling (fast and cuda modes): a pass adds samples to the
//                 caller's per-pixel records and stores the mean; every pixel, the listed
//                 pixels, or the means alone.
//   k_window / k_accum_win / k_accum_list_win
//                 windows of a virtual image (fast and cuda modes): k_render_ssaa's and the
//                 accumulation passes' samples for a rectangle of a larger image.
//   k_accum_move / k_accum_exposed
//                 scrolling an accumulated view: the kept rectangle's records and bytes moved,
//                 then samples for the exposed pixels only.
//   k_gbuffer / k_gbuffer_points / k_id_edge_rates
//                 the primary-visibility G-buffer (fast, parity and cuda modes): the primary hit's
//                 shape, distance, point and normal per pixel of a window or per picked point,
//                 nothing shaded; and the rate map of the id plane's 3 x 3 edges.
//   k_view / k_rays
//                 rays that are not the pinhole grid's (fast and cuda modes): k_window through a
//                 view matrix, and a batch of the caller's own directions, one lane each, with
//                 the colour before quantisation, its bytes and the primary hit's record.
//   k_camera / k_rays_from
//                 the same two with an origin (fast mode): every ray of a frame from one eye,
//                 and a batch with an origin per ray.
//   k_accum_cam / k_accum_list_cam
//                 the accumulation passes through free cameras (fast mode): k_accum_win's and
//                 k_accum_list_win's layout with sample j shot k_camera's way through camera j
//                 of a kernel argument of up to 16 cameras.
//   k_ao / k_occluded_rays / k_ao_resolve
//                 any-hit visibility (fast mode): a camera frame's primary hit and the blocked /
//                 open count of up to 64 directions around it, added to the caller's per-pixel
//                 records; a batch of the caller's own rays, one byte each; the records' bytes.
//   k_camera_gbuffer
//                 the G-buffer through a free camera (fast mode): k_ao's primary hit, stored.
#include <cstring>

#include "rc_cudasem.hpp"
#include "rc_lists.hpp"
#include "rc_pixel.hpp"

namespace rc {

// ---------------------------------------- one subsample, for the supersampling kernels --
// The quantised channels of subsample (xs, ys) of the image whose camera is `cam`, in fast
// mode's arithmetic or (kCuda) the CUDA port's (k_render_cuda's pixel routine), packed for the
// sums below: R | G << 16 and B (a channel's sum over a wave is <= 64 * 255).
template <bool kCuda>
__device__ __forceinline__ void sample_shoot(const Scene& sc, const Cam& cam, int xs, int ys,
                                             int maxrec, unsigned long long* __restrict__ zcount,
                                             unsigned& rg, unsigned& b) {
  V3 c;
  if constexpr (kCuda) {
    c = cusem::render_pixel(sc, cam, xs, ys, maxrec - 1);
  } else {
    int zero = 0;
    const V3 d = primary_dir(cam, xs, ys, zero);
    PixelOut po;
    shoot<kModeFast>(sc, d, maxrec, v3(0.0f, 0.0f, 0.0f), po, zero);
    c = po.rgb;
    flush_events(zero, zcount);
  }
  rg = (unsigned)quant(c.x) | ((unsigned)quant(c.y) << 16);
  b = quant(c.z);
}
// The sums over the 1 << ln lanes of a group (xor butterflies over the lane bits 1 .. n/2).
// Called by every lane of the wave.
__device__ __forceinline__ void sample_reduce(unsigned& rg, unsigned& b, int ln) {
  for (int m = 1; m < (1 << ln); m <<= 1) {
    rg += __shfl_xor(rg, m, 64);
    b += __shfl_xor(b, m, 64);
  }
}
// The rounded mean of 1 << ln samples, (sum + n/2) >> ln per channel, stored at q.
__device__ __forceinline__ void sample_store(uint8_t* __restrict__ q, unsigned rg, unsigned b,
                                             int ln) {
  const unsigned half = 1u << (ln - 1);
  q[0] = (uint8_t)(((rg & 0xffffu) + half) >> ln);
  q[1] = (uint8_t)(((rg >> 16) + half) >> ln);
  q[2] = (uint8_t)((b + half) >> ln);
}

// ------------------------------------------------- fast mode, supersampled (ssaa) --
// k_render over the subsample grid of an s x s supersampled image (s = 1 << ls; 2, 4 or 8):
// one lane shoots one subsample with the camera of the s*W x s*H image, the same tiles as
// k_render in subsample coordinates.  lane = 8 * row + col inside a wave tile and s divides 8,
// so the s x s subsamples of an output pixel are lanes of one wave: their quantised channels
// are summed with xor butterflies over the column bits (1 .. s/2) and the row bits (8 .. 4s),
// and the group's first lane stores the rounded mean, (sum + s*s/2) / (s*s).  The subsample
// image is never written.  W, nrows, row0 and row_step are in output pixels: output row r
// covers subsample rows s * (row0 + r * row_step) + j, j < s.
// Tile origins are multiples of 8 subsamples, so a group is wholly inside the image or wholly
// outside it: outside lanes skip shoot, add zeros in the butterflies (which every lane of the
// wave executes) and store nothing.
template <bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_render_ssaa(
    Scene sc, Cam cam, int W, int ls, int row0, int row_step, int nrows, int maxrec,
    uint8_t* __restrict__ out, unsigned long long* __restrict__ zcount) {
  if (!RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // no cross-term-free form here (RC_X0_*)
  __shared__ StageBuf<kStage> stage;
  stage_scene<kStage>(sc, stage);
  int lx, ly;
  tile_pixel(lx, ly);
  int bx, by;
  xcd_tile<0>(bx, by);
  const int s = 1 << ls;
  const int xs = bx * kTileW + lx;   // subsample column
  const int rs = by * kTileH + ly;   // subsample row of the local (shard) rows
  // only xs and rs stay live across shoot (k_render's x and r): the output pixel, the bounds
  // test and the group's first lane all follow from them
  const bool inside = (xs >> ls) < W && (rs >> ls) < nrows;
  unsigned rg = 0u, b = 0u;          // R | G << 16 and B: a channel's sum is <= 64 * 255
  if (inside) {
    const int y = ((row0 + (rs >> ls) * row_step) << ls) + (rs & (s - 1));
    int zero = 0;
    const V3 d = primary_dir(cam, xs, y, zero);
    PixelOut po;
    shoot<kModeFast>(sc, d, maxrec, v3(0.0f, 0.0f, 0.0f), po, zero);
    rg = (unsigned)quant(po.rgb.x) | ((unsigned)quant(po.rgb.y) << 16);
    b = quant(po.rgb.z);
    flush_events(zero, zcount);
  }
  for (int m = 1; m < s; m <<= 1) {       // columns of the group
    rg += __shfl_xor(rg, m, 64);
    b += __shfl_xor(b, m, 64);
  }
  for (int m = 8; m < 8 * s; m <<= 1) {   // rows of the group
    rg += __shfl_xor(rg, m, 64);
    b += __shfl_xor(b, m, 64);
  }
  // the group's first lane (tile origins are multiples of 8, so of s)
  if (inside && ((xs | rs) & (s - 1)) == 0) {
    const unsigned half = 1u << (2 * ls - 1);
    const int x = xs >> ls, r = rs >> ls;   // r: local (shard) output row
    uint8_t* p = out + ((size_t)r * W + x) * 3;
    p[0] = (uint8_t)(((rg & 0xffffu) + half) >> (2 * ls));
    p[1] = (uint8_t)(((rg >> 16) + half) >> (2 * ls));
    p[2] = (uint8_t)((b + half) >> (2 * ls));
  }
}

// Box filter of the two-pass path (parity and cuda modes, whose s*W x s*H image exists in
// memory): dst pixel (x, y) = the rounded mean of src's s x s block at (s*x, s*y), per channel,
// (sum + s*s/2) / (s*s).  One thread per output pixel; src is (s*W) x (s*H), dst W x H.
__global__ void __launch_bounds__(256) k_box_down(const uint8_t* __restrict__ src, int W, int H,
                                                  int ls, uint8_t* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)W * H) return;
  const int s = 1 << ls;
  const size_t y = i / (size_t)W, x = i % (size_t)W;
  const size_t srow = (size_t)W * s * 3;
  const uint8_t* p = src + y * s * srow + x * s * 3;
  unsigned r = 0u, g = 0u, b = 0u;
  for (int j = 0; j < s; ++j) {
    const uint8_t* q = p + (size_t)j * srow;
    for (int k = 0; k < s; ++k) {
      r += q[3 * k];
      g += q[3 * k + 1];
      b += q[3 * k + 2];
    }
  }
  const unsigned half = 1u << (2 * ls - 1);
  uint8_t* d = dst + i * 3;
  d[0] = (uint8_t)((r + half) >> (2 * ls));
  d[1] = (uint8_t)((g + half) >> (2 * ls));
  d[2] = (uint8_t)((b + half) >> (2 * ls));
}

// ------------------------------------------- adaptive supersampling (fast, cuda) --
// rc_options.ssaa = RC_SSAA_ADAPTIVE(s, t): the one-ray image A is rendered into `out` by
// k_render / k_render_cuda, k_aa_mark lists the pixels of A whose 3x3 contrast reaches t, and
// k_aa_refine shoots the s x s subsamples of the listed pixels only and stores their box filter
// over A's pixel.  Mark reads neighbours that refine overwrites, so the two are separate
// launches on one stream: the list is complete before the first refined store.
//
// k_aa_mark, with mark_load, MarkRow, mark_row, kMarkBlock and kMarkRows, is in rc_lists.hpp, where
// its scheme is described: the plane-by-plane test harness compiles the same text.

// k_aa_refine: over the list, not the image.  A wave serves 64 / (s*s) listed pixels per step
// (s = 1 << ls: 16, 4 or 1): lane l belongs to group l / (s*s) and shoots subsample
// (i, j) = ((l % (s*s)) % s, (l % (s*s)) / s) of its group's pixel (x, y), that is the pixel
// (s*x + i, s*y + j) of the s*W x s*H image with that image's camera (`cam`), exactly as
// k_render_ssaa / the two-pass path do, so every subsample byte is that image's byte.  The
// quantised channels are summed over the group with xor butterflies over the lane bits
// 1 .. s*s/2 and the group's first lane stores (sum + s*s/2) / (s*s) over A's pixel.
// The list's length is read from device memory (k_aa_mark's counter) and the grid is a fixed
// number of workgroups whose waves stride over the list, so the host never waits between mark
// and refine.  A wave's trip count depends on the wave alone, so all its lanes execute every
// butterfly; lanes past the list's end shoot nothing, add zeros and store nothing.
// kCuda: the CUDA port's arithmetic (k_render_cuda's pixel routine) instead of fast mode.
template <bool kCuda, bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_aa_refine(
    Scene sc, Cam cam, int W, int ls, int maxrec, const uint32_t* __restrict__ list,
    const unsigned* __restrict__ count, uint8_t* __restrict__ out,
    unsigned long long* __restrict__ zcount) {
  if (!kCuda && !RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  __shared__ StageBuf<kStage> stage;
  stage_scene<kStage>(sc, stage);   // its barrier comes before the loop: every thread is here
  const unsigned n = *count;
  const int lane = threadIdx.x & 63;
  const unsigned per = 64u >> (2 * ls);                    // listed pixels per wave step
  const unsigned sub = (unsigned)lane & ((1u << (2 * ls)) - 1u);   // subsample within the group
  // wave-uniform by construction: told to the compiler, so the loop's counters stay scalar
  const unsigned wave =
      __builtin_amdgcn_readfirstlane(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));
  const unsigned step = gridDim.x * (kBlock / 64) * per;   // <= 4096 * 4 * 16
  // 64-bit index: n + step may pass 2^32
  for (unsigned long long first = (unsigned long long)wave * per; first < n; first += step) {
    const unsigned long long k = first + ((unsigned)lane >> (2 * ls));
    const bool live = k < n;
    unsigned p = 0u, rg = 0u, b = 0u;   // R | G << 16 and B: a channel's sum is <= 64 * 255
    if (live) {
      p = list[k];
      const int xs = (int)((p % (unsigned)W) << ls) + (int)(sub & ((1u << ls) - 1u));
      const int ys = (int)((p / (unsigned)W) << ls) + (int)(sub >> ls);
      sample_shoot<kCuda>(sc, cam, xs, ys, maxrec, zcount, rg, b);
    }
    sample_reduce(rg, b, 2 * ls);
    if (live && sub == 0u) {
      // the entry is read again (opaque index) rather than kept in a register across shoot,
      // where the kernel sits at the 128-register edge
      unsigned g = (unsigned)lane >> (2 * ls);
      asm volatile("" : "+v"(g));
      p = list[first + g];
      sample_store(out + (size_t)p * 3, rg, b, 2 * ls);
    }
  }
}

// ---------------------------------------- rate-map supersampling (fast, cuda) --
// rc_render_rates*: the caller's map gives every pixel a rate in {0, 1, 2, 4, 8} (one byte per
// pixel, row-major): 0 leaves the pixel's bytes alone, 1 is the one-ray pixel, s > 1 the ssaa = s
// pixel.  k_rates_render shoots the rate-1 pixels and bins the others into one list per factor;
// k_aa_refine (rates 2 and 4) and k_rates_refine8 then shoot the listed pixels' subsamples.  No
// pixel is in two classes and nobody reads a pixel, so the stream order of the launches is all
// the ordering there is.
//
// k_rates_render: k_render's grid and tiles (one lane per pixel) for the rate-1 pixels.  The
// binning comes first, so nothing of it is live across shoot, and it does not follow the tiles:
// the map is cut into chunks of kRateChunk * 256 consecutive pixels (row-major, so the byte loads
// are contiguous) and one workgroup in every kRateChunk takes a chunk, so a class's counter gets
// one atomicAdd per chunk and not one per wave (same-address atomics were what the first form's
// time followed).  The chunk's workgroup counts first: per wave and step
// a ballot per class, the waves' sums through LDS, one atomicAdd per class by one thread; then it
// reads the chunk again and every flagged lane writes its pixel index y*W + x at the class's base
// + the flagged pixels of the waves and steps before it + the popcount of the flagged lanes below
// it (k_aa_mark's reservation, one level up).  Every lane of a wave reaches the ballots; lanes
// past the map flag nothing.  The duty rotates over the eight residues of the workgroup index, so
// it does not fall on one XCD.  cnt: [0] [1] [2] the lengths of the rate-2, rate-4 and rate-8
// lists, [3] the rate-1 pixels, [4] the map bytes that are no rate (those pixels are left alone,
// like rate 0).  The rate-2 list grows upwards from list2up, the rate-8 list downwards from
// list8down (the two ends of one W*H-entry buffer: together they never hold more than W*H
// entries), the rate-4 list upwards from list4.
// A workgroup without a rate-1 pixel ends before stage_scene; the decision is one
// __syncthreads_or, so stage_scene's barrier stays uniform.  A rate-1 lane stores its own three
// bytes: a wider store would write into a neighbour that may have rate 0.
template <bool kCuda, bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_rates_render(
    Scene sc, Cam cam, int W, int H, int maxrec, const uint8_t* __restrict__ rates,
    uint8_t* __restrict__ out, uint32_t* __restrict__ list2up, uint32_t* __restrict__ list4,
    uint32_t* __restrict__ list8down, unsigned* __restrict__ cnt,
    unsigned long long* __restrict__ zcount) {
  if (!kCuda && !RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  __shared__ StageBuf<kStage> stage;
  __shared__ unsigned wsum[kBlock / 64][5];   // per wave: the chunk's pixels per counter of cnt
  __shared__ unsigned wbase[3];               // the chunk's first slot in each list
#include "rc_rates_bin.inc"
  int lx, ly;
  tile_pixel(lx, ly);
  int bx, by;
  xcd_tile<0>(bx, by);
  const int x = bx * kTileW + lx;
  const int y = by * kTileH + ly;
  const bool one = x < W && y < H && rates[(size_t)y * W + x] == 1;
  if (!__syncthreads_or(one ? 1 : 0)) return;   // uniform: no rate-1 pixel in this tile
  stage_scene<kStage>(sc, stage);
  if (!one) return;
  V3 c;
  if constexpr (kCuda) {
    c = cusem::render_pixel(sc, cam, x, y, maxrec - 1);
  } else {
    int zero = 0;
    const V3 d = primary_dir(cam, x, y, zero);
    PixelOut po;
    shoot<kModeFast>(sc, d, maxrec, v3(0.0f, 0.0f, 0.0f), po, zero);
    c = po.rgb;
    flush_events(zero, zcount);
  }
  store_rgb(out + ((size_t)y * W + x) * 3, c);
}

// k_rates_refine8: k_aa_refine at s = 8 over a list that grows downwards (entry k is
// last[-k]): a wave serves one listed pixel per step, lane l shoots subsample (l % 8, l / 8) of
// it with the camera of the 8*W x 8*H image, the quantised channels are summed over the wave
// with xor butterflies and lane 0 stores (sum + 32) / 64.  The entry is wave-uniform and stays
// in a scalar register across shoot.  The list's length is read on the device; the grid is a
// fixed number of workgroups whose waves stride over the list.
template <bool kCuda, bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_rates_refine8(
    Scene sc, Cam cam, int W, int maxrec, const uint32_t* __restrict__ last,
    const unsigned* __restrict__ count, uint8_t* __restrict__ out,
    unsigned long long* __restrict__ zcount) {
  if (!kCuda && !RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  __shared__ StageBuf<kStage> stage;
  const unsigned n = *count;
  if (n == 0u) return;   // uniform over the grid: an empty list costs its launch
  stage_scene<kStage>(sc, stage);
  const int lane = threadIdx.x & 63;
  const unsigned wave =
      __builtin_amdgcn_readfirstlane(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));
  const unsigned step = gridDim.x * (kBlock / 64);
  // 64-bit index: n + step may pass 2^32
  for (unsigned long long k = wave; k < n; k += step) {
    const unsigned p = __builtin_amdgcn_readfirstlane(*(last - (size_t)k));
    const int xs = (int)((p % (unsigned)W) << 3) + (lane & 7);
    const int ys = (int)((p / (unsigned)W) << 3) + (lane >> 3);
    V3 c;
    if constexpr (kCuda) {
      c = cusem::render_pixel(sc, cam, xs, ys, maxrec - 1);
    } else {
      int zero = 0;
      const V3 d = primary_dir(cam, xs, ys, zero);
      PixelOut po;
      shoot<kModeFast>(sc, d, maxrec, v3(0.0f, 0.0f, 0.0f), po, zero);
      c = po.rgb;
      flush_events(zero, zcount);
    }
    unsigned rg = (unsigned)quant(c.x) | ((unsigned)quant(c.y) << 16);   // sums <= 64 * 255
    unsigned b = quant(c.z);
    for (int m = 1; m < 64; m <<= 1) {
      rg += __shfl_xor(rg, m, 64);
      b += __shfl_xor(b, m, 64);
    }
    if (lane == 0) {
      uint8_t* q = out + (size_t)p * 3;
      q[0] = (uint8_t)(((rg & 0xffffu) + 32u) >> 6);
      q[1] = (uint8_t)(((rg >> 16) + 32u) >> 6);
      q[2] = (uint8_t)((b + 32u) >> 6);
    }
  }
}

// ------------------------------------- sparse sample patterns (fast, cuda) --
// rc_render_pattern*: n samples of a pixel on its g x g subsample lattice (rc_pattern in
// include/raycast_hip.h; g = 1 << lg in {2, 4, 8}, n = 1 << ln in {2, 4, 8, 16}).  Sample k of
// pixel (x, y) is pixel (g*x + px[k], g*y + py[k]) of the g*W x g*H image, shot with that image's
// camera (`cam`) exactly as k_render_ssaa and k_aa_refine shoot theirs, so every sample byte is
// that image's byte; the image itself is never stored.
// Lane l of a wave belongs to pixel group l / n and shoots sample l % n.  The pattern travels as
// two 64-bit words of 4-bit entries (entry k in bits 4k .. 4k+3 of PatWords::x and ::y), kernel
// arguments held in scalar registers: a lane takes its own entry with one shift, no table in
// memory or LDS.  The quantised channels are summed over the group with xor butterflies over the
// lane bits 1 .. n/2, packed R | G << 16 and B (a channel's sum is <= 16 * 255), and the group's
// first lane stores (sum + n/2) >> ln.  Every lane of a wave executes every butterfly; lanes whose
// group is outside the image or past the list shoot nothing, add zeros and store nothing.  A
// group's lanes share one pixel, so a group is wholly inside or wholly outside.
struct PatWords {
  unsigned long long x, y;
};
__device__ __forceinline__ int pat_entry(unsigned long long word, unsigned k) {
  return (int)((word >> (4u * k)) & 15ull);
}

// The wave block of the dense form: a wave's 64 / n pixels are a compact bw x bh block,
//   n = 2: 8 x 4    n = 4: 4 x 4    n = 8: 4 x 2    n = 16: 2 x 2     (bw >= bh, both powers of two)
// and a workgroup's four waves sit 2 x 2, so a workgroup owns a tile of 2*bw x 2*bh = 256 / n
// output pixels: 16 x 8, 8 x 8, 8 x 4, 4 x 4.
__host__ __device__ constexpr int pat_lbw(int ln) { return (7 - ln) / 2; }   // log2 bw
__host__ __device__ constexpr int pat_lbh(int ln) { return (6 - ln) / 2; }   // log2 bh
static_assert(pat_lbw(1) == 3 && pat_lbh(1) == 2 && pat_lbw(2) == 2 && pat_lbh(2) == 2 &&
              pat_lbw(3) == 2 && pat_lbh(3) == 1 && pat_lbw(4) == 1 && pat_lbh(4) == 1,
              "a wave's 64 / n pixels");

// Dense form (threshold 0): every pixel of the image, one workgroup per tile, the tiles taken
// through xcd_tile in the grid's own order like k_render's.  The tiles are small, so a 128-byte
// line of the framebuffer spans several of them, but k_phase_a's order (chunks of 8 horizontally
// adjacent tiles share an L2) measured slower at every n (quadric, rgss4: 1024^2 0.189 against
// 0.176 ms, 2048^2 0.659 against 0.635 ms), as it did for k_render.
template <bool kCuda, bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_pattern(
    Scene sc, Cam cam, int W, int H, int lg, int ln, PatWords pat, int maxrec,
    uint8_t* __restrict__ out, unsigned long long* __restrict__ zcount) {
  if (!kCuda && !RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  __shared__ StageBuf<kStage> stage;
  stage_scene<kStage>(sc, stage);
  int bx, by;
  xcd_tile<0>(bx, by);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lbw = pat_lbw(ln), lbh = pat_lbh(ln);
  const int grp = lane >> ln;                                    // the wave's pixel group
  const unsigned k = (unsigned)lane & ((1u << ln) - 1u);         // the lane's sample
  const int x = (((bx << 1) + (wave & 1)) << lbw) + (grp & ((1 << lbw) - 1));
  const int y = (((by << 1) + (wave >> 1)) << lbh) + (grp >> lbw);
  const bool inside = x < W && y < H;
  unsigned rg = 0u, b = 0u;
  if (inside)
    sample_shoot<kCuda>(sc, cam, (x << lg) + pat_entry(pat.x, k), (y << lg) + pat_entry(pat.y, k),
                     maxrec, zcount, rg, b);
  sample_reduce(rg, b, ln);
  if (inside && k == 0u) sample_store(out + ((size_t)y * W + x) * 3, rg, b, ln);
}

// List form (threshold t > 0): over k_aa_mark's list like k_aa_refine, 64 / n listed pixels per
// wave step; the list's length is read from device memory and the grid is a fixed number of
// workgroups whose waves stride over the list.  A wave's trip count depends on the wave alone.
template <bool kCuda, bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_pattern_list(
    Scene sc, Cam cam, int W, int lg, int ln, PatWords pat, int maxrec,
    const uint32_t* __restrict__ list, const unsigned* __restrict__ count,
    uint8_t* __restrict__ out, unsigned long long* __restrict__ zcount) {
  if (!kCuda && !RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  __shared__ StageBuf<kStage> stage;
  const unsigned n = *count;
  if (n == 0u) return;   // uniform over the grid: an empty list costs its launch
  stage_scene<kStage>(sc, stage);   // its barrier comes before the loop: every thread is here
  const int lane = threadIdx.x & 63;
  const unsigned per = 64u >> ln;                              // listed pixels per wave step
  const unsigned k = (unsigned)lane & ((1u << ln) - 1u);       // the lane's sample
  const int px = pat_entry(pat.x, k), py = pat_entry(pat.y, k);
  // wave-uniform by construction: told to the compiler, so the loop's counters stay scalar
  const unsigned wave =
      __builtin_amdgcn_readfirstlane(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));
  const unsigned step = gridDim.x * (kBlock / 64) * per;   // <= 4096 * 4 * 32
  // 64-bit index: n + step may pass 2^32
  for (unsigned long long first = (unsigned long long)wave * per; first < n; first += step) {
    const unsigned long long e = first + ((unsigned)lane >> ln);
    const bool live = e < n;
    unsigned rg = 0u, b = 0u;
    if (live) {
      const unsigned p = list[e];
      sample_shoot<kCuda>(sc, cam, (int)((p % (unsigned)W) << lg) + px,
                       (int)((p / (unsigned)W) << lg) + py, maxrec, zcount, rg, b);
    }
    sample_reduce(rg, b, ln);
    if (live && k == 0u) {
      // the entry is read again (opaque index) rather than kept in a register across shoot, as
      // in k_aa_refine
      unsigned g = (unsigned)lane >> ln;
      asm volatile("" : "+v"(g));
      sample_store(out + (size_t)list[first + g] * 3, rg, b, ln);
    }
  }
}

// ------------------------------- launchers of the kernels above (ssaa .. patterns) --
static int ssaa_log2(int ssaa) { return ssaa == 2 ? 1 : ssaa == 4 ? 2 : ssaa == 8 ? 3 : -1; }

hipError_t launch_render_ssaa(const LaunchScene& s, int W, int H, int ssaa, int row0, int row_step,
                              int nrows, int maxrec, uint8_t* out, unsigned long long* zcount,
                              hipStream_t stream) {
  const int ls = ssaa_log2(ssaa);
  if (ls < 0 || W > 0x7fffffff / ssaa || H > 0x7fffffff / ssaa || nrows > 0x7fffffff / ssaa)
    return hipErrorInvalidValue;
  const int sw = W * ssaa, sr = nrows * ssaa;
  dim3 grid((sw + kTileW - 1) / kTileW, (sr + kTileH - 1) / kTileH);
  if (grid.y > 65535u) return hipErrorInvalidValue;   // grid.y of k_render's tile layout
  dispatch(stage_fits(s), [&](auto st) {
    hipLaunchKernelGGL(k_render_ssaa<st.value>, grid, dim3(kBlock), 0, stream, make_scene(s),
                       make_cam(s, sw, H * ssaa), W, ls, row0, row_step, nrows, maxrec, out,
                       zcount);
  });
  return hipGetLastError();
}

hipError_t launch_box_down(const uint8_t* src, int W, int H, int ssaa, uint8_t* dst,
                           hipStream_t stream) {
  const int ls = ssaa_log2(ssaa);
  const size_t blocks = ((size_t)W * H + 255) / 256;
  if (ls < 0 || W <= 0 || H <= 0 || blocks > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_box_down, dim3((unsigned)blocks), dim3(256), 0, stream, src, W, H, ls, dst);
  return hipGetLastError();
}

hipError_t launch_aa_mark(const uint8_t* img, int W, int H, int threshold, uint32_t* list,
                          unsigned* count, hipStream_t stream) {
  if (W <= 0 || H <= 0 || threshold < 1 || threshold > 255) return hipErrorInvalidValue;
  if ((unsigned long long)W * (unsigned long long)H >= (1ull << 32))
    return hipErrorInvalidValue;   // pixel indices are uint32
  const unsigned long long tiles_x = ((unsigned long long)W + kMarkBlock - 1) / kMarkBlock;
  const unsigned long long tiles = tiles_x * (((unsigned long long)H + kMarkRows - 1) / kMarkRows);
  if (tiles > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_aa_mark, dim3((unsigned)tiles), dim3(kMarkBlock), 0, stream, img, W, H,
                     (unsigned)tiles_x, threshold, list, count);
  return hipGetLastError();
}

// the grid of a kernel that strides over a list of at most W*H pixels with `lanes` lanes a pixel
static int list_blocks(int W, int H, int lanes, int cus, int want) {
  if (want > 0) return want;
  // the kernels are compiled for RC_PHASE_A_WAVES waves per SIMD: that many 4-wave workgroups
  // per CU are resident at once; never more workgroups than the image has wave steps
  const unsigned long long per = 64u / (unsigned)lanes * (kBlock / 64);
  const unsigned long long need = ((unsigned long long)W * H + per - 1) / per;
  const unsigned long long cap = (unsigned long long)(cus > 0 ? cus : 256) * RC_PHASE_A_WAVES;
  return (int)(need < cap ? need : cap);
}

int aa_refine_blocks(int W, int H, int ssaa, int cus, int want) {
  return list_blocks(W, H, ssaa * ssaa, cus, want);
}

hipError_t launch_aa_refine(const LaunchScene& s, int W, int H, int ssaa, int maxrec,
                            const uint32_t* list, const unsigned* count, uint8_t* out,
                            unsigned long long* zcount, int blocks, hipStream_t stream,
                            bool cuda_sem) {
  const int ls = ssaa_log2(ssaa);
  if (ls < 0 || W <= 0 || H <= 0 || W > 0x7fffffff / ssaa || H > 0x7fffffff / ssaa ||
      blocks < 1 || blocks > 4096)
    return hipErrorInvalidValue;
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, W * ssaa, H * ssaa);   // the camera of the s*W x s*H image
  dispatch(cuda_sem, stage_fits(s), [&](auto cuda, auto st) {
    hipLaunchKernelGGL((k_aa_refine<cuda.value, st.value>), dim3((unsigned)blocks), dim3(kBlock),
                       0, stream, sc, cam, W, ls, maxrec, list, count, out, zcount);
  });
  return hipGetLastError();
}

int rates_supported(int W, int H) {
  if (W <= 0 || H <= 0) return 0;
  if ((unsigned long long)W * (unsigned long long)H >= (1ull << 32)) return 0;   // uint32 entries
  if (W > 0x7fffffff / 8 || H > 0x7fffffff / 8) return 0;   // subsample coordinates at rate 8
  return ((unsigned)H + kTileH - 1) / kTileH <= 65535u;     // grid.y of k_render's tile layout
}

hipError_t launch_rates_render(const LaunchScene& s, int W, int H, int maxrec,
                               const uint8_t* rates, uint8_t* out, uint32_t* list4,
                               uint32_t* list28, unsigned* cnt, unsigned long long* zcount,
                               hipStream_t stream, bool cuda_sem) {
  if (!rates_supported(W, H)) return hipErrorInvalidValue;
  dim3 grid((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH);
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, W, H);
  dispatch(cuda_sem, stage_fits(s), [&](auto cuda, auto st) {
    hipLaunchKernelGGL((k_rates_render<cuda.value, st.value>), grid, dim3(kBlock), 0, stream, sc,
                       cam, W, H, maxrec, rates, out, list28, list4,
                       list28 + ((size_t)W * H - 1), cnt, zcount);
  });
  return hipGetLastError();
}

hipError_t launch_rates_refine8(const LaunchScene& s, int W, int H, int maxrec,
                                const uint32_t* list28, const unsigned* count, uint8_t* out,
                                unsigned long long* zcount, int blocks, hipStream_t stream,
                                bool cuda_sem) {
  if (!rates_supported(W, H) || blocks < 1 || blocks > 4096) return hipErrorInvalidValue;
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, W * 8, H * 8);   // the camera of the 8*W x 8*H image
  const uint32_t* last = list28 + ((size_t)W * H - 1);
  dispatch(cuda_sem, stage_fits(s), [&](auto cuda, auto st) {
    hipLaunchKernelGGL((k_rates_refine8<cuda.value, st.value>), dim3((unsigned)blocks),
                       dim3(kBlock), 0, stream, sc, cam, W, maxrec, last, count, out, zcount);
  });
  return hipGetLastError();
}

static int pattern_log2(int v, int lo, int hi) {
  for (int l = lo; l <= hi; ++l)
    if (v == 1 << l) return l;
  return -1;
}

int pattern_supported(int W, int H, int g, int n, bool listed) {
  const int lg = pattern_log2(g, 1, 3), ln = pattern_log2(n, 1, 4);
  if (lg < 0 || ln < 0 || n > g * g) return 0;
  if (W <= 0 || H <= 0 || W > (1 << 28) / g || H > (1 << 28) / g) return 0;   // g*W, g*H within int
  if (!listed) {   // the dense form's tiles: grid.y, and xcd_tile's int tile index
    const unsigned long long tx = (((unsigned)W - 1u) >> (pat_lbw(ln) + 1)) + 1u;
    const unsigned long long ty = (((unsigned)H - 1u) >> (pat_lbh(ln) + 1)) + 1u;
    return ty <= 65535ull && tx * ty <= 0x7fffffffull;
  }
  if ((unsigned long long)W * (unsigned long long)H >= (1ull << 32)) return 0;   // uint32 entries
  return ((unsigned)H + kTileH - 1) / kTileH <= 65535u;   // grid.y of k_render's tile layout
}

int pattern_list_blocks(int W, int H, int n, int cus, int want) {
  return list_blocks(W, H, n, cus, want);
}

// entry k of the 4-bit words: v[k] < 16 for k < n <= 16 (pattern_supported's g <= 8)
static PatWords pattern_words(int n, const uint8_t* px, const uint8_t* py) {
  PatWords w{0ull, 0ull};
  for (int k = 0; k < n; ++k) {
    w.x |= (unsigned long long)(px[k] & 15u) << (4 * k);
    w.y |= (unsigned long long)(py[k] & 15u) << (4 * k);
  }
  return w;
}

hipError_t launch_pattern(const LaunchScene& s, int W, int H, int g, int n, const uint8_t* px,
                          const uint8_t* py, int maxrec, uint8_t* out,
                          unsigned long long* zcount, hipStream_t stream, bool cuda_sem) {
  if (!pattern_supported(W, H, g, n, false)) return hipErrorInvalidValue;
  const int lg = pattern_log2(g, 1, 3), ln = pattern_log2(n, 1, 4);
  const int ltw = pat_lbw(ln) + 1, lth = pat_lbh(ln) + 1;   // the workgroup's tile
  dim3 grid((((unsigned)W - 1u) >> ltw) + 1u, (((unsigned)H - 1u) >> lth) + 1u);
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, W * g, H * g);   // the camera of the g*W x g*H image
  const PatWords pat = pattern_words(n, px, py);
  dispatch(cuda_sem, stage_fits(s), [&](auto cuda, auto st) {
    hipLaunchKernelGGL((k_pattern<cuda.value, st.value>), grid, dim3(kBlock), 0, stream, sc, cam,
                       W, H, lg, ln, pat, maxrec, out, zcount);
  });
  return hipGetLastError();
}

hipError_t launch_pattern_list(const LaunchScene& s, int W, int H, int g, int n,
                               const uint8_t* px, const uint8_t* py, int maxrec,
                               const uint32_t* list, const unsigned* count, uint8_t* out,
                               unsigned long long* zcount, int blocks, hipStream_t stream,
                               bool cuda_sem) {
  if (!pattern_supported(W, H, g, n, true) || blocks < 1 || blocks > 4096)
    return hipErrorInvalidValue;
  const int lg = pattern_log2(g, 1, 3), ln = pattern_log2(n, 1, 4);
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, W * g, H * g);   // the camera of the g*W x g*H image
  const PatWords pat = pattern_words(n, px, py);
  dispatch(cuda_sem, stage_fits(s), [&](auto cuda, auto st) {
    hipLaunchKernelGGL((k_pattern_list<cuda.value, st.value>), dim3((unsigned)blocks),
                       dim3(kBlock), 0, stream, sc, cam, W, lg, ln, pat, maxrec, list, count, out,
                       zcount);
  });
  return hipGetLastError();
}

// -------------------------------------- progressive supersampling (fast, cuda) --
// rc_accum_pass_device / rc_render_accum (include/raycast_hip.h, rc_accum_px): the caller keeps
// one 8-byte record per pixel, the sums of the n sample bytes taken so far and n itself, and a
// pass adds `count` (1..16) further samples of a sequence on the g x g subsample lattice and
// stores the rounded mean of all of them.  Sample k of pixel (x, y) is pixel
// (g*x + px[k], g*y + py[k]) of the g*W x g*H image, shot with that image's camera (`cam`) through
// sample_shoot exactly as k_pattern shoots its samples, so every sample byte is that image's byte.
// The pass's slice of the sequence travels as PatWords (entry j of the words is sample first + j),
// read with a uniform index, so the positions stay in scalar registers.
//
// One lane per pixel shoots its `count` samples one after the other (a uniform trip count), so any
// count works, not only the powers of two a lane butterfly can reduce.  The record is a uint2:
// .x = sum[0] | sum[1] << 16, .y = sum[2] | n << 16.  sample_shoot's packing R | G << 16 and B
// adds onto it directly: a channel's sum is at most 256 * 255 = 65280 < 2^16, so nothing carries
// from R into G or from B into n.  A pixel with n + count > 256 is saturated: nothing of it
// changes, and the pass counts it in *sat (one ballot a wave, an atomic by its first lane only
// when the ballot is not empty).
__device__ __forceinline__ void accum_resolve_px(uint2 rec, uint8_t& r, uint8_t& g, uint8_t& b) {
  const unsigned n = rec.y >> 16;
  if (n == 0u) {
    r = g = b = 0;
    return;
  }
  const unsigned half = n >> 1;
  r = (uint8_t)(((rec.x & 0xffffu) + half) / n);
  g = (uint8_t)(((rec.x >> 16) + half) / n);
  b = (uint8_t)(((rec.y & 0xffffu) + half) / n);
}

// Called by every lane of the wave.
__device__ __forceinline__ void accum_count_saturated(bool saturated, unsigned* __restrict__ sat) {
  const unsigned long long m = __ballot(saturated);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(sat, (unsigned)__popcll(m));
}

// Dense pass: every pixel of the image, k_render's grid, tiles and framebuffer stores.  The
// record's n is read alone before the samples (two bytes; the branch keeps it in the exec mask,
// not in a register across shoot) and the whole record once after them: one 8-byte load and one
// 8-byte store a lane, adjacent lanes of a tile row adjacent in memory.  `reset`: the record is
// not read at all and counts as zero.
// (ox, oy): the window's origin in the virtual image, in pixels (k_accum: 0, 0; k_accum_win below).
template <bool kCuda, bool kStage>
__device__ __forceinline__ void accum_dense(
    Scene sc, Cam cam, int W, int H, int ox, int oy, int lg, int count, PatWords pat, int reset,
    int maxrec, uint2* __restrict__ acc, uint8_t* __restrict__ out,
    unsigned long long* __restrict__ zcount, unsigned* __restrict__ sat) {
  if (!kCuda && !RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  __shared__ StageBuf<kStage> stage;
  __shared__ TileBytes tb;
  tile_init(tb);
  stage_scene<kStage>(sc, stage);
  if (!kStage) __syncthreads();
  int lx, ly;
  tile_pixel(lx, ly);
  int bx, by;
  xcd_tile<0>(bx, by);
  const int x0 = bx * kTileW, y0 = by * kTileH;
  const int x = x0 + lx, y = y0 + ly;
  bool saturated = false;
  if (x < W && y < H) {
    const size_t p = (size_t)y * W + x;
    const unsigned had = reset ? 0u : (unsigned)((const uint16_t*)(acc + p))[3];
    saturated = had + (unsigned)count > 256u;
    if (!saturated) {
      unsigned rg = 0u, b = 0u;
      for (int k = 0; k < count; ++k) {   // uniform
        unsigned srg, sb;
        sample_shoot<kCuda>(sc, cam, ((ox + x) << lg) + pat_entry(pat.x, (unsigned)k),
                            ((oy + y) << lg) + pat_entry(pat.y, (unsigned)k), maxrec, zcount, srg,
                            sb);
        rg += srg;
        b += sb;
      }
      uint2 rec = make_uint2(0u, 0u);
      if (!reset) rec = acc[p];
      rec.x += rg;
      rec.y += b + ((unsigned)count << 16);
      acc[p] = rec;
      uint8_t r8, g8, b8;
      accum_resolve_px(rec, r8, g8, b8);
      tile_put_rgb(tb, lx, ly, r8, g8, b8, out + p * 3);
    } else if (RC_TILE_STAGE) {   // the staged tile's whole-row stores write this pixel too
      const uint8_t* q = out + p * 3;
      tile_put_rgb(tb, lx, ly, q[0], q[1], q[2], out + p * 3);
    }
  }
  accum_count_saturated(saturated, sat);
  if (!tile_last_wave(tb)) return;
  const int nx = W - x0 < kTileW ? W - x0 : kTileW;
  tile_write_rows<kTileW * 3 / 4>(tb.rgb, [&](int q) -> uint8_t* {
    return y0 + q < H ? out + ((size_t)(y0 + q) * W + x0) * 3 : nullptr;
  }, nx * 3);
}
template <bool kCuda, bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_accum(
    Scene sc, Cam cam, int W, int H, int lg, int count, PatWords pat, int reset, int maxrec,
    uint2* __restrict__ acc, uint8_t* __restrict__ out, unsigned long long* __restrict__ zcount,
    unsigned* __restrict__ sat) {
  accum_dense<kCuda, kStage>(sc, cam, W, H, 0, 0, lg, count, pat, reset, maxrec, acc, out, zcount,
                             sat);
}

// Masked pass: over k_aa_mark's list like k_pattern_list, one lane per listed pixel (64 a wave
// step); the list's length is read from device memory and the grid is a fixed number of
// workgroups whose waves stride over the list.  A wave's trip count depends on the wave alone, so
// every lane reaches the ballot.  A listed pixel is in the list once, so its record and its three
// bytes have one writer.
// (ox, oy): as accum_dense's.
template <bool kCuda, bool kStage>
__device__ __forceinline__ void accum_listed(
    Scene sc, Cam cam, int W, int ox, int oy, int lg, int count, PatWords pat, int maxrec,
    const uint32_t* __restrict__ list, const unsigned* __restrict__ nlist,
    uint2* __restrict__ acc, uint8_t* __restrict__ out, unsigned long long* __restrict__ zcount,
    unsigned* __restrict__ sat) {
  if (!kCuda && !RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  __shared__ StageBuf<kStage> stage;
  const unsigned n = *nlist;
  if (n == 0u) return;   // uniform over the grid: an empty list costs its launch
  stage_scene<kStage>(sc, stage);   // its barrier comes before the loop: every thread is here
  const int lane = threadIdx.x & 63;
  // wave-uniform by construction: told to the compiler, so the loop's counters stay scalar
  const unsigned wave =
      __builtin_amdgcn_readfirstlane(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));
  const unsigned step = gridDim.x * (kBlock / 64) * 64u;   // <= 4096 * 4 * 64
  // 64-bit index: n + step may pass 2^32
  for (unsigned long long first = (unsigned long long)wave * 64u; first < n; first += step) {
    const unsigned long long e = first + (unsigned)lane;
    bool saturated = false;
    if (e < n) {
      const unsigned p = list[e];
      saturated = (unsigned)((const uint16_t*)(acc + p))[3] + (unsigned)count > 256u;
      if (!saturated) {
        const int xs = (int)((p % (unsigned)W + (unsigned)ox) << lg);
        const int ys = (int)((p / (unsigned)W + (unsigned)oy) << lg);
        unsigned rg = 0u, b = 0u;
        for (int k = 0; k < count; ++k) {   // uniform
          unsigned srg, sb;
          sample_shoot<kCuda>(sc, cam, xs + pat_entry(pat.x, (unsigned)k),
                              ys + pat_entry(pat.y, (unsigned)k), maxrec, zcount, srg, sb);
          rg += srg;
          b += sb;
        }
        // the entry is read again (opaque index) rather than kept in a register across shoot, as
        // in k_aa_refine
        unsigned l = (unsigned)lane;
        asm volatile("" : "+v"(l));
        const size_t q = list[first + l];
        uint2 rec = acc[q];
        rec.x += rg;
        rec.y += b + ((unsigned)count << 16);
        acc[q] = rec;
        uint8_t r8, g8, b8;
        accum_resolve_px(rec, r8, g8, b8);
        uint8_t* o = out + q * 3;
        o[0] = r8;
        o[1] = g8;
        o[2] = b8;
      }
    }
    accum_count_saturated(saturated, sat);
  }
}
template <bool kCuda, bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_accum_list(
    Scene sc, Cam cam, int W, int lg, int count, PatWords pat, int maxrec,
    const uint32_t* __restrict__ list, const unsigned* __restrict__ nlist,
    uint2* __restrict__ acc, uint8_t* __restrict__ out, unsigned long long* __restrict__ zcount,
    unsigned* __restrict__ sat) {
  accum_listed<kCuda, kStage>(sc, cam, W, 0, 0, lg, count, pat, maxrec, list, nlist, acc, out,
                              zcount, sat);
}

// out = res(acc) for every pixel, nothing shot: 8 bytes in and 3 out a pixel, memory-bound.
__global__ void __launch_bounds__(256) k_accum_resolve(const uint2* __restrict__ acc,
                                                       unsigned long long pixels,
                                                       uint8_t* __restrict__ out) {
  const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (p >= pixels) return;
  uint8_t r8, g8, b8;
  accum_resolve_px(acc[p], r8, g8, b8);
  uint8_t* o = out + p * 3;
  o[0] = r8;
  o[1] = g8;
  o[2] = b8;
}

int accum_supported(int W, int H, int g, bool listed) {
  if (pattern_log2(g, 1, 3) < 0) return 0;
  if (W <= 0 || H <= 0 || W > (1 << 28) / g || H > (1 << 28) / g) return 0;   // g*W, g*H within int
  if (!listed) {   // k_render's tiles: grid.y, and xcd_tile's int tile index
    const unsigned long long tx = ((unsigned)W + kTileW - 1) / kTileW;
    const unsigned long long ty = ((unsigned)H + kTileH - 1) / kTileH;
    return ty <= 65535ull && tx * ty <= 0x7fffffffull;
  }
  if ((unsigned long long)W * (unsigned long long)H >= (1ull << 32)) return 0;   // uint32 entries
  const unsigned long long mx = ((unsigned long long)W + kMarkBlock - 1) / kMarkBlock;
  const unsigned long long my = ((unsigned long long)H + kMarkRows - 1) / kMarkRows;
  return mx * my <= 0x7fffffffull;   // k_aa_mark's grid
}

int accum_list_blocks(int W, int H, int cus, int want) { return list_blocks(W, H, 1, cus, want); }

hipError_t launch_accum(const LaunchScene& s, int W, int H, int g, int count, const uint8_t* px,
                        const uint8_t* py, bool reset, int maxrec, void* acc, uint8_t* out,
                        unsigned long long* zcount, unsigned* sat, hipStream_t stream,
                        bool cuda_sem) {
  if (!accum_supported(W, H, g, false) || count < 1 || count > 16) return hipErrorInvalidValue;
  const int lg = pattern_log2(g, 1, 3);
  dim3 grid((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH);
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, W * g, H * g);   // the camera of the g*W x g*H image
  const PatWords pat = pattern_words(count, px, py);
  dispatch(cuda_sem, stage_fits(s), [&](auto cuda, auto st) {
    hipLaunchKernelGGL((k_accum<cuda.value, st.value>), grid, dim3(kBlock), 0, stream, sc, cam, W,
                       H, lg, count, pat, reset ? 1 : 0, maxrec, (uint2*)acc, out, zcount, sat);
  });
  return hipGetLastError();
}

hipError_t launch_accum_list(const LaunchScene& s, int W, int H, int g, int count,
                             const uint8_t* px, const uint8_t* py, int maxrec,
                             const uint32_t* list, const unsigned* nlist, void* acc, uint8_t* out,
                             unsigned long long* zcount, unsigned* sat, int blocks,
                             hipStream_t stream, bool cuda_sem) {
  if (!accum_supported(W, H, g, true) || count < 1 || count > 16 || blocks < 1 || blocks > 4096)
    return hipErrorInvalidValue;
  const int lg = pattern_log2(g, 1, 3);
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, W * g, H * g);   // the camera of the g*W x g*H image
  const PatWords pat = pattern_words(count, px, py);
  dispatch(cuda_sem, stage_fits(s), [&](auto cuda, auto st) {
    hipLaunchKernelGGL((k_accum_list<cuda.value, st.value>), dim3((unsigned)blocks), dim3(kBlock),
                       0, stream, sc, cam, W, lg, count, pat, maxrec, list, nlist, (uint2*)acc,
                       out, zcount, sat);
  });
  return hipGetLastError();
}

hipError_t launch_accum_resolve(const void* acc, int W, int H, uint8_t* out, hipStream_t stream) {
  if (W <= 0 || H <= 0) return hipErrorInvalidValue;
  const unsigned long long pixels = (unsigned long long)W * (unsigned long long)H;
  const unsigned long long blocks = (pixels + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_accum_resolve, dim3((unsigned)blocks), dim3(256), 0, stream,
                     (const uint2*)acc, pixels, out);
  return hipGetLastError();
}

// ------------------------------------- windows of a virtual image (fast, cuda) --
// rc_render_window*, rc_accum_pass_window_device (include/raycast_hip.h, rc_window): the W x H
// output is the rectangle at (x0, y0) of the full_w x full_h image, so pixel (x, y) of the window
// is pixel (x0 + x, y0 + y) of that image and its subsamples are shot with the camera of the
// s*full_w x s*full_h image (`cam`) at the coordinates s*(x0 + x) + i, s*(y0 + y) + j: what
// k_render_ssaa, k_pattern and k_accum shoot for that pixel of the whole image.  Nothing of the
// arithmetic changes, only where in the picture the rays start.
//
// k_window: k_render_ssaa's tiles over the window's own subsample grid (s = 1 << ls in 1, 2, 4, 8;
// a workgroup owns 16 x 16 subsamples, a wave an 8 x 8 block of them), one lane per subsample.
// Inside a wave's block the s x s subsamples of an output pixel are s*s adjacent lanes (lane l:
// group l / (s*s), subsample l % (s*s) of it, row-major in both), so sample_reduce sums them and
// the group's first lane stores the rounded mean.  The origin (ox, oy) = (s*x0, s*y0) is whole
// pixels, so the groups stay aligned to the wave blocks whatever x0 and y0 are, and a group is
// wholly inside the window or wholly outside it.  At s = 1 a lane is a pixel and stores its own
// bytes.  The subsample image is never stored, in cuda mode either.
template <bool kCuda, bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_window(
    Scene sc, Cam cam, int W, int H, int ls, int ox, int oy, int maxrec, uint8_t* __restrict__ out,
    unsigned long long* __restrict__ zcount) {
  if (!kCuda && !RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  __shared__ StageBuf<kStage> stage;
  stage_scene<kStage>(sc, stage);
  int bx, by;
  xcd_tile<0>(bx, by);
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned sub = lane & ((1u << (2 * ls)) - 1u);   // subsample within the group
  const unsigned grp = lane >> (2 * ls);                  // group within the wave's 8 x 8 block
  const int lgw = 3 - ls;                                 // log2 of the groups in a row of it
  // unsigned: the last tile's columns may reach past 2^31 - 1 when s*W is close to it
  const unsigned xs = (unsigned)bx * kTileW + (wave % (kTileW / 8)) * 8u +
                      ((grp & ((1u << lgw) - 1u)) << ls) + (sub & ((1u << ls) - 1u));
  const unsigned rs = (unsigned)by * kTileH + (wave / (kTileW / 8)) * 8u + ((grp >> lgw) << ls) +
                      (sub >> ls);
  // only xs and rs stay live across shoot, as in k_render_ssaa
  const bool inside = (xs >> ls) < (unsigned)W && (rs >> ls) < (unsigned)H;
  unsigned rg = 0u, b = 0u;
  if (inside) sample_shoot<kCuda>(sc, cam, ox + (int)xs, oy + (int)rs, maxrec, zcount, rg, b);
  sample_reduce(rg, b, 2 * ls);
  if (inside && sub == 0u) {   // the group's first lane
    uint8_t* q = out + ((size_t)(rs >> ls) * W + (xs >> ls)) * 3;
    if (ls == 0) {   // one sample: its own bytes (sample_store's half is for two samples and more)
      q[0] = (uint8_t)(rg & 0xffffu);
      q[1] = (uint8_t)(rg >> 16);
      q[2] = (uint8_t)b;
    } else {
      sample_store(q, rg, b, 2 * ls);
    }
  }
}

// The accumulation passes through a window: accum_dense's and accum_listed's bodies with the
// window's origin; the records and the image are the window's own W x H.
template <bool kCuda, bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_accum_win(
    Scene sc, Cam cam, int W, int H, int ox, int oy, int lg, int count, PatWords pat, int reset,
    int maxrec, uint2* __restrict__ acc, uint8_t* __restrict__ out,
    unsigned long long* __restrict__ zcount, unsigned* __restrict__ sat) {
  accum_dense<kCuda, kStage>(sc, cam, W, H, ox, oy, lg, count, pat, reset, maxrec, acc, out,
                             zcount, sat);
}
template <bool kCuda, bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_accum_list_win(
    Scene sc, Cam cam, int W, int ox, int oy, int lg, int count, PatWords pat, int maxrec,
    const uint32_t* __restrict__ list, const unsigned* __restrict__ nlist,
    uint2* __restrict__ acc, uint8_t* __restrict__ out, unsigned long long* __restrict__ zcount,
    unsigned* __restrict__ sat) {
  accum_listed<kCuda, kStage>(sc, cam, W, ox, oy, lg, count, pat, maxrec, list, nlist, acc, out,
                              zcount, sat);
}

// the window lies inside the virtual image and s times that image's sides fit an int
static bool window_inside(const Window& w, int W, int H, int s) {
  return W >= 1 && H >= 1 && w.full_w >= 1 && w.full_h >= 1 && w.x0 >= 0 && w.y0 >= 0 &&
         W <= w.full_w - w.x0 && H <= w.full_h - w.y0 && w.full_w <= 0x7fffffff / s &&
         w.full_h <= 0x7fffffff / s;
}

int window_supported(const Window& w, int W, int H, int s) {
  if ((s != 1 && ssaa_log2(s) < 0) || !window_inside(w, W, H, s)) return 0;
  // k_render's tiles over the window's subsamples: grid.y, and xcd_tile's int tile index
  const unsigned long long tx = ((unsigned long long)W * s + kTileW - 1) / kTileW;
  const unsigned long long ty = ((unsigned long long)H * s + kTileH - 1) / kTileH;
  return ty <= 65535ull && tx * ty <= 0x7fffffffull;
}

hipError_t launch_window(const LaunchScene& s, const Window& w, int W, int H, int ssaa, int maxrec,
                         uint8_t* out, unsigned long long* zcount, hipStream_t stream,
                         bool cuda_sem) {
  if (!window_supported(w, W, H, ssaa)) return hipErrorInvalidValue;
  const int ls = ssaa == 1 ? 0 : ssaa_log2(ssaa);
  dim3 grid((unsigned)(((unsigned long long)W * ssaa + kTileW - 1) / kTileW),
            (unsigned)(((unsigned long long)H * ssaa + kTileH - 1) / kTileH));
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, w.full_w * ssaa, w.full_h * ssaa);   // of the s*full_w x s*full_h image
  dispatch(cuda_sem, stage_fits(s), [&](auto cuda, auto st) {
    hipLaunchKernelGGL((k_window<cuda.value, st.value>), grid, dim3(kBlock), 0, stream, sc, cam, W,
                       H, ls, w.x0 * ssaa, w.y0 * ssaa, maxrec, out, zcount);
  });
  return hipGetLastError();
}

hipError_t launch_accum_window(const LaunchScene& s, const Window& w, int W, int H, int g,
                               int count, const uint8_t* px, const uint8_t* py, bool reset,
                               int maxrec, void* acc, uint8_t* out, unsigned long long* zcount,
                               unsigned* sat, hipStream_t stream, bool cuda_sem) {
  if (!accum_supported(W, H, g, false) || !window_inside(w, W, H, g) || count < 1 || count > 16)
    return hipErrorInvalidValue;
  const int lg = pattern_log2(g, 1, 3);
  dim3 grid((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH);
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, w.full_w * g, w.full_h * g);   // of the g*full_w x g*full_h image
  const PatWords pat = pattern_words(count, px, py);
  dispatch(cuda_sem, stage_fits(s), [&](auto cuda, auto st) {
    hipLaunchKernelGGL((k_accum_win<cuda.value, st.value>), grid, dim3(kBlock), 0, stream, sc, cam,
                       W, H, w.x0, w.y0, lg, count, pat, reset ? 1 : 0, maxrec, (uint2*)acc, out,
                       zcount, sat);
  });
  return hipGetLastError();
}

hipError_t launch_accum_list_window(const LaunchScene& s, const Window& w, int W, int H, int g,
                                    int count, const uint8_t* px, const uint8_t* py, int maxrec,
                                    const uint32_t* list, const unsigned* nlist, void* acc,
                                    uint8_t* out, unsigned long long* zcount, unsigned* sat,
                                    int blocks, hipStream_t stream, bool cuda_sem) {
  if (!accum_supported(W, H, g, true) || !window_inside(w, W, H, g) || count < 1 || count > 16 ||
      blocks < 1 || blocks > 4096)
    return hipErrorInvalidValue;
  const int lg = pattern_log2(g, 1, 3);
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, w.full_w * g, w.full_h * g);   // of the g*full_w x g*full_h image
  const PatWords pat = pattern_words(count, px, py);
  dispatch(cuda_sem, stage_fits(s), [&](auto cuda, auto st) {
    hipLaunchKernelGGL((k_accum_list_win<cuda.value, st.value>), dim3((unsigned)blocks),
                       dim3(kBlock), 0, stream, sc, cam, W, w.x0, w.y0, lg, count, pat, maxrec,
                       list, nlist, (uint2*)acc, out, zcount, sat);
  });
  return hipGetLastError();
}

// ------------------------------------ scrolling an accumulated view (fast, cuda) --
// rc_accum_scroll_device (include/raycast_hip.h): the destination state is the source state moved
// by (-dx, -dy) where the two windows overlap (the kept rectangle K, scroll_rects) and freshly
// accumulated where the pan exposed new pixels.  Two kernels, behind every other kernel of the
// file as section 16's and 17's were.
//
// k_accum_move: the kept rectangle, one lane a pixel, adjacent lanes adjacent pixels of a row: one
// 8-byte load and one 8-byte store of the record and three bytes of the image.  grid.x covers a
// row of K in 256-pixel pieces, grid.y strides over its rows; every offset is a 64-bit pixel
// index.  (kx, ky): K's corner in the destination, (sx, sy) = (kx + dx, ky + dy) in the source.
__global__ void __launch_bounds__(256) k_accum_move(
    const uint2* __restrict__ acc_src, const uint8_t* __restrict__ out_src,
    uint2* __restrict__ acc_dst, uint8_t* __restrict__ out_dst, int W, int kw, int kh, int kx,
    int ky, int sx, int sy) {
  const unsigned x = blockIdx.x * 256u + threadIdx.x;
  if (x >= (unsigned)kw) return;
  for (unsigned y = blockIdx.y; y < (unsigned)kh; y += gridDim.y) {
    const size_t s = (size_t)((unsigned)sy + y) * (unsigned)W + ((unsigned)sx + x);
    const size_t d = (size_t)((unsigned)ky + y) * (unsigned)W + ((unsigned)kx + x);
    acc_dst[d] = acc_src[s];
    const uint8_t* q = out_src + s * 3;
    uint8_t* o = out_dst + d * 3;
    const uint8_t r8 = q[0], g8 = q[1], b8 = q[2];
    o[0] = r8;
    o[1] = g8;
    o[2] = b8;
  }
}

// Pixel e of the exposed set, e < r.total: the rectangle is found by comparing e with the
// rectangles' first entries (an empty rectangle shares its first entry with the next one, so it is
// never the last one at or below e), then one unsigned divide by that rectangle's width.
__device__ __forceinline__ void exposed_pixel(const ScrollRects& r, unsigned e, int& x, int& y) {
  unsigned first = r.first[0], w = r.w[0];
  int x0 = r.x[0], y0 = r.y[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const bool here = e >= r.first[k];
    first = here ? r.first[k] : first;
    w = here ? r.w[k] : w;
    x0 = here ? r.x[k] : x0;
    y0 = here ? r.y[k] : y0;
  }
  const unsigned i = e - first, row = i / w;
  x = x0 + (int)(i - row * w);
  y = y0 + (int)row;
}

// k_accum_exposed: accum_listed's body over the exposed set instead of a list: a fixed number of
// workgroups whose waves stride over [0, r.total) with a 64-bit index, one lane per exposed pixel,
// so a strip three pixels wide fills whole waves.  `reset` (the call's first chunk): the record is
// not read and counts as zero, as in accum_dense; a later chunk adds to the record the chunk
// before it stored.  No saturation: a scroll takes at most 64 samples.  The pixel is derived
// again from the entry after the samples (opaque lane, as accum_listed reads its list entry
// again) rather than carried across sample_shoot.  (ox, oy): as accum_dense's.
template <bool kCuda, bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_accum_exposed(
    Scene sc, Cam cam, int W, ScrollRects r, int ox, int oy, int lg, int count, PatWords pat,
    int reset, int maxrec, uint2* __restrict__ acc, uint8_t* __restrict__ out,
    unsigned long long* __restrict__ zcount) {
  if (!kCuda && !RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  __shared__ StageBuf<kStage> stage;
  stage_scene<kStage>(sc, stage);   // its barrier comes before the loop: every thread is here
  const int lane = threadIdx.x & 63;
  // wave-uniform by construction: told to the compiler, so the loop's counters stay scalar
  const unsigned wave =
      __builtin_amdgcn_readfirstlane(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));
  const unsigned step = gridDim.x * (kBlock / 64) * 64u;   // <= 4096 * 4 * 64
  const unsigned n = r.total;
  // 64-bit index: n + step may pass 2^32
  for (unsigned long long first = (unsigned long long)wave * 64u; first < n; first += step) {
    if (first + (unsigned)lane >= n) continue;
    int x, y;
    exposed_pixel(r, (unsigned)first + (unsigned)lane, x, y);
    const int xs = (int)(((unsigned)x + (unsigned)ox) << lg);
    const int ys = (int)(((unsigned)y + (unsigned)oy) << lg);
    unsigned rg = 0u, b = 0u;
    for (int k = 0; k < count; ++k) {   // uniform
      unsigned srg, sb;
      sample_shoot<kCuda>(sc, cam, xs + pat_entry(pat.x, (unsigned)k),
                          ys + pat_entry(pat.y, (unsigned)k), maxrec, zcount, srg, sb);
      rg += srg;
      b += sb;
    }
    unsigned l = (unsigned)lane;
    asm volatile("" : "+v"(l));
    exposed_pixel(r, (unsigned)first + l, x, y);
    const size_t q = (size_t)(unsigned)y * (unsigned)W + (unsigned)x;
    uint2 rec = make_uint2(0u, 0u);
    if (!reset) rec = acc[q];
    rec.x += rg;
    rec.y += b + ((unsigned)count << 16);
    acc[q] = rec;
    uint8_t r8, g8, b8;
    accum_resolve_px(rec, r8, g8, b8);
    uint8_t* o = out + q * 3;
    o[0] = r8;
    o[1] = g8;
    o[2] = b8;
  }
}

ScrollRects scroll_rects(int W, int H, int dx, int dy) {
  ScrollRects r = {};
  if (W < 1 || H < 1 || (unsigned long long)W * (unsigned long long)H >= (1ull << 32)) return r;
  // 64 bits: -INT_MIN does not occur
  const long long ax = dx < 0 ? -(long long)dx : dx, ay = dy < 0 ? -(long long)dy : dy;
  if (ax < W && ay < H) {
    r.kw = W - (int)ax, r.kh = H - (int)ay;
    r.kx = dx < 0 ? (int)ax : 0, r.ky = dy < 0 ? (int)ay : 0;
  }   // else nothing is kept: K is empty at (0, 0), and the rows below it are the whole window
  const int right = r.kx + r.kw;
  const unsigned wd[4] = {(unsigned)W, (unsigned)r.kx, (unsigned)(W - right), (unsigned)W};
  const unsigned ht[4] = {(unsigned)r.ky, (unsigned)r.kh, (unsigned)r.kh,
                          (unsigned)(H - r.ky - r.kh)};
  const int xs[4] = {0, 0, right, 0}, ys[4] = {0, r.ky, r.ky, r.ky + r.kh};
  for (int k = 0; k < 4; ++k) {
    r.first[k] = r.total;
    r.w[k] = wd[k] ? wd[k] : 1u;   // an empty rectangle is never divided by
    r.x[k] = xs[k], r.y[k] = ys[k];
    r.total += wd[k] * ht[k];      // the four are disjoint parts of W*H < 2^32
  }
  return r;
}

int accum_exposed_blocks(unsigned exposed, int cus, int want) {
  if (want > 0) return want;
  const unsigned need = exposed / kBlock + (exposed % kBlock ? 1u : 0u);   // as list_blocks
  const unsigned cap = (unsigned)(cus > 0 ? cus : 256) * RC_PHASE_A_WAVES;
  if (need <= cap) return (int)need;   // one step a wave: nothing strides
  // The entries of a rectangle are row-major, so a static stride that is a multiple of its width
  // keeps a wave in one column of the window and the waves whose column crosses the expensive
  // shapes finish last; an odd number of workgroups makes the stride drift through the columns
  // (the rate map's lists: DESIGN.md section 12; here: section 18).
  return (int)(cap > 2u && (cap & 1u) == 0u ? cap - 1u : cap);
}

hipError_t launch_accum_move(int W, int H, int g, int dx, int dy, const void* acc_src,
                             const uint8_t* out_src, void* acc_dst, uint8_t* out_dst,
                             hipStream_t stream) {
  const ScrollRects r = scroll_rects(W, H, dx, dy);
  if (!accum_supported(W, H, g, true) || r.kw < 1 || r.kh < 1) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(r.kw + 255) / 256u, (unsigned)(r.kh < 65535 ? r.kh : 65535));
  hipLaunchKernelGGL(k_accum_move, grid, dim3(256), 0, stream, (const uint2*)acc_src, out_src,
                     (uint2*)acc_dst, out_dst, W, r.kw, r.kh, r.kx, r.ky, r.kx + dx, r.ky + dy);
  return hipGetLastError();
}

hipError_t launch_accum_exposed(const LaunchScene& s, const Window& w, int W, int H, int g,
                                int dx, int dy, int count, const uint8_t* px, const uint8_t* py,
                                bool reset, int maxrec, void* acc, uint8_t* out,
                                unsigned long long* zcount, int blocks, hipStream_t stream,
                                bool cuda_sem) {
  if (!accum_supported(W, H, g, true) || !window_inside(w, W, H, g) || count < 1 || count > 16 ||
      blocks < 1 || blocks > 4096)
    return hipErrorInvalidValue;
  const ScrollRects r = scroll_rects(W, H, dx, dy);
  if (r.total == 0u) return hipErrorInvalidValue;
  const int lg = pattern_log2(g, 1, 3);
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, w.full_w * g, w.full_h * g);   // of the g*full_w x g*full_h image
  const PatWords pat = pattern_words(count, px, py);
  dispatch(cuda_sem, stage_fits(s), [&](auto cuda, auto st) {
    hipLaunchKernelGGL((k_accum_exposed<cuda.value, st.value>), dim3((unsigned)blocks),
                       dim3(kBlock), 0, stream, sc, cam, W, r, w.x0, w.y0, lg, count, pat,
                       reset ? 1 : 0, maxrec, (uint2*)acc, out, zcount);
  });
  return hipGetLastError();
}

// --------------------- the primary-visibility G-buffer (fast, parity, cuda) --
// rc_render_gbuffer*, rc_pick* (include/raycast_hip.h, rc_gbuffer): what the pixel kernels know
// about a pixel's primary hit before they shade it.  No new arithmetic: the direction is
// primary_dir's (cuda: render_pixel's first lines), the scan nearest_primary's (cu_nearest's), the
// frame hit_frame's, the routines tests/test_gpu_prims.py and tests/test_gpu_shading.py pin ray by
// ray.  shade, shoot and the bounce loop are not instantiated: without kFrame a pixel costs the
// scan alone.  The primary hit does not involve the scan-order carry, so parity mode's planes are
// fast mode's.  A miss leaves id = -1 and +0 everywhere else.  The events of the C port's
// normalisations go to `zero` (the direction's, with kFrame the normal's); the CUDA port counts
// none, as in every cuda kernel.
template <bool kCuda, bool kFrame>
__device__ __forceinline__ void gbuf_pixel(const Scene& sc, const Cam& cam, int X, int Y, int& id,
                                           float& t, V3& P, V3& N, int& zero) {
  static_assert(!(kCuda && kFrame), "no reference pins the CUDA port's hit frame");
  V3 d;
  if constexpr (kCuda) {
    d.x = (float)(cam.hx + (double)cam.pw * ((double)X + 0.5));
    d.y = (float)(cam.hy - (double)cam.ph * ((double)Y + 0.5));
    d.z = -1.0f;
    d = cusem::cu_normalize(d);
    id = cusem::cu_nearest(sc, v3(0.0f, 0.0f, 0.0f), d, -1, t);
  } else {
    d = primary_dir(cam, X, Y, zero);
    id = nearest_primary(sc, d, t);
  }
  P = N = v3(0.0f, 0.0f, 0.0f);
  if (id < 0) {
    t = 0.0f;
    return;
  }
  if constexpr (kFrame) hit_frame(sc, id, v3(0.0f, 0.0f, 0.0f), d, t, P, N, zero);
}

// The planes' device pointers, null: the plane is not wanted (a kernel argument, so the tests
// below are wave-uniform and a null plane costs nothing).
struct GbufPlanes {
  int32_t* id;
  float* t;
  float* P;
  float* N;
};

// k_gbuffer: k_window's grid at s = 1 (a workgroup owns 16 x 16 pixels, a wave an 8 x 8 block),
// one lane per pixel of the W x H window whose origin in the virtual image is (ox, oy).  The
// stores are the straightforward ones: a dword per lane for id and t (eight 32-byte runs a wave),
// three dwords at a 12-byte stride for P and N (eight 96-byte runs).  kStage (the divergent record
// reads of hit_frame from LDS) goes with kFrame only: the scan reads the records uniformly.
template <bool kCuda, bool kFrame, bool kStage>
__global__ void __launch_bounds__(kBlock) k_gbuffer(Scene sc, Cam cam, int W, int H, int ox,
                                                    int oy, GbufPlanes g,
                                                    unsigned long long* __restrict__ zcount) {
  static_assert(kFrame || !kStage, "the staged scene serves hit_frame");
  if (!kCuda && !RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  __shared__ StageBuf<kStage> stage;
  stage_scene<kStage>(sc, stage);
  int lx, ly;
  tile_pixel(lx, ly);
  int bx, by;
  xcd_tile<0>(bx, by);
  // unsigned: k_window's reasoning for the last tile's columns
  const unsigned x = (unsigned)bx * kTileW + (unsigned)lx, y = (unsigned)by * kTileH + (unsigned)ly;
  if (x >= (unsigned)W || y >= (unsigned)H) return;
  int id, zero = 0;
  float t;
  V3 P, N;
  gbuf_pixel<kCuda, kFrame>(sc, cam, ox + (int)x, oy + (int)y, id, t, P, N, zero);
  const size_t i = (size_t)y * (size_t)W + x;
  if (g.id) g.id[i] = id;
  if (g.t) g.t[i] = t;
  if constexpr (kFrame) {
    if (g.P) {
      float* q = g.P + 3 * i;
      q[0] = P.x, q[1] = P.y, q[2] = P.z;
    }
    if (g.N) {
      float* q = g.N + 3 * i;
      q[0] = N.x, q[1] = N.y, q[2] = N.z;
    }
  }
  if (!kCuda) flush_events(zero, zcount);
}

// k_gbuffer_points: one lane per point of rc_pick*: the lane reads its (X, Y) pair and stores its
// 32-byte rc_hit as two 16-byte vector stores (hits is 16-byte aligned).  A point outside the
// full_w x full_h image shoots no ray: id = -2, everything else +0.  The points are scattered, so
// the scene is not staged.
template <bool kCuda, bool kFrame>
__global__ void __launch_bounds__(256) k_gbuffer_points(Scene sc, Cam cam, int full_w, int full_h,
                                                        unsigned n, const int2* __restrict__ xy,
                                                        float4* __restrict__ hits,
                                                        unsigned long long* __restrict__ zcount) {
  if (!kCuda && !RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;
  const unsigned k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const int2 p = xy[k];
  int id = -2, zero = 0;
  float t = 0.0f;
  V3 P = v3(0.0f, 0.0f, 0.0f), N = P;
  if (p.x >= 0 && p.x < full_w && p.y >= 0 && p.y < full_h)
    gbuf_pixel<kCuda, kFrame>(sc, cam, p.x, p.y, id, t, P, N, zero);
  hits[2 * (size_t)k] = make_float4(__int_as_float(id), t, P.x, P.y);
  hits[2 * (size_t)k + 1] = make_float4(P.z, N.x, N.y, N.z);
  if (!kCuda) flush_events(zero, zcount);
}

// k_id_edge_rates: rates[y][x] = s where a pixel of the 3 x 3 neighbourhood, clipped to the image,
// has another id than id[y][x], else base.  One lane per pixel in row-major order, nine clipped
// loads (a wave's three rows of them are three runs of at most 66 dwords, served by the caches: the
// kernel reads each id once from memory), one byte out.  pixels = W * H < 2^32.
__global__ void __launch_bounds__(256) k_id_edge_rates(const int32_t* __restrict__ id, unsigned W,
                                                       unsigned H, unsigned pixels, uint8_t s,
                                                       uint8_t base, uint8_t* __restrict__ rates) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= pixels) return;
  const unsigned y = i / W, x = i - y * W;
  const unsigned x0 = x > 0u ? x - 1u : 0u, x1 = x + 1u < W ? x + 1u : x;
  const unsigned y0 = y > 0u ? y - 1u : 0u, y1 = y + 1u < H ? y + 1u : y;
  const int32_t me = id[i];
  bool edge = false;
  for (unsigned yy = y0; yy <= y1; ++yy) {
    const int32_t* row = id + (size_t)yy * W;
    for (unsigned xx = x0; xx <= x1; ++xx) edge = edge || row[xx] != me;
  }
  rates[i] = edge ? s : base;
}

// the pick image: both sides at least 1 (any size up to int: no grid is laid over it)
static bool pick_image(int full_w, int full_h) { return full_w >= 1 && full_h >= 1; }

hipError_t launch_gbuffer(const LaunchScene& s, const Window& w, int W, int H, int32_t* id,
                          float* t, float* P, float* N, unsigned long long* zcount,
                          hipStream_t stream, bool cuda_sem) {
  const bool frame = P || N;
  if (!window_supported(w, W, H, 1) || (!id && !t && !frame) || (cuda_sem && frame))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH));
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, w.full_w, w.full_h);
  const GbufPlanes g{id, t, P, N};
  if (cuda_sem) {
    hipLaunchKernelGGL((k_gbuffer<true, false, false>), grid, dim3(kBlock), 0, stream, sc, cam, W,
                       H, w.x0, w.y0, g, zcount);
  } else if (!frame) {
    hipLaunchKernelGGL((k_gbuffer<false, false, false>), grid, dim3(kBlock), 0, stream, sc, cam, W,
                       H, w.x0, w.y0, g, zcount);
  } else {
    dispatch(stage_fits(s), [&](auto st) {
      hipLaunchKernelGGL((k_gbuffer<false, true, st.value>), grid, dim3(kBlock), 0, stream, sc,
                         cam, W, H, w.x0, w.y0, g, zcount);
    });
  }
  return hipGetLastError();
}

hipError_t launch_gbuffer_points(const LaunchScene& s, int full_w, int full_h, bool frame,
                                 long long n, const int32_t* xy, void* hits,
                                 unsigned long long* zcount, hipStream_t stream, bool cuda_sem) {
  if (!pick_image(full_w, full_h) || n < 1 || n > (1ll << 24) || !xy || !hits ||
      ((uintptr_t)hits & 15u) || (cuda_sem && frame))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + 255) / 256));
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, full_w, full_h);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, sc, cam, full_w, full_h, (unsigned)n,
                       (const int2*)xy, (float4*)hits, zcount);
  };
  if (cuda_sem) go(k_gbuffer_points<true, false>);
  else if (frame) go(k_gbuffer_points<false, true>);
  else go(k_gbuffer_points<false, false>);
  return hipGetLastError();
}

int id_edge_rates_supported(int W, int H, int s, int base) {
  return (s == 2 || s == 4 || s == 8) && (base == 0 || base == 1) && W >= 1 && H >= 1 &&
         (unsigned long long)W * (unsigned long long)H < (1ull << 32);
}

hipError_t launch_id_edge_rates(const int32_t* id, int W, int H, int s, int base, uint8_t* rates,
                                hipStream_t stream) {
  if (!id || !rates || !id_edge_rates_supported(W, H, s, base)) return hipErrorInvalidValue;
  const unsigned long long pixels = (unsigned long long)W * (unsigned long long)H;
  hipLaunchKernelGGL(k_id_edge_rates, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, stream,
                     id, (unsigned)W, (unsigned)H, (unsigned)pixels, (uint8_t)s, (uint8_t)base,
                     rates);
  return hipGetLastError();
}

// ------------------- rotated camera views and ray batches (fast, cuda) --
// rc_render_view*, rc_trace_rays* (include/raycast_hip.h, rc_view): rays from the origin whose
// directions are not the pinhole grid's.  No new intersection or shading arithmetic: a direction
// goes through shoot<kModeFast> (cuda: cusem::shoot_dir, render_pixel's loop) and through
// nearest_primary / hit_frame (cu_nearest) exactly as a primary ray does.
//
// view_dir: primary_dir with the view matrix between the unnormalised vector p = (px, py, -1) and
// the one normalisation: q_i = dot(row_i, p) (two products and two sums, each rounded once), then
// the mode's own normalize of q.  v is a kernel argument, so its nine floats are scalar registers
// and the nine products take them as scalar operands.
template <bool kCuda>
__device__ __forceinline__ V3 view_dir(const Cam& cam, const View& v, int x, int y,
                                       int& zero_events) {
  V3 p;
  p.x = (float)(cam.hx + (double)cam.pw * ((double)x + 0.5));
  p.y = (float)(cam.hy - (double)cam.ph * ((double)y + 0.5));
  p.z = -1.0f;
  const V3 q = v3(dot(v3(v.m[0], v.m[1], v.m[2]), p), dot(v3(v.m[3], v.m[4], v.m[5]), p),
                  dot(v3(v.m[6], v.m[7], v.m[8]), p));
  if constexpr (kCuda) return cusem::cu_normalize(q);
  else return normalize(q, zero_events);
}

// The colour of the ray from the origin along d, used as given: the mode's bounce loop
// (sample_shoot's two branches behind their directions).
template <bool kCuda>
__device__ __forceinline__ V3 dir_shoot(const Scene& sc, V3 d, int maxrec, int& zero_events) {
  if constexpr (kCuda) {
    return cusem::shoot_dir(sc, d, maxrec - 1);
  } else {
    PixelOut po;
    shoot<kModeFast>(sc, d, maxrec, v3(0.0f, 0.0f, 0.0f), po, zero_events);
    return po.rgb;
  }
}

// k_view: k_window (its grid, lane layout, bounds test, reduction and stores, line for line) with
// view_dir in primary_dir's place.  A kernel of its own: k_window sits at the 128-register edge
// and must not move.
template <bool kCuda, bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_view(
    Scene sc, Cam cam, View v, int W, int H, int ls, int ox, int oy, int maxrec,
    uint8_t* __restrict__ out, unsigned long long* __restrict__ zcount) {
  if (!kCuda && !RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  __shared__ StageBuf<kStage> stage;
  stage_scene<kStage>(sc, stage);
  int bx, by;
  xcd_tile<0>(bx, by);
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned sub = lane & ((1u << (2 * ls)) - 1u);
  const unsigned grp = lane >> (2 * ls);
  const int lgw = 3 - ls;
  const unsigned xs = (unsigned)bx * kTileW + (wave % (kTileW / 8)) * 8u +
                      ((grp & ((1u << lgw) - 1u)) << ls) + (sub & ((1u << ls) - 1u));
  const unsigned rs = (unsigned)by * kTileH + (wave / (kTileW / 8)) * 8u + ((grp >> lgw) << ls) +
                      (sub >> ls);
  const bool inside = (xs >> ls) < (unsigned)W && (rs >> ls) < (unsigned)H;
  unsigned rg = 0u, b = 0u;
  if (inside) {
    int zero = 0;
    const V3 d = view_dir<kCuda>(cam, v, ox + (int)xs, oy + (int)rs, zero);
    const V3 c = dir_shoot<kCuda>(sc, d, maxrec, zero);
    rg = (unsigned)quant(c.x) | ((unsigned)quant(c.y) << 16);
    b = quant(c.z);
    if (!kCuda) flush_events(zero, zcount);
  }
  sample_reduce(rg, b, 2 * ls);
  if (inside && sub == 0u) {   // the group's first lane
    uint8_t* q = out + ((size_t)(rs >> ls) * W + (xs >> ls)) * 3;
    if (ls == 0) {
      q[0] = (uint8_t)(rg & 0xffffu);
      q[1] = (uint8_t)(rg >> 16);
      q[2] = (uint8_t)b;
    } else {
      sample_store(q, rg, b, 2 * ls);
    }
  }
}

// The outputs of a ray batch, null: not wanted (a kernel argument, so the tests are wave-uniform).
struct RayOut {
  uint8_t* rgb8;
  float* rgb;
  float4* hits;
};

// k_rays: one lane per direction of rc_trace_rays*, read as three dwords at a 12-byte stride and
// used as given.  The colour (when rgb or rgb8 is wanted) is dir_shoot's; the record (when hits is)
// is the primary hit's, gbuf_pixel's scan and frame for that direction, stored as
// k_gbuffer_points' two 16-byte stores.  The directions are arbitrary, so the scene is not staged.
template <bool kCuda, bool kFrame>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_rays(
    Scene sc, unsigned n, const float* __restrict__ dirs, int maxrec, RayOut o,
    unsigned long long* __restrict__ zcount) {
  static_assert(!(kCuda && kFrame), "no reference pins the CUDA port's hit frame");
  if (!kCuda && !RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;
  const unsigned k = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (k >= n) return;
  const float* p = dirs + 3 * (size_t)k;
  const V3 d = v3(p[0], p[1], p[2]);
  int zero = 0;
  // the record first: nothing of it stays live across the bounce loop, which then holds only k
  if (o.hits) {
    int id;
    float t;
    V3 P = v3(0.0f, 0.0f, 0.0f), N = P;
    if constexpr (kCuda) id = cusem::cu_nearest(sc, v3(0.0f, 0.0f, 0.0f), d, -1, t);
    else id = nearest_primary(sc, d, t);
    if (id < 0) t = 0.0f;
    if constexpr (kFrame)
      if (id >= 0) hit_frame(sc, id, v3(0.0f, 0.0f, 0.0f), d, t, P, N, zero);
    o.hits[2 * (size_t)k] = make_float4(__int_as_float(id), t, P.x, P.y);
    o.hits[2 * (size_t)k + 1] = make_float4(P.z, N.x, N.y, N.z);
  }
  if (o.rgb || o.rgb8) {
    const V3 c = dir_shoot<kCuda>(sc, d, maxrec, zero);
    if (o.rgb) {
      float* q = o.rgb + 3 * (size_t)k;
      q[0] = c.x, q[1] = c.y, q[2] = c.z;
    }
    if (o.rgb8) store_rgb(o.rgb8 + 3 * (size_t)k, c);
  }
  if (!kCuda) flush_events(zero, zcount);
}

hipError_t launch_view(const LaunchScene& s, const View& v, const Window& w, int W, int H,
                       int ssaa, int maxrec, uint8_t* out, unsigned long long* zcount,
                       hipStream_t stream, bool cuda_sem) {
  if (!window_supported(w, W, H, ssaa)) return hipErrorInvalidValue;
  const int ls = ssaa == 1 ? 0 : ssaa_log2(ssaa);
  dim3 grid((unsigned)(((unsigned long long)W * ssaa + kTileW - 1) / kTileW),
            (unsigned)(((unsigned long long)H * ssaa + kTileH - 1) / kTileH));
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, w.full_w * ssaa, w.full_h * ssaa);   // of the s*full_w x s*full_h image
  dispatch(cuda_sem, stage_fits(s), [&](auto cuda, auto st) {
    hipLaunchKernelGGL((k_view<cuda.value, st.value>), grid, dim3(kBlock), 0, stream, sc, cam, v,
                       W, H, ls, w.x0 * ssaa, w.y0 * ssaa, maxrec, out, zcount);
  });
  return hipGetLastError();
}

hipError_t launch_rays(const LaunchScene& s, long long n, const float* dirs, int maxrec,
                       uint8_t* rgb8, float* rgb, void* hits, bool frame,
                       unsigned long long* zcount, hipStream_t stream, bool cuda_sem) {
  if (n < 1 || n > (1ll << 24) || !dirs || (!rgb8 && !rgb && !hits) ||
      ((uintptr_t)hits & 15u) || (cuda_sem && frame && hits))   // frame says nothing without hits
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
  const Scene sc = make_scene(s);
  const RayOut o{rgb8, rgb, (float4*)hits};
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, stream, sc, (unsigned)n, dirs, maxrec, o,
                       zcount);
  };
  if (cuda_sem) go(k_rays<true, false>);
  else if (frame && hits) go(k_rays<false, true>);
  else go(k_rays<false, false>);
  return hipGetLastError();
}

// ------------------- a free camera and rays with origins (fast) --
// rc_render_camera*, rc_trace_rays_from* (include/raycast_hip.h, rc_camera): k_view and k_rays
// with an origin.  No new arithmetic: shoot_from (rc_device.hpp) is shoot<kModeFast> with the
// general nearest and hit_frame at the origin given.
//
// RC_CAMERA_TABLE 1: k_camera reads the eye's origin-only shape terms from a table in LDS
// (EyeShape, nearest_eye), built by every workgroup for itself; 0, the default: it calls the
// general nearest with O = eye.  Equal bytes either way (`make camera-variants` builds both;
// scripts/camera_ab.py checks each against k_view's and k_rays_from's bytes and measures them).
// Measured (profiles/camera_ab_quadric.txt): the table is 0.999-1.013 of
// the general form, inside the spreads of the repeats.  The terms it saves are a few scalar-fed
// operations a shape beside the f64 work of every test, and reading them back costs LDS loads
// in their place.  So the general form ships, and the table stays behind the switch.
#ifndef RC_CAMERA_TABLE
#define RC_CAMERA_TABLE 0
#endif

struct Eye {
  float x, y, z;
};

// k_camera: k_view (its grid, lane layout, bounds test, reduction and stores) in fast mode with
// the primary ray leaving the eye.  With RC_CAMERA_TABLE the table is the workgroup's own LDS,
// filled by one thread per shape in front of stage_scene's barrier: nothing is shared between two
// frames in flight.  A scene too large to stage (stage_fits) has no table either way and takes the
// general nearest.
template <bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_camera(
    Scene sc, Cam cam, View v, Eye e, int W, int H, int ls, int ox, int oy, int maxrec,
    uint8_t* __restrict__ out, unsigned long long* __restrict__ zcount) {
  constexpr bool kTable = kStage && RC_CAMERA_TABLE;
  if (!RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  const V3 eye = v3(e.x, e.y, e.z);
  __shared__ StageBuf<kStage> stage;
  __shared__ EyeShape eyes[kTable ? kStageShapes : 1];
  if constexpr (kTable)
    if ((int)threadIdx.x < sc.n) eyes[threadIdx.x] = eye_shape(sc.shapes[threadIdx.x], eye, quad_x0(sc));
  stage_scene<kStage>(sc, stage);   // its barrier publishes the table too
  int bx, by;
  xcd_tile<0>(bx, by);
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned sub = lane & ((1u << (2 * ls)) - 1u);
  const unsigned grp = lane >> (2 * ls);
  const int lgw = 3 - ls;
  const unsigned xs = (unsigned)bx * kTileW + (wave % (kTileW / 8)) * 8u +
                      ((grp & ((1u << lgw) - 1u)) << ls) + (sub & ((1u << ls) - 1u));
  const unsigned rs = (unsigned)by * kTileH + (wave / (kTileW / 8)) * 8u + ((grp >> lgw) << ls) +
                      (sub >> ls);
  const bool inside = (xs >> ls) < (unsigned)W && (rs >> ls) < (unsigned)H;
  unsigned rg = 0u, b = 0u;
  if (inside) {
    int zero = 0;
    const V3 d = view_dir<false>(cam, v, ox + (int)xs, oy + (int)rs, zero);
    float t0;
    int i0;
    if constexpr (kTable) i0 = nearest_eye(sc, eye, d, eyes, t0);
    else i0 = nearest(sc, eye, d, -1, t0);
    const V3 c = shoot_from(sc, eye, d, i0, t0, maxrec, zero);
    rg = (unsigned)quant(c.x) | ((unsigned)quant(c.y) << 16);
    b = quant(c.z);
    flush_events(zero, zcount);
  }
  sample_reduce(rg, b, 2 * ls);
  if (inside && sub == 0u) {   // the group's first lane
    uint8_t* q = out + ((size_t)(rs >> ls) * W + (xs >> ls)) * 3;
    if (ls == 0) {
      q[0] = (uint8_t)(rg & 0xffffu);
      q[1] = (uint8_t)(rg >> 16);
      q[2] = (uint8_t)b;
    } else {
      sample_store(q, rg, b, 2 * ls);
    }
  }
}

// k_rays_from: k_rays in fast mode with a second 12-byte-stride load, the ray's origin.  The
// record is nearest(O, d, skip = -1) and its frame at O; the colour is shoot_from's.  Origins are
// device data and are not looked at: a non-finite one fails every shape test, as in the oracle.
template <bool kFrame>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_rays_from(
    Scene sc, unsigned n, const float* __restrict__ origins, const float* __restrict__ dirs,
    int maxrec, RayOut o, unsigned long long* __restrict__ zcount) {
  if (!RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;
  const unsigned k = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (k >= n) return;
  const float* p = dirs + 3 * (size_t)k;
  const float* q0 = origins + 3 * (size_t)k;
  const V3 d = v3(p[0], p[1], p[2]);
  const V3 O = v3(q0[0], q0[1], q0[2]);
  int zero = 0, zrec = 0;   // zrec: the record's frame alone (shoot_from counts its own)
  float t;
  const int id = nearest(sc, O, d, -1, t);
  if (o.hits) {
    V3 P = v3(0.0f, 0.0f, 0.0f), N = P;
    if constexpr (kFrame)
      if (id >= 0) hit_frame(sc, id, O, d, t, P, N, zrec);
    o.hits[2 * (size_t)k] = make_float4(__int_as_float(id), id < 0 ? 0.0f : t, P.x, P.y);
    o.hits[2 * (size_t)k + 1] = make_float4(P.z, N.x, N.y, N.z);
  }
  if (!o.rgb && !o.rgb8) zero = zrec;
  if (o.rgb || o.rgb8) {
    const V3 c = shoot_from(sc, O, d, id, t, maxrec, zero);
    if (o.rgb) {
      float* q = o.rgb + 3 * (size_t)k;
      q[0] = c.x, q[1] = c.y, q[2] = c.z;
    }
    if (o.rgb8) store_rgb(o.rgb8 + 3 * (size_t)k, c);
  }
  flush_events(zero, zcount);
}

hipError_t launch_camera(const LaunchScene& s, const float eye[3], const View& v, const Window& w,
                         int W, int H, int ssaa, int maxrec, uint8_t* out,
                         unsigned long long* zcount, hipStream_t stream) {
  uint32_t bits[3];
  std::memcpy(bits, eye, sizeof bits);
  if ((bits[0] | bits[1] | bits[2]) == 0u)   // the eye at +0: a view (k_view's primary forms)
    return launch_view(s, v, w, W, H, ssaa, maxrec, out, zcount, stream, false);
  if (!window_supported(w, W, H, ssaa)) return hipErrorInvalidValue;
  const int ls = ssaa == 1 ? 0 : ssaa_log2(ssaa);
  dim3 grid((unsigned)(((unsigned long long)W * ssaa + kTileW - 1) / kTileW),
            (unsigned)(((unsigned long long)H * ssaa + kTileH - 1) / kTileH));
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, w.full_w * ssaa, w.full_h * ssaa);   // of the s*full_w x s*full_h image
  const Eye e{eye[0], eye[1], eye[2]};
  dispatch(stage_fits(s), [&](auto st) {
    hipLaunchKernelGGL((k_camera<st.value>), grid, dim3(kBlock), 0, stream, sc, cam, v, e, W, H, ls,
                       w.x0 * ssaa, w.y0 * ssaa, maxrec, out, zcount);
  });
  return hipGetLastError();
}

hipError_t launch_rays_from(const LaunchScene& s, long long n, const float* origins,
                            const float* dirs, int maxrec, uint8_t* rgb8, float* rgb, void* hits,
                            bool frame, unsigned long long* zcount, hipStream_t stream) {
  if (n < 1 || n > (1ll << 24) || !origins || !dirs || (!rgb8 && !rgb && !hits) ||
      ((uintptr_t)hits & 15u))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
  const Scene sc = make_scene(s);
  const RayOut o{rgb8, rgb, (float4*)hits};
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, stream, sc, (unsigned)n, origins, dirs,
                       maxrec, o, zcount);
  };
  if (frame && hits) go(k_rays_from<true>);
  else go(k_rays_from<false>);
  return hipGetLastError();
}

// ------------------- accumulation through a free camera (fast) --
// rc_accum_pass_camera_device / rc_render_camera_accum (include/raycast_hip.h): accum_dense's and
// accum_listed's bodies with sample k shot k_camera's way through camera k of the pass: view_dir
// on the subsample's virtual coordinates, the general nearest from the eye, shoot_from and quant.
// Bodies of their own beside the old ones, so that k_accum*, k_accum_*win and k_accum_exposed keep
// their instructions.  No new arithmetic.
//
// The cameras are one kernel argument (CamSet, 768 bytes).  The sample loop is uniform, so k, the
// lattice entry and the camera are scalar: camera k is read from the argument segment with scalar
// loads at a scalar offset, never copied to scratch or chosen lane by lane.  A pass with one
// camera has that camera in every slot (the host fills them), so the loop has no branch for it.
// Nothing derived from a camera is stored anywhere: two passes in flight share nothing.
// An eye of +0 takes the general nearest like any other (bit-equal to the origin forms).
__device__ __forceinline__ void cam_sample_shoot(const Scene& sc, const Cam& cam,
                                                 const CamSet& cams, int k, int xs, int ys,
                                                 int maxrec,
                                                 unsigned long long* __restrict__ zcount,
                                                 unsigned& rg, unsigned& b) {
  int zero = 0;
  const V3 eye = v3(cams.eye[k][0], cams.eye[k][1], cams.eye[k][2]);
  const V3 d = view_dir<false>(cam, cams.view[k], xs, ys, zero);
  float t0;
  const int i0 = nearest(sc, eye, d, -1, t0);
  const V3 c = shoot_from(sc, eye, d, i0, t0, maxrec, zero);
  rg = (unsigned)quant(c.x) | ((unsigned)quant(c.y) << 16);
  b = quant(c.z);
  flush_events(zero, zcount);
}

// k_accum_cam: accum_dense line for line (its grid, tiles, the record's n read alone before the
// samples, one 8-byte load and one 8-byte store behind them, the image through the tile stores);
// across a sample only the two packed sums and what accum_dense keeps stay live.
template <bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_accum_cam(
    Scene sc, Cam cam, CamSet cams, int W, int H, int ox, int oy, int lg, int count, PatWords pat,
    int reset, int maxrec, uint2* __restrict__ acc, uint8_t* __restrict__ out,
    unsigned long long* __restrict__ zcount, unsigned* __restrict__ sat) {
  if (!RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  __shared__ StageBuf<kStage> stage;
  __shared__ TileBytes tb;
  tile_init(tb);
  stage_scene<kStage>(sc, stage);
  if (!kStage) __syncthreads();
  int lx, ly;
  tile_pixel(lx, ly);
  int bx, by;
  xcd_tile<0>(bx, by);
  const int x0 = bx * kTileW, y0 = by * kTileH;
  const int x = x0 + lx, y = y0 + ly;
  bool saturated = false;
  if (x < W && y < H) {
    const size_t p = (size_t)y * W + x;
    const unsigned had = reset ? 0u : (unsigned)((const uint16_t*)(acc + p))[3];
    saturated = had + (unsigned)count > 256u;
    if (!saturated) {
      unsigned rg = 0u, b = 0u;
      for (int k = 0; k < count; ++k) {   // uniform
        unsigned srg, sb;
        cam_sample_shoot(sc, cam, cams, k, ((ox + x) << lg) + pat_entry(pat.x, (unsigned)k),
                         ((oy + y) << lg) + pat_entry(pat.y, (unsigned)k), maxrec, zcount, srg,
                         sb);
        rg += srg;
        b += sb;
      }
      uint2 rec = make_uint2(0u, 0u);
      if (!reset) rec = acc[p];
      rec.x += rg;
      rec.y += b + ((unsigned)count << 16);
      acc[p] = rec;
      uint8_t r8, g8, b8;
      accum_resolve_px(rec, r8, g8, b8);
      tile_put_rgb(tb, lx, ly, r8, g8, b8, out + p * 3);
    } else if (RC_TILE_STAGE) {   // the staged tile's whole-row stores write this pixel too
      const uint8_t* q = out + p * 3;
      tile_put_rgb(tb, lx, ly, q[0], q[1], q[2], out + p * 3);
    }
  }
  accum_count_saturated(saturated, sat);
  if (!tile_last_wave(tb)) return;
  const int nx = W - x0 < kTileW ? W - x0 : kTileW;
  tile_write_rows<kTileW * 3 / 4>(tb.rgb, [&](int q) -> uint8_t* {
    return y0 + q < H ? out + ((size_t)(y0 + q) * W + x0) * 3 : nullptr;
  }, nx * 3);
}

// k_accum_list_cam: accum_listed line for line over k_aa_mark's list; the entry is read again
// behind the samples, as there.
template <bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_accum_list_cam(
    Scene sc, Cam cam, CamSet cams, int W, int ox, int oy, int lg, int count, PatWords pat,
    int maxrec, const uint32_t* __restrict__ list, const unsigned* __restrict__ nlist,
    uint2* __restrict__ acc, uint8_t* __restrict__ out, unsigned long long* __restrict__ zcount,
    unsigned* __restrict__ sat) {
  if (!RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  __shared__ StageBuf<kStage> stage;
  const unsigned n = *nlist;
  if (n == 0u) return;   // uniform over the grid: an empty list costs its launch
  stage_scene<kStage>(sc, stage);   // its barrier comes before the loop: every thread is here
  const int lane = threadIdx.x & 63;
  const unsigned wave =
      __builtin_amdgcn_readfirstlane(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));
  const unsigned step = gridDim.x * (kBlock / 64) * 64u;   // <= 4096 * 4 * 64
  // 64-bit index: n + step may pass 2^32
  for (unsigned long long first = (unsigned long long)wave * 64u; first < n; first += step) {
    const unsigned long long e = first + (unsigned)lane;
    bool saturated = false;
    if (e < n) {
      const unsigned p = list[e];
      saturated = (unsigned)((const uint16_t*)(acc + p))[3] + (unsigned)count > 256u;
      if (!saturated) {
        const int xs = (int)((p % (unsigned)W + (unsigned)ox) << lg);
        const int ys = (int)((p / (unsigned)W + (unsigned)oy) << lg);
        unsigned rg = 0u, b = 0u;
        for (int k = 0; k < count; ++k) {   // uniform
          unsigned srg, sb;
          cam_sample_shoot(sc, cam, cams, k, xs + pat_entry(pat.x, (unsigned)k),
                           ys + pat_entry(pat.y, (unsigned)k), maxrec, zcount, srg, sb);
          rg += srg;
          b += sb;
        }
        unsigned l = (unsigned)lane;   // opaque: the entry is read again, as in accum_listed
        asm volatile("" : "+v"(l));
        const size_t q = list[first + l];
        uint2 rec = acc[q];
        rec.x += rg;
        rec.y += b + ((unsigned)count << 16);
        acc[q] = rec;
        uint8_t r8, g8, b8;
        accum_resolve_px(rec, r8, g8, b8);
        uint8_t* o = out + q * 3;
        o[0] = r8;
        o[1] = g8;
        o[2] = b8;
      }
    }
    accum_count_saturated(saturated, sat);
  }
}

hipError_t launch_accum_cam(const LaunchScene& s, const CamSet& cams, const Window& w, int W,
                            int H, int g, int count, const uint8_t* px, const uint8_t* py,
                            bool reset, int maxrec, void* acc, uint8_t* out,
                            unsigned long long* zcount, unsigned* sat, hipStream_t stream) {
  if (!accum_supported(W, H, g, false) || !window_inside(w, W, H, g) || count < 1 || count > 16)
    return hipErrorInvalidValue;
  const int lg = pattern_log2(g, 1, 3);
  dim3 grid((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH);
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, w.full_w * g, w.full_h * g);   // of the g*full_w x g*full_h image
  const PatWords pat = pattern_words(count, px, py);
  dispatch(stage_fits(s), [&](auto st) {
    hipLaunchKernelGGL((k_accum_cam<st.value>), grid, dim3(kBlock), 0, stream, sc, cam, cams, W, H,
                       w.x0, w.y0, lg, count, pat, reset ? 1 : 0, maxrec, (uint2*)acc, out, zcount,
                       sat);
  });
  return hipGetLastError();
}

hipError_t launch_accum_list_cam(const LaunchScene& s, const CamSet& cams, const Window& w, int W,
                                 int H, int g, int count, const uint8_t* px, const uint8_t* py,
                                 int maxrec, const uint32_t* list, const unsigned* nlist,
                                 void* acc, uint8_t* out, unsigned long long* zcount,
                                 unsigned* sat, int blocks, hipStream_t stream) {
  if (!accum_supported(W, H, g, true) || !window_inside(w, W, H, g) || count < 1 || count > 16 ||
      blocks < 1 || blocks > 4096)
    return hipErrorInvalidValue;
  const int lg = pattern_log2(g, 1, 3);
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, w.full_w * g, w.full_h * g);   // of the g*full_w x g*full_h image
  const PatWords pat = pattern_words(count, px, py);
  dispatch(stage_fits(s), [&](auto st) {
    hipLaunchKernelGGL((k_accum_list_cam<st.value>), dim3((unsigned)blocks), dim3(kBlock), 0,
                       stream, sc, cam, cams, W, w.x0, w.y0, lg, count, pat, maxrec, list, nlist,
                       (uint2*)acc, out, zcount, sat);
  });
  return hipGetLastError();
}

// ------------------- any-hit visibility queries and ambient occlusion (fast) --
// rc_occluded_rays*, rc_ao_pass_device, rc_ao_resolve_device (include/raycast_hip.h, rc_ao_dirs):
// the shadow rays' question for rays that are not shade's own.  No new arithmetic: the primary hit
// is k_camera's (view_dir, the general nearest, hit_frame), the flip is the project's dot and a
// product with -1.0f, and a ray's answer is shadowed (tmax = +inf) or occluded (rc_device.hpp).
// No shade, shoot or bounce loop is instantiated.
//
// The record is one dword: open | rays << 16 (rc_ao_px's two uint16).
__device__ __forceinline__ unsigned ao_byte(unsigned rec) {
  const unsigned open = rec & 0xffffu, rays = rec >> 16;
  return rays ? (510u * open + rays) / (2u * rays) : 255u;   // 510 * 65535 < 2^25
}

// the sum of v over the wave, in every lane; called by every lane
__device__ __forceinline__ unsigned ao_wave_sum(unsigned v) {
  for (int m = 1; m < 64; m <<= 1) v += (unsigned)__shfl_xor((int)v, m, 64);
  return v;
}

// k_ao: k_camera's grid at ssaa = 1 with accum_dense's tiles, one lane a pixel.  The direction
// loop is the outer loop and its trip count and index are uniform: u_j and tmax are scalar loads
// from the argument segment (as k_accum_cam reads its cameras), the branch on tmax is uniform, and
// the lanes of a wave test one direction from neighbouring hit points, so shadowed's and occluded's
// early exits diverge little.  Per lane: the hit point, the normal, the skip index, the count.
// ray_consts stays inside shadowed and occluded: it depends on D only through its squares, which
// the flip does not change, but gfx950 has no scalar floating-point unit to hoist it into, and it
// is one evaluation a direction beside sc.n shape tests.
// stats: kAoStatSlots lines of {hit pixels, blocked rays, saturated pixels}; one atomic a wave and
// counter into the wave's line, none for a wave that has nothing to add (flush_events' manner);
// the host sums the lines.
template <bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_ao(
    Scene sc, Cam cam, View v, Eye e, AoDirs dirs, int W, int H, int ox, int oy, int reset,
    uint32_t* __restrict__ ao, uint8_t* __restrict__ out, unsigned long long* __restrict__ zcount,
    unsigned long long* __restrict__ stats) {
  if (!RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  const V3 eye = v3(e.x, e.y, e.z);
  __shared__ StageBuf<kStage> stage;
  __shared__ TileBytes tb;
  tile_init(tb);
  stage_scene<kStage>(sc, stage);
  if (!kStage) __syncthreads();
  int lx, ly;
  tile_pixel(lx, ly);
  int bx, by;
  xcd_tile<0>(bx, by);
  const int x0 = bx * kTileW, y0 = by * kTileH;
  const int x = x0 + lx, y = y0 + ly;
  const unsigned n = (unsigned)dirs.n;
  bool saturated = false, hit = false;
  unsigned blocked = 0u;
  if (x < W && y < H) {
    const size_t p = (size_t)y * W + x;
    unsigned rec = reset ? 0u : ao[p];
    saturated = (rec >> 16) + n > 65535u;
    if (!saturated) {
      int zero = 0;
      const V3 d = view_dir<false>(cam, v, ox + x, oy + y, zero);
      float t;
      const int id = nearest(sc, eye, d, -1, t);
      hit = id >= 0;
      V3 P = v3(0.0f, 0.0f, 0.0f), N = P;
      if (hit) hit_frame(sc, id, eye, d, t, P, N, zero);
      const bool bounded = dirs.tmax != __builtin_inff();   // uniform
      for (unsigned j = 0; j < n; ++j) {   // uniform
        const V3 u = v3(dirs.u[j][0], dirs.u[j][1], dirs.u[j][2]);
        if (hit) {
          const V3 D = dot(N, u) < 0.0f ? v3(u.x * -1.0f, u.y * -1.0f, u.z * -1.0f) : u;
          const bool b = bounded ? occluded(sc, P, D, id, dirs.tmax) : shadowed(sc, P, D, id);
          blocked += b ? 1u : 0u;
        }
      }
      rec += (n - blocked) + (n << 16);
      ao[p] = rec;
      flush_events(zero, zcount);
    }
    if (out) {   // uniform
      const uint8_t byte = (uint8_t)ao_byte(rec);
      if (RC_TILE_STAGE) ((uint8_t*)tb.cls[ly])[lx] = byte;
      else out[p] = byte;
    }
  }
  const unsigned hits = (unsigned)__popcll(__ballot(hit));
  const unsigned sats = (unsigned)__popcll(__ballot(saturated));
  const unsigned blk = ao_wave_sum(blocked);
  if ((threadIdx.x & 63) == 0) {
    // nearly every wave has hits to add, unlike flush_events' and accum_count_saturated's rare
    // ones: on one address the atomics of a 1024 x 1024 pass cost three times its rays (measured,
    // DESIGN.md section 27), so the waves are dealt over kAoStatSlots lines
    const unsigned w = (blockIdx.y * gridDim.x + blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    unsigned long long* s = stats + (size_t)(w & (kAoStatSlots - 1)) * kAoStatStride;
    if (hits) atomicAdd(s, (unsigned long long)hits);
    if (blk) atomicAdd(s + 1, (unsigned long long)blk);
    if (sats) atomicAdd(s + 2, (unsigned long long)sats);
  }
  if (!out || !tile_last_wave(tb)) return;
  const int nx = W - x0 < kTileW ? W - x0 : kTileW;
  tile_write_rows<kTileW / 4>(tb.cls, [&](int q) -> uint8_t* {
    return y0 + q < H ? out + (size_t)(y0 + q) * W + x0 : nullptr;
  }, nx);
}

// k_occluded_rays: k_rays_from's loads (two 12-byte strides) and the two optional per-ray words,
// one byte out a lane.  Nothing per ray is looked at: a NaN, zero or negative tmax takes occluded,
// which accepts nothing; a skip that names no shape skips nothing and switches the z rule on.  The
// branch on tmax is per lane.  No normalisation happens here, so there is no zero event to count.
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_occluded_rays(
    Scene sc, unsigned n, const float* __restrict__ origins, const float* __restrict__ dirs,
    const int* __restrict__ skip, const float* __restrict__ tmax, uint8_t* __restrict__ out) {
  if (!RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;
  const unsigned k = blockIdx.x * (unsigned)kBlock + threadIdx.x;
  if (k >= n) return;
  const float* p = dirs + 3 * (size_t)k;
  const float* q0 = origins + 3 * (size_t)k;
  const V3 D = v3(p[0], p[1], p[2]);
  const V3 O = v3(q0[0], q0[1], q0[2]);
  const int s = skip ? skip[k] : -1;
  const float tm = tmax ? tmax[k] : __builtin_inff();
  const bool b = tm == __builtin_inff() ? shadowed(sc, O, D, s) : occluded(sc, O, D, s, tm);
  out[k] = b ? 1 : 0;
}

// k_ao_resolve: out = ao_byte of every record, nothing shot: 4 bytes in and 1 out a pixel,
// memory-bound.  Lane i takes the four records from `head` + 4 i on, 16 bytes in and one aligned
// dword out (`head`: the pixels in front of out's first 4-byte boundary); with `wide` the 16 bytes
// are one load (the records there are 16-byte aligned).  The thread behind the last group takes
// the at most 3 + 3 pixels of the head and the tail one by one.
__global__ void __launch_bounds__(256) k_ao_resolve(const uint32_t* __restrict__ ao,
                                                    unsigned long long pixels, unsigned head,
                                                    unsigned long long groups, int wide,
                                                    uint8_t* __restrict__ out) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (i < groups) {
    const uint32_t* a = ao + head + 4 * i;
    uint4 r;
    if (wide) r = *(const uint4*)a;   // uniform
    else r = make_uint4(a[0], a[1], a[2], a[3]);
    *(uint32_t*)(out + head + 4 * i) =
        ao_byte(r.x) | (ao_byte(r.y) << 8) | (ao_byte(r.z) << 16) | (ao_byte(r.w) << 24);
  } else if (i == groups) {
    for (unsigned long long p = 0; p < head; ++p) out[p] = (uint8_t)ao_byte(ao[p]);
    for (unsigned long long p = head + 4 * groups; p < pixels; ++p) out[p] = (uint8_t)ao_byte(ao[p]);
  }
}

hipError_t launch_occluded_rays(const LaunchScene& s, long long n, const float* origins,
                                const float* dirs, const int* skip, const float* tmax,
                                uint8_t* out, hipStream_t stream) {
  if (n < 1 || n > (1ll << 24) || !origins || !dirs || !out) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
  const Scene sc = make_scene(s);
  hipLaunchKernelGGL(k_occluded_rays, grid, dim3(kBlock), 0, stream, sc, (unsigned)n, origins,
                     dirs, skip, tmax, out);
  return hipGetLastError();
}

hipError_t launch_ao(const LaunchScene& s, const float eye[3], const View& v, const Window& w,
                     int W, int H, const AoDirs& dirs, bool reset, void* ao, uint8_t* out,
                     unsigned long long* zcount, unsigned long long* stats,
                     hipStream_t stream) {
  if (!window_supported(w, W, H, 1) || dirs.n < 1 || dirs.n > 64 || !ao || ((uintptr_t)ao & 3u) ||
      !stats)
    return hipErrorInvalidValue;
  dim3 grid((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH);
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, w.full_w, w.full_h);
  const Eye e{eye[0], eye[1], eye[2]};
  dispatch(stage_fits(s), [&](auto st) {
    hipLaunchKernelGGL((k_ao<st.value>), grid, dim3(kBlock), 0, stream, sc, cam, v, e, dirs, W, H,
                       w.x0, w.y0, reset ? 1 : 0, (uint32_t*)ao, out, zcount, stats);
  });
  return hipGetLastError();
}

hipError_t launch_ao_resolve(const void* ao, int W, int H, uint8_t* out, hipStream_t stream) {
  if (W <= 0 || H <= 0 || !ao || !out || ((uintptr_t)ao & 3u)) return hipErrorInvalidValue;
  const unsigned long long pixels = (unsigned long long)W * (unsigned long long)H;
  unsigned long long head = (4u - ((uintptr_t)out & 3u)) & 3u;
  if (head > pixels) head = pixels;
  const unsigned long long groups = (pixels - head) / 4;
  const unsigned long long blocks = (groups + 1 + 255) / 256;   // one thread more: head and tail
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  const int wide = (((uintptr_t)ao + 4 * head) & 15u) == 0u;
  hipLaunchKernelGGL(k_ao_resolve, dim3((unsigned)blocks), dim3(256), 0, stream,
                     (const uint32_t*)ao, pixels, (unsigned)head, groups, wide, out);
  return hipGetLastError();
}

// ------------------------------------------- the G-buffer through a camera (fast) --
// rc_render_camera_gbuffer* (include/raycast_hip.h): step 1 of k_ao, stored.  k_ao's grid, scene
// staging and primary ray (view_dir at ssaa = 1, the general nearest from the eye at every eye,
// hit_frame), k_gbuffer's stores; no shade and no occluded.  frame (P or N is wanted) is a kernel
// argument's test and uniform: without it a pixel costs the scan alone and counts the direction's
// normalisation only, as k_gbuffer does.  A miss is id -1 and +0 everywhere else.
template <bool kStage>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(RC_PHASE_A_WAVES))) k_camera_gbuffer(
    Scene sc, Cam cam, View v, Eye e, int W, int H, int ox, int oy, GbufPlanes g,
    unsigned long long* __restrict__ zcount) {
  if (!RC_X0_PIXEL) sc.has_quadric = sc.has_quadric != 0;   // as k_render (RC_X0_*)
  const V3 eye = v3(e.x, e.y, e.z);
  __shared__ StageBuf<kStage> stage;
  stage_scene<kStage>(sc, stage);
  int lx, ly;
  tile_pixel(lx, ly);
  int bx, by;
  xcd_tile<0>(bx, by);
  const int x = bx * kTileW + lx, y = by * kTileH + ly;
  if (x >= W || y >= H) return;
  int zero = 0;
  const V3 d = view_dir<false>(cam, v, ox + x, oy + y, zero);
  float t;
  const int id = nearest(sc, eye, d, -1, t);
  V3 P = v3(0.0f, 0.0f, 0.0f), N = P;
  if (id < 0) t = 0.0f;
  else if (g.P || g.N) hit_frame(sc, id, eye, d, t, P, N, zero);   // uniform test
  const size_t i = (size_t)y * (size_t)W + (size_t)x;
  if (g.id) g.id[i] = id;
  if (g.t) g.t[i] = t;
  if (g.P) {
    float* q = g.P + 3 * i;
    q[0] = P.x, q[1] = P.y, q[2] = P.z;
  }
  if (g.N) {
    float* q = g.N + 3 * i;
    q[0] = N.x, q[1] = N.y, q[2] = N.z;
  }
  flush_events(zero, zcount);
}

hipError_t launch_camera_gbuffer(const LaunchScene& s, const float eye[3], const View& v,
                                 const Window& w, int W, int H, int32_t* id, float* t, float* P,
                                 float* N, unsigned long long* zcount, hipStream_t stream) {
  if (!window_supported(w, W, H, 1) || (!id && !t && !P && !N)) return hipErrorInvalidValue;
  dim3 grid((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH);
  const Scene sc = make_scene(s);
  const Cam cam = make_cam(s, w.full_w, w.full_h);
  const Eye e{eye[0], eye[1], eye[2]};
  const GbufPlanes g{id, t, P, N};
  dispatch(stage_fits(s), [&](auto st) {
    hipLaunchKernelGGL((k_camera_gbuffer<st.value>), grid, dim3(kBlock), 0, stream, sc, cam, v, e,
                       W, H, w.x0, w.y0, g, zcount);
  });
  return hipGetLastError();
}

}  // namespace rc
