// rc_kernels.h — launch interface between the host runtime (rc_api.hip, rc_sampling.hip,
// rc_shard.hip) and the kernels: the sampling family's launchers (rc_sample_kernels.hip, and
// rc_filter.hip's one and rc_guided.hip's two) first, then the renderer's and the parity
// pipeline's (rc_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rc_scene.h"

namespace rc {

// Device view of an uploaded packed scene (rc_scene.h).
struct LaunchScene {
  const rc_shape* shapes;
  const rc_light* lights;
  const rc_shade_pair* pairs;
  int n, m;
  float cam_w, cam_h;
  unsigned long long refl_mask;   // bit k: shape k reflective (n <= 64)
  int has_quadric;                // the scene has a quadric (2: none with cross terms, quad_x0)
  int o0_ok;                      // primary rays may use rc_shape::o0
  int dep_fast;                   // clean DEP entries take phase A's primary shade (Scene)
  int pin;                        // phase C's carry-point table (Scene::pin)
};

// Parity-mode workspace (device pointers), sized for W*H pixels.
struct ParityWork {
  uint8_t* cls;             // [P]   pixel class (ident / writer / dep)
  float4* wcarry;           // [P]   writer carry-out
  void* deprec;             // [P]   DepRec (phase A -> B/C)
  void* row_stats;          // [H]   RowStats (k_row_stats)
  int* row_off;             // [H]   DEP offset of each row
  int* row_soff;            // [H]   segment offset of each row
  long long* row_prevw;     // [H]   last writer pixel before each row (-1: none)
  long long* row_prevd;     // [H]   last DEP pixel before each row (-1: none)
  long long* dep_pix;       // [P]   DEP pixels in scan order
  long long* seg_key;       // [P]   per segment: the writer pixel before it (-1: none)
  int* seg_start;           // [P]   segment starts, in scan order
  void* cin;                // [P]   resolved carry-in per DEP entry (CinG tagged granules)
  int* counters;            // [16]  nseg, head, ndep, ordered, phase-C tickets, census, ...
  int* batch_state;         // [P/64+1] phase-C batch claim words (0 free, 1 claimed)
  int* batch_cnt;           // [P/64+1] entries of each batch with a published carry-in
  int* batch_rq;            // [P/64+1] batches in the order they became complete (+1; 0 empty)
  hipStream_t side;         // phase C's side stream (null: phase C after the resolver only)
  hipEvent_t fork, join;    // side stream waits on fork; the main stream waits on join
  int side_blocks;          // resident k_side workgroups
  int side_lds;             // k_side's dynamic LDS reservation (keeps it off resolver CUs)
  int split_shade;          // k_classify + colours in k_side (measured slower: off by default)
  unsigned epoch;           // this frame's carry-in tag (never 0)
  int* seg_order;           // [kSegOrderMax] segments longest first (k_seg_order)
  void* team;               // TeamState of the long-segment team
  int resolve_blocks;       // persistent resolver grid (<= resident capacity)
  int resolve_lds;          // dynamic LDS per resolver block (occupancy control)
  int team_blocks;          // workgroups in the long-segment team (0: no team)
  int helpers;              // workgroups taking handed-off dense runs (0: none)
  int hand_run;             // changes in a row before a regular wave hands its run off
  int long_len;             // segments with >= long_len entries go to the team
  int phase_c_blocks;       // grid-stride phase C grid
  int phase_c_finish;       // phase C after the resolver through k_finish's claims (RC_PHASE_C_FINISH)
  int wave_k;               // clean cooperative steps before a wave window goes back to LANE
  int resolve_k;            // the same for the team leader's block window
  int resolve_clean;        // clean windows in a row that end a RESOLVE round
  int team_cscan;           // cooperative SCAN rounds after RESOLVE rounds (early hand-back)
  int coop_group;           // lanes per entry of the cooperative evaluator (0: off)
  unsigned* trace;          // optional [2*nseg] per-segment {ticks, evals} (debug)
  // Pipelined frames (rc_frame_submit): the resolver runs on its own stream (a CU partition
  // of its own) between two hand-off events; null rstream = everything on the main stream.
  hipStream_t rstream;
  hipStream_t pstream;      // phase C's stream (null: the main stream)
  hipEvent_t rready, rdone; // main -> rstream after compaction; rstream -> pstream after it
  hipEvent_t rt0, rt1;      // optional: resolver start / end on rstream
  hipEvent_t adone;         // optional: recorded after phase A (pipelined phase A order)
  hipStream_t cstream;      // optional (with adone): compaction on this stream after adone
  uint32_t* patch;          // optional [P] packed RGB of DEP entry j (rc_render's overlapped copy)
  int defer_c;              // pipelined: launch_parity stops after the resolver; phase C is
                            // enqueued later by launch_phase_c (after rdone)
  int inject;               // test aid: the resolver raises its error word (code 4) at start
  int batch_ints;           // ints from batch_state on (claims, counts, queue), cleared by k_row_stats
  int inres;                // phase C inside the resolver: its waves shade ready batches once
                            // their own work is done (rc_tuning.side 3)
  int block_min;            // regular segments of >= block_min entries get a whole workgroup
  int headb_first;          // regular workgroups that start on the per-wave queue (head B) at once
};

constexpr int kSegOrderMax = 65536;   // segments ordered for the resolver queue (else FIFO)
constexpr int kCinBytes = 24;         // one carry-in = three tagged 8-byte granules
constexpr int kLdsShapesMax = 64;     // k_resolve stages up to this many shapes in LDS
constexpr int kDenseSlots = 64;       // k_resolve's hand-off ring (helper workgroups at most)

// ------------------------------------ defined in rc_sample_kernels.hip: the sampling family --
// Supersampled fast mode (rc_options.ssaa = 2, 4 or 8), fused: rows row0 + k*row_step of the
// W x H box-filtered image into `out`; the ssaa*W x ssaa*H subsample image is never stored.
// zcount counts the zero-normalize events of every subsample.
hipError_t launch_render_ssaa(const LaunchScene& s, int W, int H, int ssaa, int row0, int row_step,
                              int nrows, int maxrec, uint8_t* out, unsigned long long* zcount,
                              hipStream_t stream);
// The two-pass path's box filter: dst (W x H) <- src (ssaa*W x ssaa*H), both compact RGB.
hipError_t launch_box_down(const uint8_t* src, int W, int H, int ssaa, uint8_t* dst,
                           hipStream_t stream);
// The separable reconstruction filter (rc_filter.hip; rc_filter in include/raycast_hip.h):
// dst (W x H) <- src (ssaa*W x ssaa*H) through the ntaps = ssaa + 2h integer taps, applied along
// x and along y with src's coordinates clamped to the image.  hipErrorInvalidValue for anything
// rc_filter_check or the size limits (W, H <= 2^28 / ssaa) refuse.  src and dst must not overlap.
constexpr int kFilterMaxTaps = 24;
// the output tile one workgroup owns, per factor
constexpr int filter_tile_w(int ssaa) { return ssaa == 8 ? 16 : 32; }
constexpr int filter_tile_h(int ssaa) { return ssaa == 2 ? 16 : 8; }
hipError_t launch_filter_down(const uint8_t* src, int W, int H, int ssaa, const int16_t* taps,
                              int ntaps, uint8_t* dst, hipStream_t stream);

// Adaptive supersampling (rc_options.ssaa = RC_SSAA_ADAPTIVE(s, t); fast and cuda modes), after
// launch_render has put the one-ray W x H image into `img`, all on one stream:
//   launch_aa_mark    appends the index y*W + x of every pixel whose 3x3 contrast is >= threshold
//                     to `list` (W*H entries of room) and counts them in *count (zeroed by the
//                     caller, on the stream); W*H >= 2^32 is refused;
//   launch_aa_refine  shoots the ssaa x ssaa subsamples of the listed pixels with the camera of
//                     the ssaa*W x ssaa*H image and stores their box filter over `out`'s pixels;
//                     `blocks` workgroups (aa_refine_blocks) stride over the list, whose length
//                     is read on the device.  zcount: the subsamples' zero-normalize events (fast).
// Mark reads pixels that refine overwrites: they must stay two launches.
hipError_t launch_aa_mark(const uint8_t* img, int W, int H, int threshold, uint32_t* list,
                          unsigned* count, hipStream_t stream);
hipError_t launch_aa_refine(const LaunchScene& s, int W, int H, int ssaa, int maxrec,
                            const uint32_t* list, const unsigned* count, uint8_t* out,
                            unsigned long long* zcount, int blocks, hipStream_t stream,
                            bool cuda_sem);
// want > 0: that many; else from the CU count, at most the wave steps a W x H list can need
int aa_refine_blocks(int W, int H, int ssaa, int cus, int want);

// Supersampling by a per-pixel rate map (rc_render_rates*; fast and cuda modes), all on one
// stream.  cnt is five words zeroed by the caller on the stream: [0] [1] [2] the lengths of the
// rate-2, rate-4 and rate-8 lists, [3] the rate-1 pixels, [4] the map bytes that are no rate.
//   launch_rates_render   shoots the rate-1 pixels of `rates` (W*H bytes) into `out` and lists
//                         the others: rate 4 in list4, rate 2 upwards from list28[0], rate 8
//                         downwards from list28[W*H - 1] (W*H entries each);
//   launch_aa_refine      (above) then serves the rate-2 list (list28, cnt) and the rate-4 list
//                         (list4, cnt + 1);
//   launch_rates_refine8  serves the rate-8 list (list28, cnt + 2) with `blocks` workgroups.
// rates_supported: W*H < 2^32, 8*W and 8*H within int, a grid the tile layout can address.
int rates_supported(int W, int H);
hipError_t launch_rates_render(const LaunchScene& s, int W, int H, int maxrec,
                               const uint8_t* rates, uint8_t* out, uint32_t* list4,
                               uint32_t* list28, unsigned* cnt, unsigned long long* zcount,
                               hipStream_t stream, bool cuda_sem);
hipError_t launch_rates_refine8(const LaunchScene& s, int W, int H, int maxrec,
                                const uint32_t* list28, const unsigned* count, uint8_t* out,
                                unsigned long long* zcount, int blocks, hipStream_t stream,
                                bool cuda_sem);

// Sparse sample patterns (rc_render_pattern*; fast and cuda modes): n samples (2, 4, 8 or 16,
// n <= g*g) of every refined pixel at the positions (px[k], py[k]) of its g x g subsample lattice
// (g = 2, 4 or 8), shot with the camera of the g*W x g*H image, n lanes a pixel; the rounded
// mean (sum + n/2) / n is stored.  The positions travel to the kernels as 4-bit entries of two
// 64-bit kernel arguments.
//   launch_pattern       every pixel of the W x H image (256 / n pixels per workgroup);
//   launch_pattern_list  the pixels launch_aa_mark listed, over `out`'s one-ray pixels, with
//                        `blocks` workgroups (pattern_list_blocks) striding over the list, whose
//                        length is read on the device.
// zcount: the samples' zero-normalize events (fast).
// pattern_supported: g, n as above; W, H in 1 .. 2^28 / g; a grid the tile layout can address
// (dense: at most 65535 rows of tiles and 2^31 - 1 tiles; listed: W*H < 2^32 and k_render's
// rows of tiles).  The launchers return hipErrorInvalidValue for anything it refuses.
int pattern_supported(int W, int H, int g, int n, bool listed);
hipError_t launch_pattern(const LaunchScene& s, int W, int H, int g, int n, const uint8_t* px,
                          const uint8_t* py, int maxrec, uint8_t* out,
                          unsigned long long* zcount, hipStream_t stream, bool cuda_sem);
hipError_t launch_pattern_list(const LaunchScene& s, int W, int H, int g, int n,
                               const uint8_t* px, const uint8_t* py, int maxrec,
                               const uint32_t* list, const unsigned* count, uint8_t* out,
                               unsigned long long* zcount, int blocks, hipStream_t stream,
                               bool cuda_sem);
// want > 0: that many; else from the CU count, at most the wave steps a W x H list can need
int pattern_list_blocks(int W, int H, int n, int cus, int want);

// Progressive supersampling (rc_accum_pass_device, rc_render_accum; fast and cuda modes): `acc`
// holds one rc_accum_px per pixel (8 bytes, 8-byte aligned: the sums of the sample bytes taken so
// far and their number n); a pass shoots `count` (1..16) further samples at the positions
// (px[j], py[j]), j < count, of the g x g lattice with the camera of the g*W x g*H image, one
// lane a pixel, adds them to the record and stores the rounded mean of all n + count samples in
// `out`.  A pixel with n + count > 256 is left as it is and counted in *sat (zeroed by the caller
// on the stream).
//   launch_accum          every pixel (k_render's tiles); reset: the records are not read and
//                         count as zero;
//   launch_accum_list     the pixels launch_aa_mark listed from `out`, with `blocks` workgroups
//                         (accum_list_blocks) striding over the list, whose length is read on the
//                         device; the other pixels' records and bytes are not stored to;
//   launch_accum_resolve  out = the rounded means of `acc`, nothing shot ((0, 0, 0) where n = 0).
// accum_supported: g in {2, 4, 8}; W, H in 1 .. 2^28 / g; dense: at most 65535 rows of tiles and
// 2^31 - 1 tiles; listed: W*H < 2^32 and a grid launch_aa_mark can address.  The launchers return
// hipErrorInvalidValue for anything it refuses.
int accum_supported(int W, int H, int g, bool listed);
hipError_t launch_accum(const LaunchScene& s, int W, int H, int g, int count, const uint8_t* px,
                        const uint8_t* py, bool reset, int maxrec, void* acc, uint8_t* out,
                        unsigned long long* zcount, unsigned* sat, hipStream_t stream,
                        bool cuda_sem);
hipError_t launch_accum_list(const LaunchScene& s, int W, int H, int g, int count,
                             const uint8_t* px, const uint8_t* py, int maxrec,
                             const uint32_t* list, const unsigned* nlist, void* acc, uint8_t* out,
                             unsigned long long* zcount, unsigned* sat, int blocks,
                             hipStream_t stream, bool cuda_sem);
hipError_t launch_accum_resolve(const void* acc, int W, int H, uint8_t* out, hipStream_t stream);
// want > 0: that many; else from the CU count, at most the wave steps a W x H list can need
int accum_list_blocks(int W, int H, int cus, int want);

// Windows of a virtual image (rc_render_window*, rc_accum_pass_window_device; fast and cuda
// modes): the W x H output is the rectangle at (x0, y0) of the full_w x full_h image, shot with
// the camera of the s*full_w x s*full_h image (rc_window's fields).
//   launch_window             the ssaa = s image of the window (s = 1, 2, 4 or 8), one lane per
//                             subsample over the window's own subsample grid, nothing stored but
//                             the W x H output;
//   launch_accum_window       launch_accum with the window's origin (s = the sequence's g);
//   launch_accum_list_window  launch_accum_list with it; list, acc and out are the window's own.
// window_supported: s as above; the window inside the image, all sizes >= 1, the origin >= 0;
// s*full_w and s*full_h within int; at most 65535 rows of tiles and 2^31 - 1 tiles in the window's
// subsample grid.  The accumulation launchers add accum_supported(W, H, g, listed).  The launchers
// return hipErrorInvalidValue for anything these refuse.
struct Window {
  int full_w, full_h, x0, y0;
};
int window_supported(const Window& w, int W, int H, int s);
hipError_t launch_window(const LaunchScene& s, const Window& w, int W, int H, int ssaa, int maxrec,
                         uint8_t* out, unsigned long long* zcount, hipStream_t stream,
                         bool cuda_sem);
hipError_t launch_accum_window(const LaunchScene& s, const Window& w, int W, int H, int g,
                               int count, const uint8_t* px, const uint8_t* py, bool reset,
                               int maxrec, void* acc, uint8_t* out, unsigned long long* zcount,
                               unsigned* sat, hipStream_t stream, bool cuda_sem);
hipError_t launch_accum_list_window(const LaunchScene& s, const Window& w, int W, int H, int g,
                                    int count, const uint8_t* px, const uint8_t* py, int maxrec,
                                    const uint32_t* list, const unsigned* nlist, void* acc,
                                    uint8_t* out, unsigned long long* zcount, unsigned* sat,
                                    int blocks, hipStream_t stream, bool cuda_sem);

// Scrolling an accumulated view (rc_accum_scroll_device; fast and cuda modes): the window moved
// by (dx, dy) = new origin - old origin, source and destination two states of the same W x H.
// scroll_rects: the kept rectangle K in destination coordinates, kw x kh at (kx, ky) (kw = kh = 0:
// nothing is kept), and the exposed set, the complement of K, as four rectangles in the order rows
// above K, columns left of K, columns right of K, rows below K: rectangle k holds entries
// [first[k], first[k + 1]) of [0, total), row-major, w[k] wide (1 where it is empty) at
// (x[k], y[k]).  total = W*H - kw*kh.  W*H >= 2^32 or a side below 1: everything is 0.
//   launch_accum_move     the records and bytes of K from the source to the destination, nothing
//                         shot; the arrays must not overlap;
//   launch_accum_exposed  `count` (1..16) samples for every exposed pixel of the window `w`, with
//                         `blocks` workgroups (accum_exposed_blocks) striding over the exposed set;
//                         reset: the records are not read and count as zero.  acc and out are the
//                         destination's; the pixels of K are not stored to.
// Both return hipErrorInvalidValue for what accum_supported(W, H, g, true) refuses; the former
// for an empty K, the latter for an empty exposed set, a window outside its image, count outside
// 1..16 and blocks outside 1..4096.
struct ScrollRects {
  unsigned first[4], w[4];
  int x[4], y[4];
  unsigned total;
  int kx, ky, kw, kh;
};
ScrollRects scroll_rects(int W, int H, int dx, int dy);
hipError_t launch_accum_move(int W, int H, int g, int dx, int dy, const void* acc_src,
                             const uint8_t* out_src, void* acc_dst, uint8_t* out_dst,
                             hipStream_t stream);
hipError_t launch_accum_exposed(const LaunchScene& s, const Window& w, int W, int H, int g,
                                int dx, int dy, int count, const uint8_t* px, const uint8_t* py,
                                bool reset, int maxrec, void* acc, uint8_t* out,
                                unsigned long long* zcount, int blocks, hipStream_t stream,
                                bool cuda_sem);
// want > 0: that many; else from the CU count, at most the wave steps `exposed` pixels can need
int accum_exposed_blocks(unsigned exposed, int cus, int want);

// The primary-visibility G-buffer (rc_render_gbuffer*, rc_pick*, rc_id_edge_rates_device; fast,
// parity and cuda modes): the primary hit of every pixel of a window, or of n points of the
// full_w x full_h image, and the rate map of an id plane's edges.
//   launch_gbuffer         one lane per pixel over launch_window's grid at s = 1; a null plane is
//                          not stored (at least one is not null); P and N (three floats a pixel)
//                          not in cuda mode;
//   launch_gbuffer_points  one lane per point, n in 1 .. 2^24; xy: n (x, y) pairs; hits: n 32-byte
//                          rc_hit records, 16-byte aligned; frame: P and N too (not in cuda mode);
//                          a point outside the image gets id = -2 and zeros;
//   launch_id_edge_rates   rates = s where the clipped 3 x 3 neighbourhood of `id` holds another
//                          value, else base; no scene, no workspace.
// The launchers return hipErrorInvalidValue for what window_supported(w, W, H, 1) or
// id_edge_rates_supported refuses and for the rules above.
hipError_t launch_gbuffer(const LaunchScene& s, const Window& w, int W, int H, int32_t* id,
                          float* t, float* P, float* N, unsigned long long* zcount,
                          hipStream_t stream, bool cuda_sem);
hipError_t launch_gbuffer_points(const LaunchScene& s, int full_w, int full_h, bool frame,
                                 long long n, const int32_t* xy, void* hits,
                                 unsigned long long* zcount, hipStream_t stream, bool cuda_sem);
// s in {2, 4, 8}, base in {0, 1}, both sides at least 1, W * H below 2^32
int id_edge_rates_supported(int W, int H, int s, int base);
hipError_t launch_id_edge_rates(const int32_t* id, int W, int H, int s, int base, uint8_t* rates,
                                hipStream_t stream);

// Rotated camera views and caller-supplied ray batches (rc_render_view*, rc_trace_rays*; fast and
// cuda modes): rays from the origin whose directions are not the pinhole grid's.
//   launch_view  launch_window with the view matrix m (rc_view::m, row-major) applied to the
//                unnormalised primary vector of every subsample before the one normalisation;
//                the same grid, lanes and limits (window_supported);
//   launch_rays  one lane per direction, n in 1 .. 2^24; dirs: n x 3 floats used as given; any of
//                rgb8 (n x 3 bytes), rgb (n x 3 floats, the colour before quantisation) and hits
//                (n 32-byte rc_hit records, 16-byte aligned) may be null, one is not; frame: P and
//                N in the records (not in cuda mode).
// The launchers return hipErrorInvalidValue for what breaks these rules.
struct View {
  float m[9];
};
hipError_t launch_view(const LaunchScene& s, const View& v, const Window& w, int W, int H,
                       int ssaa, int maxrec, uint8_t* out, unsigned long long* zcount,
                       hipStream_t stream, bool cuda_sem);
hipError_t launch_rays(const LaunchScene& s, long long n, const float* dirs, int maxrec,
                       uint8_t* rgb8, float* rgb, void* hits, bool frame,
                       unsigned long long* zcount, hipStream_t stream, bool cuda_sem);

// A free camera and rays with origins (rc_render_camera*, rc_trace_rays_from*; fast mode only).
//   launch_camera     launch_view with every primary ray leaving eye (three floats, used as
//                     given); an eye of three +0 is launch_view itself;
//   launch_rays_from  launch_rays with an origin per ray (origins: n x 3 floats, device memory,
//                     not looked at by the launcher).
hipError_t launch_camera(const LaunchScene& s, const float eye[3], const View& v, const Window& w,
                         int W, int H, int ssaa, int maxrec, uint8_t* out,
                         unsigned long long* zcount, hipStream_t stream);
hipError_t launch_rays_from(const LaunchScene& s, long long n, const float* origins,
                            const float* dirs, int maxrec, uint8_t* rgb8, float* rgb, void* hits,
                            bool frame, unsigned long long* zcount, hipStream_t stream);

// Accumulation through a free camera (rc_accum_pass_camera_device, rc_render_camera_accum; fast
// mode only): launch_accum_window and launch_accum_list_window with sample j of the pass shot as
// launch_camera shoots a subsample, through camera j of `cams`.  The cameras travel by value as a
// kernel argument (768 bytes) and are read with the pass's uniform sample index, so a caller with
// one camera for the whole pass fills every slot it uses with that camera.  Slots at and past
// `count` are not read.  An eye of three +0 is not dispatched anywhere else: the general nearest
// at +0 gives the origin forms' bits.  The guards are the window launchers'.
struct CamSet {
  float eye[16][3];
  View view[16];
};
static_assert(sizeof(CamSet) == 768, "16 eyes and 16 views, one kernel argument");
hipError_t launch_accum_cam(const LaunchScene& s, const CamSet& cams, const Window& w, int W,
                            int H, int g, int count, const uint8_t* px, const uint8_t* py,
                            bool reset, int maxrec, void* acc, uint8_t* out,
                            unsigned long long* zcount, unsigned* sat, hipStream_t stream);
hipError_t launch_accum_list_cam(const LaunchScene& s, const CamSet& cams, const Window& w, int W,
                                 int H, int g, int count, const uint8_t* px, const uint8_t* py,
                                 int maxrec, const uint32_t* list, const unsigned* nlist,
                                 void* acc, uint8_t* out, unsigned long long* zcount,
                                 unsigned* sat, int blocks, hipStream_t stream);

// Any-hit visibility queries and ambient occlusion (rc_occluded_rays*, rc_ao_pass_device,
// rc_ao_resolve_device, rc_render_ao; fast mode only).
//   launch_occluded_rays  one lane per ray, n in 1 .. 2^24; origins, dirs: n x 3 floats used as
//                         given; skip (n ints) and tmax (n floats) may be null: -1 and +inf
//                         everywhere; out: one byte a ray, 1 blocked.  tmax = +inf takes shadowed,
//                         anything else occluded (rc_device.hpp), lane by lane;
//   launch_ao             launch_camera's primary ray at ssaa = 1 (the general nearest at every
//                         eye), then from a hit the set's n directions, flipped into the normal's
//                         hemisphere, with skip = the hit shape and the set's tmax; ao: one 4-byte
//                         record a pixel (open | rays << 16), 4-byte aligned; reset: not read, counts
//                         as zero; out: W*H bytes or null; stats: kAoStatBytes of counters, zeroed by
//                         the caller: kAoStatSlots lines of kAoStatStride 64-bit words, the first
//                         three of a line {hit pixels, blocked rays, saturated pixels}; a wave adds
//                         to one line with one atomic a counter, and the sums over the lines are
//                         the pass's counts (one line for all would serialise the pass's waves).
//                         The set travels by value as a kernel argument (776 bytes) and is read
//                         with the uniform direction index.  The guards are window_supported's
//                         at factor 1 and n in 1..64;
//   launch_ao_resolve     out = the bytes of `ao`, nothing shot (255 where rays = 0).
// The launchers return hipErrorInvalidValue for what breaks these rules.
struct AoDirs {
  int n;
  float tmax;
  float u[64][3];
};
static_assert(sizeof(AoDirs) == 776, "rc_ao_dirs' layout, one kernel argument");
constexpr int kAoStatSlots = 256;    // a power of two
constexpr int kAoStatStride = 16;    // 64-bit words: a 128-byte line a slot
constexpr size_t kAoStatBytes = (size_t)kAoStatSlots * kAoStatStride * sizeof(unsigned long long);
hipError_t launch_occluded_rays(const LaunchScene& s, long long n, const float* origins,
                                const float* dirs, const int* skip, const float* tmax,
                                uint8_t* out, hipStream_t stream);
hipError_t launch_ao(const LaunchScene& s, const float eye[3], const View& v, const Window& w,
                     int W, int H, const AoDirs& dirs, bool reset, void* ao, uint8_t* out,
                     unsigned long long* zcount, unsigned long long* stats,
                     hipStream_t stream);
hipError_t launch_ao_resolve(const void* ao, int W, int H, uint8_t* out, hipStream_t stream);

// The G-buffer through a camera, the guided filter of the occlusion records and the ambient
// compose (rc_render_camera_gbuffer*, rc_ao_filter_device, rc_ao_compose_device; fast mode only).
//   launch_camera_gbuffer  launch_ao's primary ray, stored: id, t, P, N of the general nearest from
//                          `eye` and its hit_frame, a null plane is not stored, a miss is id -1 and
//                          +0 everywhere else (rc_sample_kernels.hip);
//   launch_ao_filter       out = the cross-bilateral pooling of the records `ao` (launch_ao's
//                          dwords, 4-byte aligned) guided by id, P (3 W floats a row) and N, all
//                          W x H and non-null; no scene (rc_guided.hip).  The filter travels by
//                          value (32 bytes).  The guards: radius 0..kAoFilterMaxRadius, both sides
//                          1 .. kGuidedMaxSide (one workgroup a 16 x 16 tile, grid.y <= 65535);
//   launch_ao_compose      out = in + the ambient term of the pixel's shape scaled by ao / 255,
//                          saturated; diffuse: n x 3 floats of the uploaded scene; out may be in.
// hipErrorInvalidValue for what breaks these rules.
constexpr int kAoFilterMaxRadius = 8;
constexpr int kGuidedMaxSide = 16 * 65535;
struct AoFilter {
  int radius;
  float nmin, dplane;
  uint16_t taps[kAoFilterMaxRadius + 1];
  uint16_t pad;
};
static_assert(sizeof(AoFilter) == 32, "rc_ao_filter's layout, one kernel argument");
struct Ambient {
  float c[3];
};
hipError_t launch_camera_gbuffer(const LaunchScene& s, const float eye[3], const View& v,
                                 const Window& w, int W, int H, int32_t* id, float* t, float* P,
                                 float* N, unsigned long long* zcount, hipStream_t stream);
hipError_t launch_ao_filter(const void* ao, const int32_t* id, const float* P, const float* N,
                            int W, int H, const AoFilter& f, uint8_t* out, hipStream_t stream);
hipError_t launch_ao_compose(const float* diffuse, int n_shapes, const Ambient& ambient,
                             const int32_t* id, const uint8_t* ao, const uint8_t* in, uint8_t* out,
                             int W, int H, hipStream_t stream);

// ------------------- defined in rc_kernels.hip: the renderer, the parity pipeline, row shards --
// cuda_sem: RC_MODE_CUDA (the CUDA port's arithmetic, rc_cudasem.hpp) instead of fast mode
hipError_t launch_render(const LaunchScene& s, int W, int H, int row0, int row_step, int nrows,
                         int maxrec, uint8_t* out, unsigned long long* zcount,
                         hipStream_t stream, bool cuda_sem = false);

hipError_t launch_parity(const LaunchScene& s, int W, int H, int maxrec, uint8_t* out,
                         const ParityWork& w, unsigned long long* zcount, hipStream_t stream,
                         const hipEvent_t* ev);

// Top byte of a colour-patch entry (ParityWork::patch) once phase C has stored it: the frame's
// mark, 0x80 | (epoch & 0x7f) of its carry-in epoch (never 0, the cleared value); the low three
// bytes are R, G, B.  rc_render's host side
// only reads the array during a frame (an entry is this frame's once its top byte is this
// frame's mark) and never stores to it then: a host store into a line that phase C is still
// writing in pieces (k_dep_chunks) was seen undone by the device's later store to that line,
// leaving a stale mark (round 6, profiles/r06n_patch_marks.txt).  Marks of kPatchMarks
// consecutive epochs are distinct, so the array is cleared once per kPatchMarks epochs
// (ensure_host_patch).
constexpr unsigned kPatchMarks = 128;
__host__ __device__ constexpr uint32_t patch_mark(unsigned epoch) {
  return (epoch << 24) | 0x80000000u;
}

// Phase C of a frame launched with defer_c: waits for w.rdone on `stream`.
hipError_t launch_phase_c(const LaunchScene& s, int W, int H, int maxrec, uint8_t* out,
                          const ParityWork& w, unsigned long long* zcount, hipStream_t stream);

// Row shards (rc_shard.hip; wire formats in rc_kernels.hip).  kMaxShards ranks at most.
constexpr int kMaxShards = 16;
size_t shard_entry_bytes();   // one DEP entry on the wire
size_t shard_row_bytes();     // one row summary on the wire
// A rank: phase A on rows row0 + k*row_step (k < nrows) into rank-local buffers, the local
// DEP list (w.dep_pix, local pixels; w.counters[2] = entries) and the wire entries / rows.
// img_rec / img_wcarry (the root): DEP lines and writer carries go straight to the root
// resolver's image-indexed buffers and its entries are thin {image pixel, writer} pairs.
hipError_t launch_shard_local(const LaunchScene& s, int W, int H, int row0, int row_step,
                              int nrows, int maxrec, uint8_t* out, const ParityWork& w,
                              void* ent, void* rows, unsigned long long* zcount,
                              hipStream_t stream, void* img_rec = nullptr,
                              float4* img_wcarry = nullptr);
// The root: image scan order from the gathered rows ([G][rmax]) and entries (rank g's at
// offs[g]) in a lone frame's layout (pixel-indexed records, primary shades and writer carries
// in w.deprec / w.wcarry, which hold W*H + 1 pixels: the last is a spare for entries beyond a
// fixed-size exchange's bound), the carry resolver with phase C inside it (w.inres) and the
// phase C tail, shading every DEP entry into `out` (W*H + 1 pixels; its non-DEP pixels are the
// gathered row blocks).  ev (optional): [0] resolver start, [1] resolver end.  bound: entries
// delivered per rank (the fixed-size exchange; beyond it a rank's list is not read as records).
// ent0 (optional): rank 0's entries, read in place (the root's own list is not gathered).
hipError_t launch_shard_resolve(const LaunchScene& s, int W, int H, int G, int rmax,
                                const void* rows_all, const void* ent_all, const void* ent0,
                                const long long* offs, int maxrec, const ParityWork& w,
                                uint8_t* out, unsigned long long* zcount, hipStream_t stream,
                                const hipEvent_t* ev, int bound = 0x7fffffff, int thin0 = 0);
// The root: image <- gathered row blocks [G][rmax][W*3]; block0 (optional): rank 0's block in
// place of gathered[0] (the root's own rows are not copied).
hipError_t launch_deinterleave(const uint8_t* gathered, const uint8_t* block0, int G, int rmax,
                               int W, int H, uint8_t* img, hipStream_t stream);

size_t deprec_bytes();
size_t row_stats_bytes();
size_t team_state_bytes();
size_t team_dq_offset();   // DenseQueue {prod, claim, finished} inside TeamState
size_t team_slot_offset(); // the team's hand-off slots: [team_slot_bufs()][team_slot_blocks()]
int team_slot_bufs();      //   x 4 tagged granules {payload, round}
int team_slot_blocks();
size_t team_handoff_diag_offset();   // 0 unless an RC_HANDOFF_DIAG build
int resolve_blocks_resident(int cus, int lds_bytes);
// k_resolve<true>'s resources: registers per lane (VGPRs + AGPRs), scratch bytes per lane, and
// the workgroups one CU can hold with `lds_bytes` of dynamic LDS each (occupancy API).
int resolve_resources(int lds_bytes, int* regs, int* scratch, int* wg_per_cu);
int side_lds_bytes(int resolve_dyn_lds);
int phase_c_side_blocks(int cus, int side_lds);

}  // namespace rc
