// rc_sampling.hip — the sampling features of libraycast_hip.so's C-ABI (include/raycast_hip.h):
// rate maps, reconstruction filters, sparse sample patterns, progressive accumulation, windows of a
// virtual image, the primary-visibility G-buffer, rotated views and ray batches, the free camera
// and rays with origins, accumulation through free cameras, any-hit visibility queries with the
// ambient-occlusion pass and the camera's G-buffer, guided filter and ambient compose, with adaptive
// supersampling's getters.  Host code only: the kernels are
// rc_sample_kernels.hip's, rc_filter.hip's and rc_guided.hip's (the one-ray image is rc_kernels.hip's k_render), the device context and the frame scaffold (enter,
// ws_frame, claim_event_set, finish_device, finish_host) are rc_api.hip's, through rc_runtime.h.
//
// A feature is one Refusal description, one enqueue body between SampleFrame::begin and ::end,
// one record in DevCtx and two entry points that are their null checks, `refused` and one call
// of device_entry or host_entry.  Nothing here reads a build-time
// diagnostic switch, so one object serves every variant of the library.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "raycast_hip.h"
#include "rc_kernels.h"
#include "rc_runtime.h"
#include "rc_scene.h"

using namespace rcrt;

// ---------------------------------------------------------------------- refusals --
// What a feature's entry points refuse from their arguments alone, before the first HIP call.
// The clauses are tested in the order of the fields; a null message switches its clause off.
// Every message is a whole format string that starts with the entry point's name.
struct Refusal {
  const char* adaptive;   // (who, opt->ssaa): no adaptive threshold in the options
  int factor_min;         // 1: the options' factor must be off (the feature carries its own grid);
  const char* factor;     // 2: it must be 2, 4 or 8; (who, opt->ssaa)
  const char* mode;       // (who): fast and cuda mode only
  const char* shards;     // (who, opt->num_gpus): one GPU only
  // check(ss): the feature's own check of its argument, which prints its own message
  // then: the threshold in 0..255
  const char* side;       // (who, W, H, g): both sides in 1 .. 2^28 / g
  // then: with `masked`, W * H below 2^32; then supported(ss): the kernels' grid limits
};

static int no_check(int) { return 0; }

// a refusal's message on stderr; -1
__attribute__((format(printf, 1, 2))) static int say(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vfprintf(stderr, fmt, ap);
  va_end(ap);
  return -1;
}

// an environment reader's warning on stderr; 0: the variable is ignored
__attribute__((format(printf, 1, 2))) static int warn(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vfprintf(stderr, fmt, ap);
  va_end(ap);
  return 0;
}

// g: the lattice the side limit is taken at (0: the options' factor); threshold and masked: of
// the features that take an edge threshold as an argument (0 and false elsewhere).
template <class Check, class Supported>
static int refused(const Refusal& d, const char* who, const rc_options* opt, int W, int H, int g,
                   int threshold, bool masked, Check check, Supported supported) {
  const int ss = ssaa_factor(opt, who);
  if (ss < 0) return -1;   // ssaa_decode has said why (a threshold without a factor included)
  if (d.adaptive && RC_SSAA_THRESHOLD(opt->ssaa) > 0) return say(d.adaptive, who, opt->ssaa);
  if (d.factor && (d.factor_min == 1 ? ss > 1 : ss < d.factor_min))
    return say(d.factor, who, opt->ssaa);
  if (d.mode && opt->mode != RC_MODE_FAST && opt->mode != RC_MODE_CUDA) return say(d.mode, who);
  if (opt->num_gpus > 1) return say(d.shards, who, opt->num_gpus);
  if (check(ss)) return -1;
  if (threshold < 0 || threshold > 255)
    return say("Error: %s: threshold %d is not 0..255\n", who, threshold);
  if (g == 0) g = ss;
  if (d.side && (W <= 0 || H <= 0 || W > (1 << 28) / g || H > (1 << 28) / g))
    return say(d.side, who, W, H, g);
  if (masked && (unsigned long long)W * (unsigned long long)H >= (1ull << 32))
    return say("Error: %s: %d x %d with a threshold is too large (32-bit pixel indices)\n", who, W,
               H);
  return supported(ss) ? -1 : 0;
}

static const char kLatticeSide[] =
    "Error: %s: %d x %d on a lattice of %d: both sides must be 1 .. 2^28 / g\n";

static const Refusal kFilteredRefusal = {
    "Error: %s: an adaptive threshold (ssaa %d): a refined pixel's filter footprint would reach "
    "its unrefined neighbours' subsamples; use a plain factor\n",
    2, "Error: %s: ssaa %d: a filtered frame needs a factor of 2, 4 or 8\n",
    nullptr,
    "Error: %s: num_gpus %d: the row shards do not supersample\n",
    "Error: %s: %d x %d at factor %d: both sides must be 1 .. 2^28 / s\n"};

static const Refusal kPatternRefusal = {
    nullptr,
    1, "Error: %s: ssaa %d in the options: the pattern carries the grid, leave ssaa at 0 or 1\n",
    "Error: %s: a sample pattern is for fast and cuda mode: every pixel of a parity image depends "
    "on the scan-order carry of the whole image, so it cannot be shot sparsely; use plain ssaa\n",
    "Error: %s: num_gpus %d: the row shards take no sample pattern\n",
    kLatticeSide};

static const Refusal kAccumRefusal = {
    nullptr,
    1, "Error: %s: ssaa %d in the options: the sample sequence carries the grid, leave ssaa at 0 "
    "or 1\n",
    "Error: %s: accumulated samples are for fast and cuda mode: every pixel of a parity image "
    "depends on the scan-order carry of the whole image, so it cannot be shot sparsely; use plain "
    "ssaa\n",
    "Error: %s: num_gpus %d: the row shards take no accumulator\n",
    kLatticeSide};

static const Refusal kWindowRefusal = {
    "Error: %s: ssaa %d carries an adaptive threshold: adaptive refinement of a window is an "
    "accumulation pass with a threshold (rc_accum_pass_window_device)\n",
    0, nullptr,
    "Error: %s: windows are for fast and cuda mode: a window of a parity image depends on the "
    "scan-order carry of every pixel before it\n",
    "Error: %s: num_gpus %d: the row shards take no window\n",
    nullptr};   // rc_window_check tests the sizes

static const Refusal kRatesRefusal = {
    nullptr,
    1, "Error: %s: ssaa %d in the options: the rate map carries the factor per pixel, leave ssaa "
    "at 0 or 1\n",
    "Error: %s: a rate map is for fast and cuda mode: every pixel of a parity image depends on "
    "the scan-order carry of the whole image, so it cannot be shot sparsely\n",
    "Error: %s: num_gpus %d: the row shards take no rate map\n",
    nullptr};   // rc::rates_supported tests the sizes

// One argument order (who, opt, W, H, the feature's own) and one return: -1 refused, 0 passed.
// A caller that needs the factor afterwards takes it from ssaa_factor.
static int filtered_refused(const char* who, const rc_options* opt, int W, int H,
                            const rc_filter* f) {
  return refused(kFilteredRefusal, who, opt, W, H, 0, 0, false,
                 [&](int ss) { return rc_filter_check(f, ss); }, no_check);
}

static int pattern_refused(const char* who, const rc_options* opt, int W, int H,
                           const rc_pattern* pat, int threshold) {
  const bool masked = threshold > 0;
  return refused(kPatternRefusal, who, opt, W, H, pat->grid, threshold, masked,
                 [&](int) { return rc_pattern_check(pat); }, [&](int) {
                   if (rc::pattern_supported(W, H, pat->grid, pat->nsamples, masked)) return 0;
                   return say("Error: %s: %d x %d is too large for %d samples a pixel (at most "
                              "65535 rows of tiles)\n", who, W, H, pat->nsamples);
                 });
}

// whatever the passes: `masked`: the call has a pass over the edge list, `dense`: one over every
// pixel
static int accum_refused(const char* who, const rc_options* opt, int W, int H,
                         const rc_sample_seq* seq, int threshold, bool dense, bool masked) {
  return refused(kAccumRefusal, who, opt, W, H, seq->grid, threshold, masked,
                 [&](int) { return rc_sample_seq_check(seq); }, [&](int) {
                   if ((!dense || rc::accum_supported(W, H, seq->grid, false)) &&
                       (!masked || rc::accum_supported(W, H, seq->grid, true)))
                     return 0;
                   return say("Error: %s: %d x %d is too large for the kernels' grids (at most "
                              "65535 rows of tiles)\n", who, W, H);
                 });
}

static int window_refused(const char* who, const rc_options* opt, int W, int H,
                          const rc_window* win) {
  return refused(kWindowRefusal, who, opt, W, H, 0, 0, false,
                 [&](int ss) { return rc_window_check(win, W, H, ss); }, no_check);
}

static const Refusal kGbufferRefusal = {
    "Error: %s: ssaa %d carries an adaptive threshold: a G-buffer holds one primary hit a pixel; "
    "the planes of the s x s image are a window of the s*full_w x s*full_h image\n",
    1, "Error: %s: ssaa %d in the options: a G-buffer of the s x s image is a window of the "
    "s*full_w x s*full_h image, leave ssaa at 0 or 1\n",
    nullptr,   // parity mode is accepted: the primary hit does not involve the carry
    "Error: %s: num_gpus %d: the row shards render no G-buffer\n",
    nullptr};   // rc_window_check tests the sizes

// frame: P or N is asked for.  image(): the entry's own test of its sizes (rc_window_check for the
// planes, the image's sides for pick), which prints its own message.
template <class Image>
static int gbuffer_refused(const char* who, const rc_options* opt, bool frame, Image image) {
  return refused(kGbufferRefusal, who, opt, 0, 0, 0, 0, false, [&](int) {
    if (frame && opt->mode == RC_MODE_CUDA)
      return say("Error: %s: the hit point and the normal (P, N, frame = 1) are for fast and parity "
                 "mode: no reference pins the CUDA port's hit frame; ask for id and t\n", who);
    return image();
  }, no_check);
}

static const Refusal kViewRefusal = {
    "Error: %s: ssaa %d carries an adaptive threshold: a view is shot at a plain factor\n",
    0, nullptr,
    "Error: %s: views are for fast and cuda mode: a parity image is defined by the scan-order "
    "carry of the reference's own camera\n",
    "Error: %s: num_gpus %d: the row shards take no view\n",
    nullptr};   // rc_window_check tests the sizes

static int view_refused(const char* who, const rc_options* opt, int W, int H, const rc_view* view,
                        const rc_window* vw) {
  return refused(kViewRefusal, who, opt, W, H, 0, 0, false, [&](int ss) {
    return rc_view_check(view) || rc_window_check(vw, W, H, ss);
  }, no_check);
}

static const Refusal kRaysRefusal = {
    "Error: %s: ssaa %d carries an adaptive threshold: a ray is one sample, leave ssaa at 0 or 1\n",
    1, "Error: %s: ssaa %d in the options: a ray is one sample, leave ssaa at 0 or 1\n",
    "Error: %s: ray batches are for fast and cuda mode: a parity colour is defined by the "
    "scan-order carry of the reference's own camera\n",
    "Error: %s: num_gpus %d: the row shards trace no ray batch\n",
    nullptr};

static int rays_refused(const char* who, const rc_options* opt, int64_t n, const rc_ray_out* out) {
  return refused(kRaysRefusal, who, opt, 0, 0, 0, 0, false, [&](int) {
    if (out->frame && out->hits && opt->mode == RC_MODE_CUDA)
      return say("Error: %s: the hit point and the normal (frame = 1) are for fast mode: no "
                 "reference pins the CUDA port's hit frame; ask for id and t\n", who);
    if (n < 1 || n > ((int64_t)1 << 24))
      return say("Error: %s: n %lld is not 1 .. 2^24 rays\n", who, (long long)n);
    return 0;
  }, no_check);
}

// The camera family is the view family in fast mode alone: the tables' mode clause refuses parity,
// and cuda mode is the first thing the family's own check refuses.
static int camera_mode_refused(const char* who, const rc_options* opt) {
  if (opt->mode == RC_MODE_FAST) return 0;
  return say("Error: %s: rays with an origin are for fast mode: the oracle exports no hit frame "
             "for the CUDA port, so no reference pins a colour there\n", who);
}

static const Refusal kCameraRefusal = {
    "Error: %s: ssaa %d carries an adaptive threshold: a camera frame is shot at a plain factor\n",
    0, nullptr,
    "Error: %s: cameras are for fast mode: a parity image is defined by the scan-order carry of "
    "the reference's own camera\n",
    "Error: %s: num_gpus %d: the row shards take no camera\n",
    nullptr};   // rc_window_check tests the sizes

static int camera_refused(const char* who, const rc_options* opt, int W, int H,
                          const rc_camera* cam, const rc_window* vw) {
  return refused(kCameraRefusal, who, opt, W, H, 0, 0, false, [&](int ss) {
    return camera_mode_refused(who, opt) || rc_camera_check(cam) ||
           rc_window_check(vw, W, H, ss);
  }, no_check);
}

// Accumulation through a camera: the accumulation family's clauses in the camera family's mode
// (parity by the table, cuda first in the check, then the sequence).
static const Refusal kCameraAccumRefusal = {
    nullptr,
    1, "Error: %s: ssaa %d in the options: the sample sequence carries the grid, leave ssaa at 0 "
    "or 1\n",
    "Error: %s: accumulated samples through a camera are for fast mode: every pixel of a parity "
    "image depends on the scan-order carry of the reference's own camera\n",
    "Error: %s: num_gpus %d: the row shards take no accumulator\n",
    kLatticeSide};

static int camera_accum_refused(const char* who, const rc_options* opt, int W, int H,
                                const rc_sample_seq* seq, int threshold, bool dense, bool masked) {
  return refused(kCameraAccumRefusal, who, opt, W, H, seq->grid, threshold, masked,
                 [&](int) { return camera_mode_refused(who, opt) || rc_sample_seq_check(seq); },
                 [&](int) {
                   if ((!dense || rc::accum_supported(W, H, seq->grid, false)) &&
                       (!masked || rc::accum_supported(W, H, seq->grid, true)))
                     return 0;
                   return say("Error: %s: %d x %d is too large for the kernels' grids (at most "
                              "65535 rows of tiles)\n", who, W, H);
                 });
}

// The last two clauses of the pair: the number of cameras (`per`: the pass's count, the host
// form's nsamples), then the first camera rc_camera_check would refuse, named by its index.
static int cameras_refused(const char* who, const rc_camera* cams, int ncams, int per,
                           const char* per_name) {
  if (ncams != 1 && ncams != per)
    return say("Error: %s: ncams %d is not 1 or %s (%d): one camera for all the samples, or one "
               "for each\n", who, ncams, per_name, per);
  for (int j = 0; j < ncams; ++j) {
    for (int k = 0; k < 3; ++k)
      if (!__builtin_isfinite(cams[j].eye[k]))
        return say("Error: %s: cams[%d] fails rc_camera_check: eye[%d] is not finite\n", who, j,
                   k);
    for (int k = 0; k < 9; ++k)
      if (!__builtin_isfinite(cams[j].view.m[k]))
        return say("Error: %s: cams[%d] fails rc_camera_check: view.m[%d] (row %d, column %d) is "
                   "not finite\n", who, j, k, k / 3, k % 3);
  }
  return 0;
}

static const Refusal kRaysFromRefusal = {
    "Error: %s: ssaa %d carries an adaptive threshold: a ray is one sample, leave ssaa at 0 or 1\n",
    1, "Error: %s: ssaa %d in the options: a ray is one sample, leave ssaa at 0 or 1\n",
    "Error: %s: rays with an origin are for fast mode: a parity colour is defined by the "
    "scan-order carry of the reference's own camera\n",
    "Error: %s: num_gpus %d: the row shards trace no ray batch\n",
    nullptr};

static int rays_from_refused(const char* who, const rc_options* opt, int64_t n) {
  return refused(kRaysFromRefusal, who, opt, 0, 0, 0, 0, false, [&](int) {
    if (camera_mode_refused(who, opt)) return -1;
    if (n < 1 || n > ((int64_t)1 << 24))
      return say("Error: %s: n %lld is not 1 .. 2^24 rays\n", who, (long long)n);
    return 0;
  }, no_check);
}

static int rates_refused(const char* who, const rc_options* opt, int W, int H) {
  return refused(kRatesRefusal, who, opt, W, H, 0, 0, false, [&](int) {
    if (rc::rates_supported(W, H)) return 0;
    return say("Error: %s: %d x %d is too large for a rate map (32-bit pixel indices at 8 "
               "subsamples a side, at most 65535 rows of tiles)\n", who, W, H);
  }, no_check);
}

// Any-hit visibility and ambient occlusion: the camera family's mode clauses in their order
// (parity, num_gpus, cuda), what the entry tests of its sizes in between (image(): rc_window_check
// for a pass, nothing for a ray batch), then the options' ssaa, which is not decoded: anything but
// 0 and 1 is refused in one clause, behind the sizes.  The table's other fields stay unused.
static const Refusal kAoRefusal = {
    nullptr,
    1, "Error: %s: ssaa %d in the options: an occlusion query has one primary ray a pixel and one "
    "sample a ray, leave ssaa at 0 or 1\n",
    "Error: %s: occlusion queries are for fast mode: a parity image is defined by the scan-order "
    "carry of the reference's own camera\n",
    "Error: %s: num_gpus %d: the row shards answer no occlusion query\n",
    nullptr};   // rc_window_check tests the sizes

template <class Image>
static int one_ray_refused(const Refusal& d, const char* who, const rc_options* opt, Image image) {
  if (opt->mode != RC_MODE_FAST && opt->mode != RC_MODE_CUDA) return say(d.mode, who);
  if (opt->num_gpus > 1) return say(d.shards, who, opt->num_gpus);
  if (camera_mode_refused(who, opt) || image()) return -1;
  if (d.factor && opt->ssaa != 0 && opt->ssaa != 1) return say(d.factor, who, opt->ssaa);
  return 0;
}

template <class Image>
static int ao_refused(const char* who, const rc_options* opt, Image image) {
  return one_ray_refused(kAoRefusal, who, opt, image);
}

// What rc_ao_dirs_check refuses of a non-null set, as words for the caller's message; null: the
// set passes.
static const char* ao_dirs_problem(const rc_ao_dirs* d, char* buf, size_t room) {
  if (d->n < 1 || d->n > RC_AO_MAX_DIRS) {
    std::snprintf(buf, room, "n %d is not 1..%d", d->n, RC_AO_MAX_DIRS);
    return buf;
  }
  if (!(d->tmax > 0.0f)) {   // NaN included
    std::snprintf(buf, room, "tmax %g is not in (0, +inf]", (double)d->tmax);
    return buf;
  }
  for (int j = 0; j < d->n; ++j) {
    const float* u = d->u[j];
    for (int k = 0; k < 3; ++k)
      if (!__builtin_isfinite(u[k])) {
        std::snprintf(buf, room, "u[%d][%d] is not finite", j, k);
        return buf;
      }
    if (u[0] == 0.0f && u[1] == 0.0f && u[2] == 0.0f) {
      std::snprintf(buf, room, "u[%d] is the zero vector", j);
      return buf;
    }
  }
  return nullptr;
}

// The guided family.  The G-buffer through a camera: the occlusion pass's
// clauses without its state and directions, in one_ray_refused's order.  The compose: the mode
// clauses alone (it shoots nothing, so the options' ssaa is not looked at).
static const Refusal kCameraGbufferRefusal = {
    nullptr,
    1, "Error: %s: ssaa %d in the options: a G-buffer holds one primary hit a pixel, leave ssaa at "
    "0 or 1\n",
    "Error: %s: a G-buffer through a camera is for fast mode: the reference has one camera, and "
    "rc_render_gbuffer gives its planes in parity mode\n",
    "Error: %s: num_gpus %d: the row shards render no G-buffer\n",
    nullptr};   // rc_window_check tests the sizes

static const Refusal kComposeRefusal = {
    nullptr,
    1, nullptr,
    "Error: %s: the ambient term is for fast mode: the reference's shading has none, so no parity "
    "image carries one\n",
    "Error: %s: num_gpus %d: the row shards compose nothing\n",
    nullptr};

// What rc_ao_filter_check refuses of a non-null filter, as words for the caller's message; null:
// the filter passes.
static const char* ao_filter_problem(const rc_ao_filter* f, char* buf, size_t room) {
  if (f->radius < 0 || f->radius > RC_AO_FILTER_MAX_RADIUS) {
    std::snprintf(buf, room, "radius %d is not 0..%d", f->radius, RC_AO_FILTER_MAX_RADIUS);
    return buf;
  }
  if (f->pad != 0) {
    std::snprintf(buf, room, "pad %u is not 0", (unsigned)f->pad);
    return buf;
  }
  if (f->taps[0] == 0) return "taps[0] is 0: the centre is always pooled";
  unsigned long long sum = f->taps[0];
  for (int d = 1; d <= f->radius; ++d) sum += 2ull * f->taps[d];
  if (sum * sum > 32768ull) {
    std::snprintf(buf, room, "the taps sum to %llu along a side and %llu over the window, more "
                  "than 32768: the sums are 32-bit", sum, sum * sum);
    return buf;
  }
  if (f->nmin != f->nmin) return "nmin is NaN";
  if (!(f->dplane >= 0.0f)) {   // NaN included
    std::snprintf(buf, room, "dplane %g is NaN or negative", (double)f->dplane);
    return buf;
  }
  return nullptr;
}

// both sides at least 1 and the image within one grid of 16 x 16 tiles (and, one lane a pixel,
// within 2^31 - 1 workgroups of 256)
static int guided_image_refused(const char* who, int W, int H) {
  if (W >= 1 && H >= 1 && W <= rc::kGuidedMaxSide && H <= rc::kGuidedMaxSide &&
      ((unsigned long long)W * (unsigned long long)H + 255) / 256 <= 0x7fffffffull)
    return 0;
  if (W < 1 || H < 1)
    return say("Error: %s: %d x %d: both sides must be at least 1\n", who, W, H);
  return say("Error: %s: %d x %d is past one grid: sides up to %d (16 x 16 tiles) and 2^39 pixels "
             "at most\n", who, W, H, rc::kGuidedMaxSide);
}

// ------------------------------------------- sample lattices: patterns and sequences --
// (x, y) pairs, x to the right and y downwards (include/raycast_hip.h, rc_pattern)
static const struct {
  const char* name;
  int grid, nsamples;
  uint8_t xy[RC_PATTERN_MAX_SAMPLES][2];
} kPatterns[] = {
    {"diag2", 2, 2, {{0, 0}, {1, 1}}},
    {"rgss4", 4, 4, {{1, 0}, {3, 1}, {0, 2}, {2, 3}}},
    {"checker8", 4, 8, {{0, 0}, {2, 0}, {1, 1}, {3, 1}, {0, 2}, {2, 2}, {1, 3}, {3, 3}}},
    {"queens8", 8, 8, {{3, 0}, {6, 1}, {2, 2}, {7, 3}, {1, 4}, {4, 5}, {0, 6}, {5, 7}}},
};

// The built-in pattern `name` into an rc_pattern or an rc_sample_seq (the same four fields);
// -1 and `out` as it was: no such pattern.
template <class Lattice>
static int builtin_pattern(const char* name, Lattice* out) {
  for (const auto& p : kPatterns) {
    if (std::strcmp(name, p.name)) continue;
    std::memset(out, 0, sizeof *out);
    out->grid = p.grid;
    out->nsamples = p.nsamples;
    for (int k = 0; k < p.nsamples; ++k) {
      out->x[k] = p.xy[k][0];
      out->y[k] = p.xy[k][1];
    }
    return 0;
  }
  return -1;
}

// The rules an rc_pattern and an rc_sample_seq share: the lattice g is 2, 4 or 8, the count n
// passes the type's own rule (count_refused(g, n) says why not), every point lies on the lattice
// and no two coincide.
template <class Rule>
static int lattice_check(const char* who, int g, int n, const uint8_t* x, const uint8_t* y,
                         Rule count_refused) {
  if (g != 2 && g != 4 && g != 8) return say("Error: %s: grid %d is not 2, 4 or 8\n", who, g);
  if (count_refused(g, n)) return -1;
  for (int k = 0; k < n; ++k) {
    if (x[k] >= g || y[k] >= g)
      return say("Error: %s: sample %d at (%d, %d) is off the %d x %d lattice\n", who, k, x[k],
                 y[k], g, g);
    for (int j = 0; j < k; ++j)
      if (x[j] == x[k] && y[j] == y[k])
        return say("Error: %s: samples %d and %d are both at (%d, %d)\n", who, j, k, x[k], y[k]);
  }
  return 0;
}

extern "C" {

// ------------------------ getters: adaptive supersampling, rate maps, two-pass frames --
int rc_adaptive_stats_get(rc_adaptive_stats* out) {
  Entered e;
  if (!out || enter(kCurrentDevice, false, e) || !e.c->aa.valid) return -1;
  const ListFrame& f = e.c->aa;
  if (list_frame_refined(f, &out->refined_pixels)) return -1;
  out->rays = (int64_t)f.pixels + (int64_t)f.rays * out->refined_pixels;
  return 0;
}

int rc_adaptive_phase_ms(double ms[3]) {
  Entered e;
  if (!ms || enter(kCurrentDevice, false, e)) return -1;
  hipEvent_t* ev = e.c->span_ev[kSpanAdaptive];
  return ev ? read_spans({ev[0], ev[2], ev[3], ev[1]}, ms) : -1;
}

int rc_rate_stats_get(rc_rate_stats* out) {
  Entered e;
  if (!out || enter(kCurrentDevice, false, e) || !e.c->rates.valid) return -1;
  HIP_TRY(hipEventSynchronize(e.c->rates.done));   // the frame's stream, up to its refinement
  unsigned n[5] = {0, 0, 0, 0, 0};   // launch_rates_render's counter block
  HIP_TRY(hipMemcpy(n, e.c->rates.count.p, sizeof n, hipMemcpyDeviceToHost));
  out->pixels[0] = (int64_t)n[3];
  out->pixels[1] = (int64_t)n[0];
  out->pixels[2] = (int64_t)n[1];
  out->pixels[3] = (int64_t)n[2];
  out->invalid = (int64_t)n[4];
  out->rays = out->pixels[0] + 4 * out->pixels[1] + 16 * out->pixels[2] + 64 * out->pixels[3];
  return 0;
}

int rc_rate_phase_ms(double ms[2]) {
  Entered e;
  if (!ms || enter(kCurrentDevice, false, e)) return -1;
  hipEvent_t* ev = e.c->span_ev[kSpanRates];
  return ev ? read_spans({ev[0], ev[2], ev[1]}, ms) : -1;
}

int rc_filter_phase_ms(double ms[2]) {
  Entered e;
  if (!ms || enter(kCurrentDevice, false, e)) return -1;
  hipEvent_t* ev = e.c->span_ev[kSpanFilter];
  return ev ? read_spans({ev[0], e.c->filt.mid, ev[e.c->filt.end]}, ms) : -1;
}

// ---------------------------------------------------------- reconstruction filters --
static bool filter_factor(int s) { return s == 2 || s == 4 || s == 8; }

int rc_filter_box(int s, rc_filter* out) {
  if (!out || !filter_factor(s)) return -1;
  std::memset(out, 0, sizeof *out);
  out->ntaps = s;
  for (int i = 0; i < s; ++i) out->taps[i] = 1;
  return 0;
}

int rc_filter_tent(int s, rc_filter* out) {
  if (!out || !filter_factor(s)) return -1;
  std::memset(out, 0, sizeof *out);
  out->ntaps = 2 * s;
  for (int i = 0; i < s; ++i) out->taps[i] = out->taps[2 * s - 1 - i] = (int16_t)(2 * i + 1);
  return 0;
}

// The rules of include/raycast_hip.h (rc_filter).  The bound on the absolute sum is what keeps
// the kernel's arithmetic in int32: a horizontal sum is at most 2048 * 255 < 2^19 in magnitude,
// the full sum at most 2048^2 * 255, and with the rounding term S*S/2 <= 2^21 that stays below
// 2^31, so the separable evaluation is exact.
int rc_filter_check(const rc_filter* f, int s) {
  const char* who = "rc_filter_check";
  if (!f) return say("Error: %s: a null filter\n", who);
  if (!filter_factor(s)) return say("Error: %s: factor %d is not 2, 4 or 8\n", who, s);
  const int n = f->ntaps;
  if (n > RC_FILTER_MAX_TAPS)
    return say("Error: %s: %d taps, at most %d\n", who, n, RC_FILTER_MAX_TAPS);
  if (n < s || ((n - s) & 1))
    return say("Error: %s: %d taps at factor %d: the count is s + 2h with a halo h >= 0, so it is "
               "at least s and differs from s by an even number\n", who, n, s);
  if ((n - s) / 2 > s)
    return say("Error: %s: %d taps at factor %d: the halo %d is wider than one output pixel "
               "(h <= s, at most %d taps)\n", who, n, s, (n - s) / 2, 3 * s);
  long long sum = 0, mag = 0;
  for (int i = 0; i < n; ++i) {
    sum += f->taps[i];
    mag += f->taps[i] < 0 ? -(long long)f->taps[i] : f->taps[i];
  }
  if (sum <= 0)
    return say("Error: %s: the taps sum to %lld, the sum must be positive\n", who, sum);
  if (mag > 2048)
    return say("Error: %s: the taps' absolute values sum to %lld, at most 2048 (the int32 "
               "bound)\n", who, mag);
  return 0;
}

int rc_filter_env(const rc_options* opt, rc_filter* out) {
  const char* v = std::getenv("RAYCAST_FILTER");
  if (!v || !opt || !out) return 0;
  bool tent = false;
  if (!std::strcmp(v, "tent")) tent = true;
  else if (std::strcmp(v, "box"))
    std::fprintf(stderr, "Warning: RAYCAST_FILTER '%s' is not box or tent, using box\n", v);
  const int s = RC_SSAA_FACTOR(opt->ssaa);
  if (!filter_factor(s))
    return warn("Warning: RAYCAST_FILTER '%s' needs RAYCAST_SSAA 2, 4 or 8, ignored\n", v);
  if (RC_SSAA_THRESHOLD(opt->ssaa) > 0)
    return warn("Warning: RAYCAST_FILTER '%s' does not combine with RAYCAST_SSAA_ADAPTIVE (a "
                "refined pixel's footprint would reach its unrefined neighbours), ignored\n", v);
  return tent && rc_filter_tent(s, out) == 0 ? 1 : 0;
}

// ------------------------------------------------------------ sparse sample patterns --
int rc_pattern_stats_get(rc_pattern_stats* out) {
  Entered e;
  if (!out || enter(kCurrentDevice, false, e) || !e.c->pat.valid) return -1;
  const PatternFrame& f = e.c->pat;
  const bool listed = f.threshold > 0;
  int64_t refined = (int64_t)f.pixels;   // without a threshold: known without the device
  if (listed && list_frame_refined(f, &refined)) return -1;
  out->refined_pixels = refined;
  out->rays = (listed ? (int64_t)f.pixels : 0) + (int64_t)f.rays * refined;
  return 0;
}

int rc_pattern_phase_ms(double ms[3]) {
  Entered e;
  if (!ms || enter(kCurrentDevice, false, e)) return -1;
  hipEvent_t* ev = e.c->span_ev[kSpanPattern];
  if (!ev) return -1;
  if (e.c->pat.ev_listed) return read_spans({ev[0], ev[2], ev[3], ev[1]}, ms);
  ms[1] = ms[2] = 0.0;
  return read_spans({ev[0], ev[1]}, ms);
}

int rc_pattern_builtin(const char* name, rc_pattern* out) {
  return name && out ? builtin_pattern(name, out) : -1;
}

int rc_pattern_check(const rc_pattern* p) {
  const char* who = "rc_pattern_check";
  if (!p) return say("Error: %s: a null pattern\n", who);
  return lattice_check(who, p->grid, p->nsamples, p->x, p->y, [&](int g, int n) {
    if (n != 2 && n != 4 && n != 8 && n != 16)
      return say("Error: %s: %d samples, not 2, 4, 8 or 16\n", who, n);
    if (n > g * g)
      return say("Error: %s: %d samples on a %d x %d lattice of %d points\n", who, n, g, g, g * g);
    return 0;
  });
}

int rc_pattern_env(const rc_options* opt, rc_pattern* out, int* threshold) {
  const char* v = std::getenv("RAYCAST_PATTERN");
  if (!v || !opt || !out || !threshold) return 0;
  const char* colon = std::strchr(v, ':');
  const std::string name = colon ? std::string(v, colon) : std::string(v);
  rc_pattern pat;
  if (rc_pattern_builtin(name.c_str(), &pat))
    return warn("Warning: RAYCAST_PATTERN '%s': '%s' is not diag2, rgss4, checker8 or queens8, "
                "ignored\n", v, name.c_str());
  long t = 0;
  if (colon) {
    char* end = nullptr;
    t = std::strtol(colon + 1, &end, 10);
    if (colon[1] < '0' || colon[1] > '9' || *end != '\0' || t > 255)
      return warn("Warning: RAYCAST_PATTERN '%s': '%s' is not a threshold 0..255, ignored\n", v,
                  colon + 1);
  }
  if (opt->mode != RC_MODE_FAST && opt->mode != RC_MODE_CUDA)
    return warn("Warning: RAYCAST_PATTERN '%s' is for fast and cuda mode (a parity image cannot be "
                "shot sparsely), ignored\n", v);
  if (RC_SSAA_FACTOR(opt->ssaa) > 1 || RC_SSAA_THRESHOLD(opt->ssaa) > 0)
    return warn("Warning: RAYCAST_PATTERN '%s' does not combine with RAYCAST_SSAA %d (the pattern "
                "carries its own grid), ignored\n", v, RC_SSAA_FACTOR(opt->ssaa));
  *out = pat;
  *threshold = (int)t;
  return 1;
}

// ------------------------------------------------------- progressive supersampling --
int rc_accum_stats_get(rc_accum_stats* out) {
  Entered e;
  if (!out || enter(kCurrentDevice, false, e) || !e.c->acc.valid) return -1;
  const AccumFrame& f = e.c->acc;
  HIP_TRY(hipEventSynchronize(f.done));   // the call's stream, up to its last pass
  unsigned n[AccumFrame::kSlots][2] = {};   // per pass {listed, saturated}
  HIP_TRY(hipMemcpy(n, f.count.p, (size_t)f.passes * sizeof n[0], hipMemcpyDeviceToHost));
  std::memset(out, 0, sizeof *out);   // a call without a pass (a scroll that exposes nothing)
  out->passes = f.passes;
  for (int k = 0; k < f.passes; ++k) {
    out->active_pixels = f.listed[k] ? (int64_t)n[k][0] : (int64_t)f.pixels;
    out->saturated = (int64_t)n[k][1];
    out->rays += (out->active_pixels - out->saturated) * f.samples[k];
  }
  return 0;
}

int rc_accum_phase_ms(double ms[2]) {
  Entered e;
  if (!ms || enter(kCurrentDevice, false, e)) return -1;
  hipEvent_t* ev = e.c->span_ev[kSpanAccum];
  if (!ev) return -1;
  hipEvent_t first = ev[e.c->acc.ev_first];
  if (e.c->acc.ev_listed) return read_spans({first, ev[3], ev[1]}, ms);
  ms[0] = 0.0;
  return read_spans({first, ev[1]}, ms + 1);
}

// hier<g>: point k is the bit-reversal r of k over 2 * lg bits; x takes r's even bits, y its odd
// bits (include/raycast_hip.h, rc_sample_seq)
static void hier_seq(int lg, rc_sample_seq* out) {
  out->grid = 1 << lg;
  out->nsamples = 1 << (2 * lg);
  for (int k = 0; k < out->nsamples; ++k) {
    int r = 0;
    for (int b = 0; b < 2 * lg; ++b) r |= ((k >> b) & 1) << (2 * lg - 1 - b);
    int x = 0, y = 0;
    for (int i = 0; i < lg; ++i) {
      x |= ((r >> (2 * i)) & 1) << i;
      y |= ((r >> (2 * i + 1)) & 1) << i;
    }
    out->x[k] = (uint8_t)x;
    out->y[k] = (uint8_t)y;
  }
}

int rc_sample_seq_builtin(const char* name, rc_sample_seq* out) {
  if (!name || !out) return -1;
  std::memset(out, 0, sizeof *out);
  for (int lg = 1; lg <= 3; ++lg) {
    const char hier[] = {'h', 'i', 'e', 'r', (char)('0' + (1 << lg)), '\0'};
    if (std::strcmp(name, hier)) continue;
    hier_seq(lg, out);
    return 0;
  }
  return builtin_pattern(name, out);
}

int rc_sample_seq_check(const rc_sample_seq* s) {
  const char* who = "rc_sample_seq_check";
  if (!s) return say("Error: %s: a null sequence\n", who);
  return lattice_check(who, s->grid, s->nsamples, s->x, s->y, [&](int g, int n) {
    const int most = g * g < RC_ACCUM_MAX_SAMPLES ? g * g : RC_ACCUM_MAX_SAMPLES;
    if (n >= 1 && n <= most) return 0;
    return say("Error: %s: %d samples, not 1..%d (a %d x %d lattice, at most %d)\n", who, n, most,
               g, g, RC_ACCUM_MAX_SAMPLES);
  });
}

// ------------------------------------------------------- windows of a virtual image --
int rc_window_check(const rc_window* w, int W, int H, int s) {
  const char* who = "rc_window_check";
  if (!w) return say("Error: %s: a null window\n", who);
  if (s == 0) s = 1;   // as rc_options.ssaa
  if (s != 1 && s != 2 && s != 4 && s != 8)
    return say("Error: %s: factor %d is not 0, 1, 2, 4 or 8\n", who, s);
  if (w->full_w < 1 || w->full_h < 1 || W < 1 || H < 1)
    return say("Error: %s: a %d x %d window of a %d x %d image: every size must be at least 1\n",
               who, W, H, w->full_w, w->full_h);
  if (w->x0 < 0 || w->y0 < 0)
    return say("Error: %s: origin (%d, %d): a window starts inside the image, at 0 or above\n",
               who, w->x0, w->y0);
  // W > full_w - x0 rather than x0 + W > full_w: no sum that could overflow
  if (w->x0 > w->full_w || W > w->full_w - w->x0 || w->y0 > w->full_h || H > w->full_h - w->y0)
    return say("Error: %s: a %d x %d window at (%d, %d) reaches outside the %d x %d image\n", who,
               W, H, w->x0, w->y0, w->full_w, w->full_h);
  if (w->full_w > 0x7fffffff / s || w->full_h > 0x7fffffff / s)
    return say("Error: %s: %d times %d x %d: the subsample image's sides must stay within 2^31 - "
               "1\n", who, s, w->full_w, w->full_h);
  if (!rc::window_supported(rc::Window{w->full_w, w->full_h, w->x0, w->y0}, W, H, s))
    return say("Error: %s: a %d x %d window at factor %d is too large for the kernel's grid (at "
               "most 65535 rows of 16-subsample tiles, 2^31 - 1 tiles)\n", who, W, H, s);
  return 0;
}

// one decimal field of RAYCAST_WINDOW: digits only, within int; *p moves behind it
static bool window_field(const char** p, int* out) {
  const char* q = *p;
  long long v = 0;
  if (*q < '0' || *q > '9') return false;
  for (; *q >= '0' && *q <= '9'; ++q) {
    v = v * 10 + (*q - '0');
    if (v > 0x7fffffffll) return false;
  }
  *p = q;
  *out = (int)v;
  return true;
}

int rc_window_env(const rc_options* opt, int W, int H, rc_window* out) {
  const char* v = std::getenv("RAYCAST_WINDOW");
  if (!v || !opt || !out) return 0;
  rc_window w;
  const char* p = v;
  int f[4] = {0, 0, 0, 0};
  bool ok = window_field(&p, &f[0]);
  const char seps[3] = {'x', '+', '+'};
  for (int k = 0; ok && k < 3; ++k) ok = *p++ == seps[k] && window_field(&p, &f[k + 1]);
  if (!ok || *p != '\0')
    return warn("Warning: RAYCAST_WINDOW '%s' is not FWxFH+X0+Y0 (four decimal numbers), "
                "ignored\n", v);
  w.full_w = f[0], w.full_h = f[1], w.x0 = f[2], w.y0 = f[3];
  if (opt->mode != RC_MODE_FAST && opt->mode != RC_MODE_CUDA)
    return warn("Warning: RAYCAST_WINDOW '%s' is for fast and cuda mode (a window of a parity "
                "image depends on the scan-order carry of every pixel before it), ignored\n", v);
  if (RC_SSAA_THRESHOLD(opt->ssaa) > 0)
    return warn("Warning: RAYCAST_WINDOW '%s' does not combine with RAYCAST_SSAA_ADAPTIVE, "
                "ignored\n", v);
  const char* pat = std::getenv("RAYCAST_PATTERN");
  if (pat && pat[0])
    return warn("Warning: RAYCAST_WINDOW '%s' does not combine with RAYCAST_PATTERN, ignored\n",
                v);
  const char* filt = std::getenv("RAYCAST_FILTER");
  if (filt && !std::strcmp(filt, "tent"))
    return warn("Warning: RAYCAST_WINDOW '%s' does not combine with RAYCAST_FILTER=tent, "
                "ignored\n", v);
  if (opt->num_gpus > 1)
    return warn("Warning: RAYCAST_WINDOW '%s' does not combine with RAYCAST_GPUS %d (the row "
                "shards take no window), ignored\n", v, opt->num_gpus);
  if (rc_window_check(&w, W, H, RC_SSAA_FACTOR(opt->ssaa)))
    return warn("Warning: RAYCAST_WINDOW '%s' does not hold a %d x %d window, ignored\n", v, W, H);
  *out = w;
  return 1;
}

// ------------------------------------------------------------- rotated camera views --
int rc_view_check(const rc_view* v) {
  const char* who = "rc_view_check";
  if (!v) return say("Error: %s: a null view\n", who);
  for (int k = 0; k < 9; ++k)
    if (!__builtin_isfinite(v->m[k]))
      return say("Error: %s: m[%d] (row %d, column %d) is not finite\n", who, k, k / 3, k % 3);
  return 0;
}

int rc_camera_check(const rc_camera* cam) {
  const char* who = "rc_camera_check";
  if (!cam) return say("Error: %s: a null camera\n", who);
  for (int k = 0; k < 3; ++k)
    if (!__builtin_isfinite(cam->eye[k]))
      return say("Error: %s: eye[%d] is not finite\n", who, k);
  return rc_view_check(&cam->view);
}

}  // extern "C"

// ------------------------------------------------------------------ enqueue bodies --
// The first and the last lines of a sampling frame's body inside ws_frame.  begin: the scene, the
// zero-normalize counter and the feature's own counters (bytes of *counters, 0: none) zeroed on
// the stream, then the event set is claimed for `owner` and ev[0] recorded.  end: ev[1] recorded
// and the set stored as the owner's.  What a feature records around ev[1] (RateFrame::done before
// it, the pattern's and the accumulation's `done` behind it) and its record's flags stay in its
// body, the flags behind end().
struct SampleFrame {
  DevCtx& c;
  hipStream_t stream;
  SpanOwner owner;
  rc::LaunchScene ls;
  unsigned long long* zc = nullptr;
  hipEvent_t* ev = nullptr;

  int begin(const rc_scene* s, const DevBuf* counters, size_t bytes) {
    if (upload_scene(c.fb, stream, s, ls)) return -1;
    zc = (unsigned long long*)c.fb.zcount.p;
    HIP_TRY(hipMemsetAsync(zc, 0, sizeof(unsigned long long), stream));
    if (bytes) HIP_TRY(hipMemsetAsync(counters->p, 0, bytes, stream));
    ev = claim_event_set(c, owner, false, true);
    HIP_TRY(hipEventRecord(ev[0], stream));
    return 0;
  }
  int end() {
    HIP_TRY(hipEventRecord(ev[1], stream));
    c.span_ev[owner] = ev;
    return 0;
  }
};

// a record's `done` event, created on first use
static int ensure_done(hipEvent_t& done) {
  if (!done) HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
  return 0;
}

// One rate-map frame on `stream` through the device's one-frame workspace (the caller holds
// c.mu and has passed rates_refused): the rate-1 pixels with the binning, then the three lists'
// refinements, with no host wait in between.  The host does not know which lists are empty, so
// all three are launched.
static int enqueue_rates(DevCtx& c, const rc_scene* s, int W, int H, const rc_options* opt,
                         const uint8_t* d_rates, uint8_t* d_out, hipStream_t stream) {
  RateFrame& r = c.rates;
  auto prepare = [&]() -> int {
    const size_t entries = (size_t)W * H;
    if (c.aa_list.ensure(entries * sizeof(uint32_t)) ||
        r.list.ensure(entries * sizeof(uint32_t)) || r.count.ensure(32)) {
      std::fprintf(stderr, "Error: out of device memory for the rate lists (%d x %d)\n", W, H);
      return -1;
    }
    return ensure_done(r.done);
  };
  return ws_frame(c, stream, prepare, [&]() -> int {
    SampleFrame f{c, stream, kSpanRates};
    if (f.begin(s, &r.count, 32)) return -1;
    unsigned* cnt = (unsigned*)r.count.p;
    uint32_t* list4 = (uint32_t*)c.aa_list.p;
    uint32_t* list28 = (uint32_t*)r.list.p;
    const int maxrec = opt->max_recursion;
    const bool cuda = opt->mode == RC_MODE_CUDA;
    // The lists follow the map's row-major order, so over a uniform region entry k is pixel
    // k + const and a wave's static stride (workgroups * 4 waves * pixels per step) that is a
    // multiple of W keeps the wave in one column of the image: the waves whose column crosses
    // the expensive shapes finish last.  An odd number of workgroups makes the stride drift
    // through the columns (measured: DESIGN.md section 12).  An explicit adaptive_blocks holds.
    const int want = tune().adaptive_blocks;
    auto blocks = [&](int ss) {
      const int b = rc::aa_refine_blocks(W, H, ss, c.cus, want);
      return want <= 0 && b > 2 && (b & 1) == 0 ? b - 1 : b;
    };
    HIP_TRY(rc::launch_rates_render(f.ls, W, H, maxrec, d_rates, d_out, list4, list28, cnt, f.zc,
                                    stream, cuda));
    HIP_TRY(hipEventRecord(f.ev[2], stream));
    HIP_TRY(rc::launch_aa_refine(f.ls, W, H, 2, maxrec, list28, cnt, d_out, f.zc, blocks(2),
                                 stream, cuda));
    HIP_TRY(rc::launch_aa_refine(f.ls, W, H, 4, maxrec, list4, cnt + 1, d_out, f.zc, blocks(4),
                                 stream, cuda));
    HIP_TRY(rc::launch_rates_refine8(f.ls, W, H, maxrec, list28, cnt + 2, d_out, f.zc, blocks(8),
                                     stream, cuda));
    HIP_TRY(hipEventRecord(r.done, stream));
    if (f.end()) return -1;
    r.valid = true;
    return 0;
  });
}

// One pattern frame on `stream` through the device's one-frame workspace (the caller holds c.mu
// and has passed pattern_refused).  at = 0: the dense kernel.  at > 0: the one-ray image by the
// plain kernel, the adaptive path's edge list (launch_aa_mark into aa_list), then the pattern
// kernel over the list: three launches with no host wait in between.
static int enqueue_pattern(DevCtx& c, const rc_scene* s, int W, int H, const rc_options* opt,
                           const rc_pattern* pat, int at, uint8_t* d_out, hipStream_t stream) {
  PatternFrame& p = c.pat;
  auto prepare = [&]() -> int {
    if (at == 0) return 0;
    if (p.count.ensure(8) || c.aa_list.ensure((size_t)W * H * sizeof(uint32_t))) {
      std::fprintf(stderr, "Error: out of device memory for the edge list (%d x %d)\n", W, H);
      return -1;
    }
    return ensure_done(p.done);
  };
  return ws_frame(c, stream, prepare, [&]() -> int {
    SampleFrame f{c, stream, kSpanPattern};
    if (f.begin(s, &p.count, at > 0 ? 8 : 0)) return -1;
    unsigned* cnt = (unsigned*)p.count.p;
    uint32_t* list = (uint32_t*)c.aa_list.p;
    const int maxrec = opt->max_recursion, g = pat->grid, n = pat->nsamples;
    const bool cuda = opt->mode == RC_MODE_CUDA;
    if (at == 0) {
      HIP_TRY(rc::launch_pattern(f.ls, W, H, g, n, pat->x, pat->y, maxrec, d_out, f.zc, stream,
                                 cuda));
    } else {
      HIP_TRY(rc::launch_render(f.ls, W, H, 0, 1, H, maxrec, d_out, f.zc, stream, cuda));
      HIP_TRY(hipEventRecord(f.ev[2], stream));
      HIP_TRY(rc::launch_aa_mark(d_out, W, H, at, list, cnt, stream));
      HIP_TRY(hipEventRecord(f.ev[3], stream));
      HIP_TRY(rc::launch_pattern_list(
          f.ls, W, H, g, n, pat->x, pat->y, maxrec, list, cnt, d_out, f.zc,
          rc::pattern_list_blocks(W, H, n, c.cus, tune().adaptive_blocks), stream, cuda));
    }
    if (f.end()) return -1;
    // behind the span's end, and only where rc_pattern_stats_get has a count to wait for
    if (at > 0) HIP_TRY(hipEventRecord(p.done, stream));
    p.valid = true;
    p.rays = n;
    p.threshold = at;
    p.pixels = (long long)W * H;
    p.ev_listed = at > 0;
    return 0;
  });
}

// One pass of an accumulation call: samples [first, first + count) of the sequence, over every
// pixel (at = 0) or over the pixels whose contrast in `out` reaches at; reset: the records count
// as zero and are not read.
struct AccumPass {
  int first, count, at;
  bool reset;
};

// The passes of one accumulation call on `stream` through the device's one-frame workspace (the
// caller holds c.mu and has passed accum_refused and the range checks; at most
// AccumFrame::kSlots passes).  A pass over every pixel is one launch; a masked pass is the
// adaptive path's edge list (launch_aa_mark over d_out into aa_list) and the list kernel.
// Nothing waits for the host: pass k counts into slot k of the call's counter block.
// win (or null): the samples are those of this window of a virtual image (it has passed
// rc_window_check at the sequence's g); the edge list, the records and the image stay the
// window's own W x H.
static int enqueue_accum(DevCtx& c, const rc_scene* s, int W, int H, const rc_options* opt,
                         const rc_sample_seq* seq, const AccumPass* passes, int npasses,
                         rc_accum_px* d_acc, uint8_t* d_out, hipStream_t stream,
                         const rc_window* win = nullptr) {
  AccumFrame& a = c.acc;
  bool masked = false;
  for (int k = 0; k < npasses; ++k) masked = masked || passes[k].at > 0;
  auto prepare = [&]() -> int {
    if (a.count.ensure(AccumFrame::kSlots * 8) ||
        (masked && c.aa_list.ensure((size_t)W * H * sizeof(uint32_t)))) {
      std::fprintf(stderr, "Error: out of device memory for the edge list (%d x %d)\n", W, H);
      return -1;
    }
    return ensure_done(a.done);
  };
  return ws_frame(c, stream, prepare, [&]() -> int {
    a.valid = false;   // the block is this call's from here on
    SampleFrame f{c, stream, kSpanAccum};
    if (f.begin(s, &a.count, (size_t)npasses * 8)) return -1;
    unsigned* cnt = (unsigned*)a.count.p;
    uint32_t* list = (uint32_t*)c.aa_list.p;
    const int maxrec = opt->max_recursion, g = seq->grid;
    const bool cuda = opt->mode == RC_MODE_CUDA;
    const rc::Window vw = win ? rc::Window{win->full_w, win->full_h, win->x0, win->y0}
                              : rc::Window{W, H, 0, 0};
    for (int k = 0; k < npasses; ++k) {
      const AccumPass& p = passes[k];
      const bool last = k + 1 == npasses;
      if (last && k > 0) HIP_TRY(hipEventRecord(f.ev[2], stream));
      const uint8_t* px = seq->x + p.first;
      const uint8_t* py = seq->y + p.first;
      unsigned* slot = cnt + 2 * k;
      if (p.at == 0) {
        if (win)
          HIP_TRY(rc::launch_accum_window(f.ls, vw, W, H, g, p.count, px, py, p.reset, maxrec,
                                          d_acc, d_out, f.zc, slot + 1, stream, cuda));
        else
          HIP_TRY(rc::launch_accum(f.ls, W, H, g, p.count, px, py, p.reset, maxrec, d_acc, d_out,
                                   f.zc, slot + 1, stream, cuda));
      } else {
        HIP_TRY(rc::launch_aa_mark(d_out, W, H, p.at, list, slot, stream));
        if (last) HIP_TRY(hipEventRecord(f.ev[3], stream));
        const int blocks = rc::accum_list_blocks(W, H, c.cus, tune().adaptive_blocks);
        if (win)
          HIP_TRY(rc::launch_accum_list_window(f.ls, vw, W, H, g, p.count, px, py, maxrec, list,
                                               slot, d_acc, d_out, f.zc, slot + 1, blocks, stream,
                                               cuda));
        else
          HIP_TRY(rc::launch_accum_list(f.ls, W, H, g, p.count, px, py, maxrec, list, slot, d_acc,
                                        d_out, f.zc, slot + 1, blocks, stream, cuda));
      }
      a.samples[k] = (uint8_t)p.count;
      a.listed[k] = p.at > 0;
    }
    if (f.end()) return -1;
    HIP_TRY(hipEventRecord(a.done, stream));
    a.valid = true;
    a.passes = npasses;
    a.pixels = (long long)W * H;
    a.ev_first = npasses > 1 ? 2 : 0;
    a.ev_listed = passes[npasses - 1].at > 0;
    return 0;
  });
}

// One scroll on `stream` through the device's one-frame workspace (the caller holds c.mu and has
// passed rc_accum_scroll_device's refusals): the kept rectangle moved from the source state to the
// destination, then seq[0..count) for the exposed pixels in chunks of at most 16, the first one
// resetting; chunk k counts into slot k, nothing waits for the host.  The accumulation family's
// record and spans: ev[3] stands between the move and the samples, so rc_accum_phase_ms reads
// {move, samples} through its listed form.
static int enqueue_scroll(DevCtx& c, const rc_scene* s, const rc_window* win, int W, int H,
                          const rc_options* opt, const rc_sample_seq* seq, int count, int dx,
                          int dy, const rc_accum_px* d_acc_src, const uint8_t* d_out_src,
                          rc_accum_px* d_acc_dst, uint8_t* d_out_dst, hipStream_t stream) {
  AccumFrame& a = c.acc;
  const rc::ScrollRects r = rc::scroll_rects(W, H, dx, dy);
  const int chunks = r.total ? (count + 15) / 16 : 0;
  auto prepare = [&]() -> int {
    if (a.count.ensure(AccumFrame::kSlots * 8)) {
      std::fprintf(stderr, "Error: out of device memory for the pass counters\n");
      return -1;
    }
    return ensure_done(a.done);
  };
  return ws_frame(c, stream, prepare, [&]() -> int {
    a.valid = false;   // the block is this call's from here on
    SampleFrame f{c, stream, kSpanAccum};
    if (f.begin(s, &a.count, (size_t)chunks * 8)) return -1;
    const int g = seq->grid;
    if (r.kw > 0)
      HIP_TRY(rc::launch_accum_move(W, H, g, dx, dy, d_acc_src, d_out_src, d_acc_dst, d_out_dst,
                                    stream));
    HIP_TRY(hipEventRecord(f.ev[3], stream));
    const rc::Window vw{win->full_w, win->full_h, win->x0, win->y0};
    const int blocks = rc::accum_exposed_blocks(r.total, c.cus, tune().adaptive_blocks);
    for (int k = 0; k < chunks; ++k) {
      const int n = count - 16 * k < 16 ? count - 16 * k : 16;
      HIP_TRY(rc::launch_accum_exposed(f.ls, vw, W, H, g, dx, dy, n, seq->x + 16 * k,
                                       seq->y + 16 * k, k == 0, opt->max_recursion, d_acc_dst,
                                       d_out_dst, f.zc, blocks, stream,
                                       opt->mode == RC_MODE_CUDA));
      a.samples[k] = (uint8_t)n;
      a.listed[k] = false;
    }
    if (f.end()) return -1;
    HIP_TRY(hipEventRecord(a.done, stream));
    a.valid = true;
    a.passes = chunks;
    a.pixels = (long long)r.total;
    a.ev_first = 0;
    a.ev_listed = true;
    return 0;
  });
}

// One window frame on `stream` through the device's one-frame workspace (the caller holds c.mu
// and has passed window_refused): one launch of k_window at the options' factor.
static int enqueue_window(DevCtx& c, const rc_scene* s, const rc_window* win, int W, int H,
                          const rc_options* opt, uint8_t* d_out, hipStream_t stream) {
  return ws_frame(c, stream, [] { return 0; }, [&]() -> int {
    SampleFrame f{c, stream, kSpanWindow};
    if (f.begin(s, nullptr, 0)) return -1;
    HIP_TRY(rc::launch_window(f.ls, rc::Window{win->full_w, win->full_h, win->x0, win->y0}, W, H,
                              ssaa_factor(opt, "rc_render_window"), opt->max_recursion, d_out,
                              f.zc, stream, opt->mode == RC_MODE_CUDA));
    return f.end();
  });
}

// One G-buffer frame on `stream` through the device's one-frame workspace (the caller holds c.mu
// and has passed gbuffer_refused): one launch of k_gbuffer for the window's pixels (pts null) or of
// k_gbuffer_points for the n points.  It uses the workspace's scene and zero-normalize counter and
// no other feature's record.
struct GbufPoints {
  int frame;
  long long n;
  const int32_t* xy;
  rc_hit* hits;
};
static int enqueue_gbuffer(DevCtx& c, const rc_scene* s, const rc::Window& vw, int W, int H,
                           const rc_options* opt, const rc_gbuffer* planes, const GbufPoints* pts,
                           hipStream_t stream) {
  return ws_frame(c, stream, [] { return 0; }, [&]() -> int {
    SampleFrame f{c, stream, kSpanGbuffer};
    if (f.begin(s, nullptr, 0)) return -1;
    const bool cuda = opt->mode == RC_MODE_CUDA;
    if (pts)
      HIP_TRY(rc::launch_gbuffer_points(f.ls, vw.full_w, vw.full_h, pts->frame != 0, pts->n,
                                        pts->xy, pts->hits, f.zc, stream, cuda));
    else
      HIP_TRY(rc::launch_gbuffer(f.ls, vw, W, H, planes->id, planes->t, planes->P, planes->N, f.zc,
                                 stream, cuda));
    return f.end();
  });
}

// One view frame or one ray batch on `stream` through the device's one-frame workspace (the caller
// holds c.mu and has passed view_refused or rays_refused): one launch of k_view at the options'
// factor for the window's pixels (rays null), or of k_rays for the n directions.  It uses the
// workspace's scene and zero-normalize counter and no other feature's record.
struct RayBatch {
  long long n;
  const float* dirs;
  rc_ray_out out;
};
static int enqueue_view(DevCtx& c, const rc_scene* s, const rc_view* view, const rc_window* vw,
                        int W, int H, const rc_options* opt, uint8_t* d_out, const RayBatch* rays,
                        hipStream_t stream) {
  return ws_frame(c, stream, [] { return 0; }, [&]() -> int {
    SampleFrame f{c, stream, kSpanView};
    if (f.begin(s, nullptr, 0)) return -1;
    const bool cuda = opt->mode == RC_MODE_CUDA;
    if (rays) {
      HIP_TRY(rc::launch_rays(f.ls, rays->n, rays->dirs, opt->max_recursion, rays->out.rgb8,
                              rays->out.rgb, rays->out.hits, rays->out.frame != 0, f.zc, stream,
                              cuda));
    } else {
      rc::View v;
      std::memcpy(v.m, view->m, sizeof v.m);
      HIP_TRY(rc::launch_view(f.ls, v, rc::Window{vw->full_w, vw->full_h, vw->x0, vw->y0}, W, H,
                              ssaa_factor(opt, "rc_render_view"), opt->max_recursion, d_out, f.zc,
                              stream, cuda));
    }
    return f.end();
  });
}

// enqueue_view for the camera family (the caller has passed camera_refused or
// rays_from_refused): one launch of k_camera for the window's pixels (rays null), or of
// k_rays_from for the n rays whose origins are `origins`.  The view family's span owner: a camera
// frame is a view frame to rc_view_phase_ms.
static int enqueue_camera(DevCtx& c, const rc_scene* s, const rc_camera* cam, const rc_window* vw,
                          int W, int H, const rc_options* opt, uint8_t* d_out,
                          const RayBatch* rays, const float* origins, hipStream_t stream) {
  return ws_frame(c, stream, [] { return 0; }, [&]() -> int {
    SampleFrame f{c, stream, kSpanView};
    if (f.begin(s, nullptr, 0)) return -1;
    if (rays) {
      HIP_TRY(rc::launch_rays_from(f.ls, rays->n, origins, rays->dirs, opt->max_recursion,
                                   rays->out.rgb8, rays->out.rgb, rays->out.hits,
                                   rays->out.frame != 0, f.zc, stream));
    } else {
      rc::View v;
      std::memcpy(v.m, cam->view.m, sizeof v.m);
      HIP_TRY(rc::launch_camera(f.ls, cam->eye, v,
                                rc::Window{vw->full_w, vw->full_h, vw->x0, vw->y0}, W, H,
                                ssaa_factor(opt, "rc_render_camera"), opt->max_recursion, d_out,
                                f.zc, stream));
    }
    return f.end();
  });
}

// enqueue_accum for passes through cameras (the caller holds c.mu and has passed
// camera_accum_refused, the range checks and cameras_refused; fast mode): the accumulation
// family's frame, with its counter slots, its span owner and its edge list, and the camera
// kernels in the window kernels' place.  Sample j of pass k goes through cams[cam0[k] + j], or
// through cams[0] when ncams is 1.  The cameras are copied into the launch's argument here, so the
// caller's array is free when the call returns and nothing of a camera stays on the device.
static int enqueue_accum_camera(DevCtx& c, const rc_scene* s, const rc_camera* cams, int ncams,
                                const rc_window* vw, int W, int H, const rc_options* opt,
                                const rc_sample_seq* seq, const AccumPass* passes,
                                const int* cam0, int npasses, rc_accum_px* d_acc, uint8_t* d_out,
                                hipStream_t stream) {
  AccumFrame& a = c.acc;
  bool masked = false;
  for (int k = 0; k < npasses; ++k) masked = masked || passes[k].at > 0;
  auto prepare = [&]() -> int {
    if (a.count.ensure(AccumFrame::kSlots * 8) ||
        (masked && c.aa_list.ensure((size_t)W * H * sizeof(uint32_t)))) {
      std::fprintf(stderr, "Error: out of device memory for the edge list (%d x %d)\n", W, H);
      return -1;
    }
    return ensure_done(a.done);
  };
  return ws_frame(c, stream, prepare, [&]() -> int {
    a.valid = false;   // the block is this call's from here on
    SampleFrame f{c, stream, kSpanAccum};
    if (f.begin(s, &a.count, (size_t)npasses * 8)) return -1;
    unsigned* cnt = (unsigned*)a.count.p;
    uint32_t* list = (uint32_t*)c.aa_list.p;
    const int maxrec = opt->max_recursion, g = seq->grid;
    const rc::Window win{vw->full_w, vw->full_h, vw->x0, vw->y0};
    for (int k = 0; k < npasses; ++k) {
      const AccumPass& p = passes[k];
      const bool last = k + 1 == npasses;
      if (last && k > 0) HIP_TRY(hipEventRecord(f.ev[2], stream));
      rc::CamSet set;
      for (int j = 0; j < 16; ++j) {   // the slots past the pass's count are not read: camera 0's
        const rc_camera& cam = cams[ncams == 1 || j >= p.count ? 0 : cam0[k] + j];
        std::memcpy(set.eye[j], cam.eye, sizeof set.eye[j]);
        std::memcpy(set.view[j].m, cam.view.m, sizeof set.view[j].m);
      }
      const uint8_t* px = seq->x + p.first;
      const uint8_t* py = seq->y + p.first;
      unsigned* slot = cnt + 2 * k;
      if (p.at == 0) {
        HIP_TRY(rc::launch_accum_cam(f.ls, set, win, W, H, g, p.count, px, py, p.reset, maxrec,
                                     d_acc, d_out, f.zc, slot + 1, stream));
      } else {
        HIP_TRY(rc::launch_aa_mark(d_out, W, H, p.at, list, slot, stream));
        if (last) HIP_TRY(hipEventRecord(f.ev[3], stream));
        HIP_TRY(rc::launch_accum_list_cam(
            f.ls, set, win, W, H, g, p.count, px, py, maxrec, list, slot, d_acc, d_out, f.zc,
            slot + 1, rc::accum_list_blocks(W, H, c.cus, tune().adaptive_blocks), stream));
      }
      a.samples[k] = (uint8_t)p.count;
      a.listed[k] = p.at > 0;
    }
    if (f.end()) return -1;
    HIP_TRY(hipEventRecord(a.done, stream));
    a.valid = true;
    a.passes = npasses;
    a.pixels = (long long)W * H;
    a.ev_first = npasses > 1 ? 2 : 0;
    a.ev_listed = passes[npasses - 1].at > 0;
    return 0;
  });
}

// The passes of one ambient-occlusion call on `stream` through the device's one-frame workspace
// (the caller holds c.mu and has passed the pass's refusals): one launch of k_ao a set, pass k with
// sets[k]; the first one resets when `reset`, the last one alone stores the bytes (d_out, or null).
// The counter block is zeroed in front of every pass, so it holds the last pass's counts and
// nothing waits for the host.  The set is copied into the launch's argument here.  rays (or null):
// the call is a ray batch instead, one launch of k_occluded_rays, which counts nothing.
struct OccludedBatch {
  long long n;
  const float *origins, *dirs;
  const int32_t* skip;
  const float* tmax;
  uint8_t* out;
};
static int enqueue_ao(DevCtx& c, const rc_scene* s, const rc_camera* cam, const rc_window* vw,
                      int W, int H, const rc_ao_dirs* sets, int nsets, bool reset, rc_ao_px* d_ao,
                      uint8_t* d_out, const OccludedBatch* rays, hipStream_t stream) {
  AoFrame& a = c.ao;
  auto prepare = [&]() -> int {
    if (rays) return 0;
    if (a.count.ensure(rc::kAoStatBytes)) {
      std::fprintf(stderr, "Error: out of device memory for the occlusion counters\n");
      return -1;
    }
    return ensure_done(a.done);
  };
  return ws_frame(c, stream, prepare, [&]() -> int {
    SampleFrame f{c, stream, kSpanAo};
    if (rays) {
      if (f.begin(s, nullptr, 0)) return -1;
      HIP_TRY(rc::launch_occluded_rays(f.ls, rays->n, rays->origins, rays->dirs, rays->skip,
                                       rays->tmax, rays->out, stream));
      return f.end();
    }
    a.valid = false;   // the block is this call's from here on
    if (f.begin(s, &a.count, rc::kAoStatBytes)) return -1;
    rc::View v;
    std::memcpy(v.m, cam->view.m, sizeof v.m);
    const rc::Window win{vw->full_w, vw->full_h, vw->x0, vw->y0};
    for (int k = 0; k < nsets; ++k) {
      if (k > 0) HIP_TRY(hipMemsetAsync(a.count.p, 0, rc::kAoStatBytes, stream));
      rc::AoDirs d;
      static_assert(sizeof d == sizeof sets[k], "rc_ao_dirs is the kernel's argument");
      std::memcpy(&d, &sets[k], sizeof d);
      HIP_TRY(rc::launch_ao(f.ls, cam->eye, v, win, W, H, d, reset && k == 0, d_ao,
                            k + 1 == nsets ? d_out : nullptr, f.zc,
                            (unsigned long long*)a.count.p, stream));
    }
    if (f.end()) return -1;
    HIP_TRY(hipEventRecord(a.done, stream));
    a.valid = true;
    a.n = sets[nsets - 1].n;
    return 0;
  });
}

// One G-buffer frame through a camera on `stream` through the device's one-frame workspace (the
// caller holds c.mu and has passed camera_gbuffer_refused): one launch of k_camera_gbuffer.  The
// G-buffer family's span owner: a camera's planes are a G-buffer frame to rc_gbuffer_phase_ms.
static int enqueue_camera_gbuffer(DevCtx& c, const rc_scene* s, const rc_camera* cam,
                                  const rc_window* vw, int W, int H, const rc_gbuffer* planes,
                                  hipStream_t stream) {
  return ws_frame(c, stream, [] { return 0; }, [&]() -> int {
    SampleFrame f{c, stream, kSpanGbuffer};
    if (f.begin(s, nullptr, 0)) return -1;
    rc::View v;
    std::memcpy(v.m, cam->view.m, sizeof v.m);
    HIP_TRY(rc::launch_camera_gbuffer(f.ls, cam->eye, v,
                                      rc::Window{vw->full_w, vw->full_h, vw->x0, vw->y0}, W, H,
                                      planes->id, planes->t, planes->P, planes->N, f.zc, stream));
    return f.end();
  });
}

// the uploaded scene's diffuse colours (rc_scene.h: 3 floats a shape behind the pairs)
static const float* scene_diffuse(const DevCtx& c, const rc_scene* s) {
  return (const float*)((const char*)c.fb.scene.p + s->img->off_diffuse);
}

static rc::AoFilter ao_filter_arg(const rc_ao_filter* f) {
  rc::AoFilter a;
  static_assert(sizeof a == sizeof *f, "rc_ao_filter is the kernel's argument");
  std::memcpy(&a, f, sizeof a);
  return a;
}

// The compose on `stream` through the workspace (its scene alone: no counter, no event).
static int enqueue_compose(DevCtx& c, const rc_scene* s, const int32_t* d_id, const uint8_t* d_ao,
                           const float ambient[3], const uint8_t* d_in, uint8_t* d_out, int W,
                           int H, hipStream_t stream) {
  return ws_frame(c, stream, [] { return 0; }, [&]() -> int {
    rc::LaunchScene ls;
    if (upload_scene(c.fb, stream, s, ls)) return -1;
    const rc::Ambient amb{{ambient[0], ambient[1], ambient[2]}};
    HIP_TRY(rc::launch_ao_compose(scene_diffuse(c, s), ls.n, amb, d_id, d_ao, d_in, d_out, W, H,
                                  stream));
    return 0;
  });
}

// rc_render_ambient's frame on c.stream (the caller holds c.mu and has passed every entry's
// refusal): k_camera at one ray a pixel into c.out, the occlusion passes into the library's
// state (enqueue_ao's: a reset pass, the counter block zeroed in front of every pass), the
// camera's id, P and N, the filter into the library's plane and the compose in place, as one
// workspace frame with one span and one zero-normalize count over all its kernels.
static int enqueue_ambient(DevCtx& c, const rc_scene* s, const rc_camera* cam, const rc_window* vw,
                           int W, int H, const rc_options* opt, const rc_ao_dirs* sets, int nsets,
                           const rc_ao_filter* filter, const float ambient[3]) {
  AoFrame& a = c.ao;
  GuidedFrame& g = c.guided;
  hipStream_t stream = c.stream;
  auto prepare = [&]() -> int {
    if (a.count.ensure(rc::kAoStatBytes)) {
      std::fprintf(stderr, "Error: out of device memory for the occlusion counters\n");
      return -1;
    }
    return ensure_done(a.done);
  };
  return ws_frame(c, stream, prepare, [&]() -> int {
    SampleFrame f{c, stream, kSpanAo};
    a.valid = false;
    if (f.begin(s, &a.count, rc::kAoStatBytes)) return -1;
    rc::View v;
    std::memcpy(v.m, cam->view.m, sizeof v.m);
    const rc::Window win{vw->full_w, vw->full_h, vw->x0, vw->y0};
    uint8_t* img = (uint8_t*)c.out.p;
    HIP_TRY(rc::launch_camera(f.ls, cam->eye, v, win, W, H, 1, opt->max_recursion, img, f.zc,
                              stream));
    for (int k = 0; k < nsets; ++k) {
      if (k > 0) HIP_TRY(hipMemsetAsync(a.count.p, 0, rc::kAoStatBytes, stream));
      rc::AoDirs d;
      std::memcpy(&d, &sets[k], sizeof d);
      HIP_TRY(rc::launch_ao(f.ls, cam->eye, v, win, W, H, d, k == 0, g.state.p, nullptr, f.zc,
                            (unsigned long long*)a.count.p, stream));
    }
    HIP_TRY(rc::launch_camera_gbuffer(f.ls, cam->eye, v, win, W, H, (int32_t*)g.id.p, nullptr,
                                      (float*)g.P.p, (float*)g.N.p, f.zc, stream));
    HIP_TRY(rc::launch_ao_filter(g.state.p, (const int32_t*)g.id.p, (const float*)g.P.p,
                                 (const float*)g.N.p, W, H, ao_filter_arg(filter),
                                 (uint8_t*)g.plane.p, stream));
    const rc::Ambient amb{{ambient[0], ambient[1], ambient[2]}};
    HIP_TRY(rc::launch_ao_compose(scene_diffuse(c, s), f.ls.n, amb, (const int32_t*)g.id.p,
                                  (const uint8_t*)g.plane.p, img, img, W, H, stream));
    if (f.end()) return -1;
    HIP_TRY(hipEventRecord(a.done, stream));
    a.valid = true;
    a.n = sets[nsets - 1].n;
    return 0;
  });
}

// -------------------------------------------------------------- the two entry shapes --
// A *_device entry behind its null checks and its refusal: on the current device, on the
// caller's stream or the context's, enqueue(c, st), then finish_device.  plain: the frame goes
// through the plain path (enqueue_render: rc_render_filtered_device), whose scene upload and
// events live on c.stream, so c.stream is the caller's stream for the enqueue, and whose frame
// may be a parity frame that logs a hand-off entry.
template <class Enqueue>
static int device_entry(const rc_options* opt, void* stream, rc_timing* timing, bool plain,
                        Enqueue enqueue) {
  Entered e;
  if (enter(kCurrentDevice, true, e)) return -1;
  DevCtx& c = *e.c;
  hipStream_t st = stream ? (hipStream_t)stream : c.stream;
  const long long own = plain ? c.lone_log.head : kNoLog;
  hipStream_t saved = c.stream;
  if (plain) c.stream = st;
  const int rc = enqueue(c, st);
  c.stream = saved;
  return rc ? -1 : finish_device(c, opt, st, timing, own);
}

// A host-pixmap entry behind its null checks and its refusal (t0: taken before the refusal, so
// that total_ms covers the whole call): the timing zeroed, one tuning snapshot, opt->device
// entered, c.out for the W x H image and ensure_more(c) for what the feature adds, enqueue(c) on
// c.stream, then finish_host.  oom (W, H): the message when either allocation fails, null: the
// entry returns silently (rc_render_filtered, like rc_render).  plain: as device_entry; such a
// frame also gets rc_render's tail (the counts through pin_tail, the pixmap prefaulted).
template <class Ensure, class Enqueue>
static int host_entry(const rc_options* opt, int W, int H, uint8_t* pixmap, rc_timing* timing,
                      HostClock::time_point t0, const char* oom, bool plain, Ensure ensure_more,
                      Enqueue enqueue) {
  if (timing) std::memset(timing, 0, sizeof *timing);
  const rc_tuning tu = tune();
  Entered e;
  if (enter_host(opt, e)) return -1;
  DevCtx& c = *e.c;
  // a null pixmap: the call has no image (the G-buffer's entries); what ensure_more allocated is
  // copied back by enqueue on c.stream, in front of finish_host's wait
  const size_t bytes = pixmap ? (size_t)W * H * 3 : 0;
  if (c.out.ensure(bytes) || ensure_more(c)) return oom ? say(oom, W, H) : -1;
  const long long own = plain ? c.lone_log.head : kNoLog;
  if (enqueue(c)) return -1;
  return finish_host(c, opt, pixmap, bytes, tu, {plain, plain, own}, timing, t0);
}

static int nothing_more(DevCtx&) { return 0; }
static const char kImageOom[] = "Error: out of device memory for the image (%d x %d)\n";

extern "C" {

// rc_render_rates*: W <= 0 or H <= 0 returns silently, before the refusal.
int rc_render_rates_device(const rc_scene* s, int W, int H, const rc_options* opt,
                           const uint8_t* d_rates, uint8_t* d_out, void* stream,
                           rc_timing* timing) {
  const char* who = "rc_render_rates_device";
  if (!s || !opt || !d_rates || !d_out) return say("Error: %s: a null pointer\n", who);
  if (W <= 0 || H <= 0) return -1;
  if (rates_refused(who, opt, W, H)) return -1;
  return device_entry(opt, stream, timing, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_rates(c, s, W, H, opt, d_rates, d_out, st);
  });
}

int rc_render_rates(const rc_scene* s, int W, int H, const rc_options* opt, const uint8_t* rates,
                    uint8_t* pixmap, rc_timing* timing) {
  const char* who = "rc_render_rates";
  if (!s || !opt || !rates || !pixmap) return say("Error: %s: a null pointer\n", who);
  if (W <= 0 || H <= 0) return -1;
  const auto t0 = HostClock::now();
  if (rates_refused(who, opt, W, H)) return -1;
  const size_t pixels = (size_t)W * H;
  for (size_t i = 0; i < pixels; ++i) {
    const unsigned r = rates[i];
    if (r > 8u || !((0x117u >> r) & 1u))   // bits 0, 1, 2, 4, 8
      return say("Error: %s: rate %u at pixel (%zu, %zu) is not 0, 1, 2, 4 or 8\n", who, r,
                 i % (size_t)W, i / (size_t)W);
  }
  return host_entry(
      opt, W, H, pixmap, timing, t0,
      "Error: out of device memory for the image and its rate map (%d x %d)\n", false,
      [&](DevCtx& c) { return c.rates.map.ensure(pixels); },
      [&](DevCtx& c) -> int {
        uint8_t* d_out = (uint8_t*)c.out.p;
        uint8_t* d_rates = (uint8_t*)c.rates.map.p;
        // the pixmap goes in as well as out: the bytes of rate-0 pixels come back as they were
        HIP_TRY(hipMemcpyAsync(d_rates, rates, pixels, hipMemcpyHostToDevice, c.stream));
        HIP_TRY(hipMemcpyAsync(d_out, pixmap, pixels * 3, hipMemcpyHostToDevice, c.stream));
        return enqueue_rates(c, s, W, H, opt, d_rates, d_out, c.stream);
      });
}

int rc_render_pattern_device(const rc_scene* s, int W, int H, const rc_options* opt,
                             const rc_pattern* pat, int threshold, uint8_t* d_out, void* stream,
                             rc_timing* timing) {
  const char* who = "rc_render_pattern_device";
  if (!s || !opt || !pat || !d_out) return say("Error: %s: a null pointer\n", who);
  if (pattern_refused(who, opt, W, H, pat, threshold)) return -1;
  return device_entry(opt, stream, timing, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_pattern(c, s, W, H, opt, pat, threshold, d_out, st);
  });
}

int rc_render_pattern(const rc_scene* s, int W, int H, const rc_options* opt,
                      const rc_pattern* pat, int threshold, uint8_t* pixmap, rc_timing* timing) {
  const char* who = "rc_render_pattern";
  if (!s || !opt || !pat || !pixmap) return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  if (pattern_refused(who, opt, W, H, pat, threshold)) return -1;
  return host_entry(opt, W, H, pixmap, timing, t0, kImageOom, false, nothing_more, [&](DevCtx& c) {
    return enqueue_pattern(c, s, W, H, opt, pat, threshold, (uint8_t*)c.out.p, c.stream);
  });
}

// rc_accum_pass_device and rc_accum_pass_window_device (win: null for the former)
static int accum_pass(const char* who, const rc_scene* s, const rc_window* win, int W, int H,
                      const rc_options* opt, const rc_sample_seq* seq, int first, int count,
                      int threshold, int reset, rc_accum_px* d_acc, uint8_t* d_out, void* stream,
                      rc_timing* timing) {
  if (!s || !opt || !seq || !d_acc || !d_out) return say("Error: %s: a null pointer\n", who);
  if ((uintptr_t)d_acc & 7u)
    return say("Error: %s: the accumulator is not 8-byte aligned\n", who);
  if (accum_refused(who, opt, W, H, seq, threshold, threshold == 0, threshold > 0)) return -1;
  if (win && rc_window_check(win, W, H, seq->grid)) return -1;
  if (count < 1 || count > 16 || first < 0 || first > seq->nsamples - count)
    return say("Error: %s: samples [%d, %d + %d) of a sequence of %d: a pass takes 1..16 samples "
               "inside the sequence\n", who, first, first, count, seq->nsamples);
  if (reset && threshold > 0)
    return say("Error: %s: reset with threshold %d: a reset pass takes every pixel (there is no "
               "image yet to find edges in), leave the threshold at 0\n", who, threshold);
  const AccumPass pass{first, count, threshold, reset != 0};
  return device_entry(opt, stream, timing, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_accum(c, s, W, H, opt, seq, &pass, 1, d_acc, d_out, st, win);
  });
}

int rc_accum_pass_device(const rc_scene* s, int W, int H, const rc_options* opt,
                         const rc_sample_seq* seq, int first, int count, int threshold, int reset,
                         rc_accum_px* d_acc, uint8_t* d_out, void* stream, rc_timing* timing) {
  return accum_pass("rc_accum_pass_device", s, nullptr, W, H, opt, seq, first, count, threshold,
                    reset, d_acc, d_out, stream, timing);
}

int rc_accum_pass_window_device(const rc_scene* s, const rc_window* win, int W, int H,
                                const rc_options* opt, const rc_sample_seq* seq, int first,
                                int count, int threshold, int reset, rc_accum_px* d_acc,
                                uint8_t* d_out, void* stream, rc_timing* timing) {
  const char* who = "rc_accum_pass_window_device";
  if (!win) return say("Error: %s: a null pointer\n", who);
  return accum_pass(who, s, win, W, H, opt, seq, first, count, threshold, reset, d_acc, d_out,
                    stream, timing);
}

int rc_accum_scroll_device(const rc_scene* s, const rc_window* win, int W, int H,
                           const rc_options* opt, const rc_sample_seq* seq, int count, int dx,
                           int dy, const rc_accum_px* d_acc_src, const uint8_t* d_out_src,
                           rc_accum_px* d_acc_dst, uint8_t* d_out_dst, void* stream,
                           rc_timing* timing) {
  const char* who = "rc_accum_scroll_device";
  if (!s || !win || !opt || !seq || !d_acc_src || !d_out_src || !d_acc_dst || !d_out_dst)
    return say("Error: %s: a null pointer\n", who);
  if (((uintptr_t)d_acc_src | (uintptr_t)d_acc_dst) & 7u)
    return say("Error: %s: an accumulator is not 8-byte aligned\n", who);
  if (accum_refused(who, opt, W, H, seq, 0, true, false)) return -1;
  if (rc_window_check(win, W, H, seq->grid)) return -1;
  if ((unsigned long long)W * (unsigned long long)H >= (1ull << 32))
    return say("Error: %s: %d x %d is too large to scroll (32-bit pixel indices)\n", who, W, H);
  if (count < 1 || count > seq->nsamples)
    return say("Error: %s: count %d is not 1..%d (the sequence's length)\n", who, count,
               seq->nsamples);
  const size_t pixels = (size_t)W * H;
  const auto overlap = [](const void* a, const void* b, size_t n) {
    return (uintptr_t)a < (uintptr_t)b + n && (uintptr_t)b < (uintptr_t)a + n;
  };
  if (overlap(d_acc_src, d_acc_dst, pixels * sizeof(rc_accum_px)))
    return say("Error: %s: the source and the destination accumulators overlap: a kept record "
               "moves from one state to the other, keep two states and swap them\n", who);
  if (overlap(d_out_src, d_out_dst, pixels * 3))
    return say("Error: %s: the source and the destination images overlap: a kept pixel moves "
               "from one state to the other, keep two states and swap them\n", who);
  return device_entry(opt, stream, timing, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_scroll(c, s, win, W, H, opt, seq, count, dx, dy, d_acc_src, d_out_src,
                          d_acc_dst, d_out_dst, st);
  });
}

int rc_render_window_device(const rc_scene* s, const rc_window* win, int W, int H,
                            const rc_options* opt, uint8_t* d_out, void* stream,
                            rc_timing* timing) {
  const char* who = "rc_render_window_device";
  if (!s || !win || !opt || !d_out) return say("Error: %s: a null pointer\n", who);
  if (window_refused(who, opt, W, H, win)) return -1;
  return device_entry(opt, stream, timing, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_window(c, s, win, W, H, opt, d_out, st);
  });
}

int rc_render_window(const rc_scene* s, const rc_window* win, int W, int H, const rc_options* opt,
                     uint8_t* pixmap, rc_timing* timing) {
  const char* who = "rc_render_window";
  if (!s || !win || !opt || !pixmap) return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  if (window_refused(who, opt, W, H, win)) return -1;
  return host_entry(opt, W, H, pixmap, timing, t0, kImageOom, false, nothing_more, [&](DevCtx& c) {
    return enqueue_window(c, s, win, W, H, opt, (uint8_t*)c.out.p, c.stream);
  });
}

// ------------------------------------------------ the primary-visibility G-buffer --
// The tail's options of a G-buffer frame: one kernel between ev[0] and ev[1] whatever the mode, so
// the timing record is filled as a fast frame's (everything parity-specific stays 0).
static rc_options gbuffer_tail(const rc_options* opt) {
  rc_options o = *opt;
  o.mode = RC_MODE_FAST;
  return o;
}

// rc_render_gbuffer and rc_render_gbuffer_device behind their null checks: the refusal and the
// window the frame is shot through (win null: the whole W x H image)
static int gbuffer_planes_refused(const char* who, const rc_options* opt, const rc_window* win,
                                  int W, int H, const rc_gbuffer* planes, rc_window* vw) {
  if (!planes->id && !planes->t && !planes->P && !planes->N)
    return say("Error: %s: all four planes are null: ask for at least one of id, t, P and N\n",
               who);
  *vw = win ? *win : rc_window{W, H, 0, 0};
  return gbuffer_refused(who, opt, planes->P || planes->N,
                         [&] { return rc_window_check(vw, W, H, 1); });
}

int rc_render_gbuffer_device(const rc_scene* s, const rc_window* win, int W, int H,
                             const rc_options* opt, const rc_gbuffer* d_planes, void* stream,
                             rc_timing* timing) {
  const char* who = "rc_render_gbuffer_device";
  if (!s || !opt || !d_planes) return say("Error: %s: a null pointer\n", who);
  rc_window vw;
  if (gbuffer_planes_refused(who, opt, win, W, H, d_planes, &vw)) return -1;
  const rc_options tail = gbuffer_tail(opt);
  return device_entry(&tail, stream, timing, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_gbuffer(c, s, rc::Window{vw.full_w, vw.full_h, vw.x0, vw.y0}, W, H, opt,
                           d_planes, nullptr, st);
  });
}

int rc_render_gbuffer(const rc_scene* s, const rc_window* win, int W, int H, const rc_options* opt,
                      const rc_gbuffer* planes, rc_timing* timing) {
  const char* who = "rc_render_gbuffer";
  if (!s || !opt || !planes) return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  rc_window vw;
  if (gbuffer_planes_refused(who, opt, win, W, H, planes, &vw)) return -1;
  const rc_options tail = gbuffer_tail(opt);
  const size_t px = (size_t)W * H * sizeof(float);
  return host_entry(
      &tail, W, H, nullptr, timing, t0,
      "Error: out of device memory for the G-buffer's planes (%d x %d)\n", false,
      [&](DevCtx& c) {   // device copies of the planes asked for
        GbufFrame& g = c.gbuf;
        return (planes->id && g.id.ensure(px)) || (planes->t && g.t.ensure(px)) ||
               (planes->P && g.P.ensure(3 * px)) || (planes->N && g.N.ensure(3 * px));
      },
      [&](DevCtx& c) -> int {
        const GbufFrame& g = c.gbuf;
        const rc_gbuffer d{planes->id ? (int32_t*)g.id.p : nullptr,
                           planes->t ? (float*)g.t.p : nullptr,
                           planes->P ? (float*)g.P.p : nullptr,
                           planes->N ? (float*)g.N.p : nullptr};
        if (enqueue_gbuffer(c, s, rc::Window{vw.full_w, vw.full_h, vw.x0, vw.y0}, W, H, opt, &d,
                            nullptr, c.stream))
          return -1;
        // behind the kernel on c.stream, in front of finish_host's wait
        auto back = [&](void* host, const void* dev, size_t bytes) -> int {
          if (host) HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c.stream));
          return 0;
        };
        return back(planes->id, d.id, px) || back(planes->t, d.t, px) ||
               back(planes->P, d.P, 3 * px) || back(planes->N, d.N, 3 * px);
      });
}

// rc_pick and rc_pick_device behind their null checks
static int pick_refused(const char* who, const rc_options* opt, int full_w, int full_h, int frame,
                        int64_t n) {
  if (gbuffer_refused(who, opt, frame != 0, [&] {
        if (full_w >= 1 && full_h >= 1) return 0;
        return say("Error: %s: a %d x %d image: both sides must be at least 1\n", who, full_w,
                   full_h);
      }))
    return -1;
  if (n < 1 || n > ((int64_t)1 << 24))
    return say("Error: %s: n %lld is not 1 .. 2^24 points\n", who, (long long)n);
  return 0;
}

int rc_pick_device(const rc_scene* s, int full_w, int full_h, const rc_options* opt, int frame,
                   int64_t n, const int32_t* d_xy, rc_hit* d_hits, void* stream) {
  const char* who = "rc_pick_device";
  if (!s || !opt || !d_xy || !d_hits) return say("Error: %s: a null pointer\n", who);
  if ((uintptr_t)d_hits & 15u)
    return say("Error: %s: the records are not 16-byte aligned\n", who);
  if (pick_refused(who, opt, full_w, full_h, frame, n)) return -1;
  const rc_options tail = gbuffer_tail(opt);
  const GbufPoints pts{frame, n, d_xy, d_hits};
  return device_entry(&tail, stream, nullptr, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_gbuffer(c, s, rc::Window{full_w, full_h, 0, 0}, 0, 0, opt, nullptr, &pts, st);
  });
}

int rc_pick(const rc_scene* s, int full_w, int full_h, const rc_options* opt, int frame, int64_t n,
            const int32_t* xy, rc_hit* hits) {
  const char* who = "rc_pick";
  if (!s || !opt || !xy || !hits) return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  if (pick_refused(who, opt, full_w, full_h, frame, n)) return -1;
  for (int64_t k = 0; k < n; ++k) {
    const int x = xy[2 * k], y = xy[2 * k + 1];
    if (x < 0 || x >= full_w || y < 0 || y >= full_h)
      return say("Error: %s: point %lld at (%d, %d) is outside the %d x %d image\n", who,
                 (long long)k, x, y, full_w, full_h);
  }
  const rc_options tail = gbuffer_tail(opt);
  const size_t nxy = (size_t)n * 2 * sizeof(int32_t), nhits = (size_t)n * sizeof(rc_hit);
  return host_entry(
      &tail, 0, 0, nullptr, nullptr, t0, "Error: out of device memory for the picked points\n",
      false, [&](DevCtx& c) { return c.gbuf.xy.ensure(nxy) || c.gbuf.hits.ensure(nhits); },
      [&](DevCtx& c) -> int {
        const GbufPoints pts{frame, n, (const int32_t*)c.gbuf.xy.p, (rc_hit*)c.gbuf.hits.p};
        HIP_TRY(hipMemcpyAsync(c.gbuf.xy.p, xy, nxy, hipMemcpyHostToDevice, c.stream));
        if (enqueue_gbuffer(c, s, rc::Window{full_w, full_h, 0, 0}, 0, 0, opt, nullptr, &pts,
                            c.stream))
          return -1;
        HIP_TRY(hipMemcpyAsync(hits, c.gbuf.hits.p, nhits, hipMemcpyDeviceToHost, c.stream));
        return 0;
      });
}

// No frame of the workspace: the edge map of an id plane alone, on the current device.
int rc_id_edge_rates_device(const int32_t* d_id, int W, int H, int s, int base, uint8_t* d_rates,
                            void* stream) {
  const char* who = "rc_id_edge_rates_device";
  if (!d_id || !d_rates) return say("Error: %s: a null pointer\n", who);
  if (s != 2 && s != 4 && s != 8) return say("Error: %s: s %d is not 2, 4 or 8\n", who, s);
  if (base != 0 && base != 1) return say("Error: %s: base %d is not 0 or 1\n", who, base);
  if (W < 1 || H < 1)
    return say("Error: %s: %d x %d: both sides must be at least 1\n", who, W, H);
  if ((unsigned long long)W * (unsigned long long)H >= (1ull << 32))
    return say("Error: %s: %d x %d is too large (32-bit pixel indices)\n", who, W, H);
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  DevCtx* c;
  if (ctx_get(dev, &c)) return -1;
  HIP_TRY(rc::launch_id_edge_rates(d_id, W, H, s, base, d_rates,
                                   stream ? (hipStream_t)stream : c->stream));
  return 0;
}

int rc_gbuffer_phase_ms(double ms[1]) {
  Entered e;
  if (!ms || enter(kCurrentDevice, false, e)) return -1;
  hipEvent_t* ev = e.c->span_ev[kSpanGbuffer];
  return ev ? read_spans({ev[0], ev[1]}, ms) : -1;
}

// ------------------------------------------- rotated camera views and ray batches --
int rc_render_view_device(const rc_scene* s, const rc_view* view, const rc_window* win, int W,
                          int H, const rc_options* opt, uint8_t* d_out, void* stream,
                          rc_timing* timing) {
  const char* who = "rc_render_view_device";
  if (!s || !view || !opt || !d_out) return say("Error: %s: a null pointer\n", who);
  const rc_window vw = win ? *win : rc_window{W, H, 0, 0};
  if (view_refused(who, opt, W, H, view, &vw)) return -1;
  return device_entry(opt, stream, timing, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_view(c, s, view, &vw, W, H, opt, d_out, nullptr, st);
  });
}

int rc_render_view(const rc_scene* s, const rc_view* view, const rc_window* win, int W, int H,
                   const rc_options* opt, uint8_t* pixmap, rc_timing* timing) {
  const char* who = "rc_render_view";
  if (!s || !view || !opt || !pixmap) return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  const rc_window vw = win ? *win : rc_window{W, H, 0, 0};
  if (view_refused(who, opt, W, H, view, &vw)) return -1;
  return host_entry(opt, W, H, pixmap, timing, t0, kImageOom, false, nothing_more, [&](DevCtx& c) {
    return enqueue_view(c, s, view, &vw, W, H, opt, (uint8_t*)c.out.p, nullptr, c.stream);
  });
}

// rc_trace_rays and rc_trace_rays_device behind their null checks
static int rays_out_refused(const char* who, const rc_ray_out* out) {
  if (out->rgb8 || out->rgb || out->hits) return 0;
  return say("Error: %s: all three outputs are null: ask for at least one of rgb8, rgb and hits\n",
             who);
}

int rc_trace_rays_device(const rc_scene* s, const rc_options* opt, int64_t n, const float* d_dirs,
                         const rc_ray_out* d_out, void* stream) {
  const char* who = "rc_trace_rays_device";
  if (!s || !opt || !d_dirs || !d_out) return say("Error: %s: a null pointer\n", who);
  if (rays_out_refused(who, d_out)) return -1;
  if ((uintptr_t)d_out->hits & 15u)
    return say("Error: %s: the records are not 16-byte aligned\n", who);
  if (rays_refused(who, opt, n, d_out)) return -1;
  const RayBatch rays{n, d_dirs, *d_out};
  return device_entry(opt, stream, nullptr, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_view(c, s, nullptr, nullptr, 0, 0, opt, nullptr, &rays, st);
  });
}

int rc_trace_rays(const rc_scene* s, const rc_options* opt, int64_t n, const float* dirs,
                  const rc_ray_out* out) {
  const char* who = "rc_trace_rays";
  if (!s || !opt || !dirs || !out) return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  if (rays_out_refused(who, out)) return -1;
  if (rays_refused(who, opt, n, out)) return -1;
  const size_t n3 = (size_t)n * 3, nhits = (size_t)n * sizeof(rc_hit);
  return host_entry(
      opt, 0, 0, nullptr, nullptr, t0, "Error: out of device memory for the ray batch\n", false,
      [&](DevCtx& c) {   // device copies of the directions and of the outputs asked for
        ViewFrame& v = c.view;
        return v.dirs.ensure(n3 * sizeof(float)) || (out->rgb8 && v.rgb8.ensure(n3)) ||
               (out->rgb && v.rgb.ensure(n3 * sizeof(float))) ||
               (out->hits && v.hits.ensure(nhits));
      },
      [&](DevCtx& c) -> int {
        const ViewFrame& v = c.view;
        const RayBatch rays{n, (const float*)v.dirs.p,
                            rc_ray_out{out->rgb8 ? (uint8_t*)v.rgb8.p : nullptr,
                                       out->rgb ? (float*)v.rgb.p : nullptr,
                                       out->hits ? (rc_hit*)v.hits.p : nullptr, out->frame}};
        HIP_TRY(hipMemcpyAsync(v.dirs.p, dirs, n3 * sizeof(float), hipMemcpyHostToDevice,
                               c.stream));
        if (enqueue_view(c, s, nullptr, nullptr, 0, 0, opt, nullptr, &rays, c.stream)) return -1;
        // behind the kernel on c.stream, in front of finish_host's wait
        auto back = [&](void* host, const void* dev, size_t bytes) -> int {
          if (host) HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c.stream));
          return 0;
        };
        return back(out->rgb8, rays.out.rgb8, n3) ||
               back(out->rgb, rays.out.rgb, n3 * sizeof(float)) ||
               back(out->hits, rays.out.hits, nhits);
      });
}

int rc_view_phase_ms(double ms[1]) {
  Entered e;
  if (!ms || enter(kCurrentDevice, false, e)) return -1;
  hipEvent_t* ev = e.c->span_ev[kSpanView];
  return ev ? read_spans({ev[0], ev[1]}, ms) : -1;
}

// --------------------------------------------- a free camera and rays with origins --
int rc_render_camera_device(const rc_scene* s, const rc_camera* cam, const rc_window* win, int W,
                            int H, const rc_options* opt, uint8_t* d_out, void* stream,
                            rc_timing* timing) {
  const char* who = "rc_render_camera_device";
  if (!s || !cam || !opt || !d_out) return say("Error: %s: a null pointer\n", who);
  const rc_window vw = win ? *win : rc_window{W, H, 0, 0};
  if (camera_refused(who, opt, W, H, cam, &vw)) return -1;
  return device_entry(opt, stream, timing, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_camera(c, s, cam, &vw, W, H, opt, d_out, nullptr, nullptr, st);
  });
}

int rc_render_camera(const rc_scene* s, const rc_camera* cam, const rc_window* win, int W, int H,
                     const rc_options* opt, uint8_t* pixmap, rc_timing* timing) {
  const char* who = "rc_render_camera";
  if (!s || !cam || !opt || !pixmap) return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  const rc_window vw = win ? *win : rc_window{W, H, 0, 0};
  if (camera_refused(who, opt, W, H, cam, &vw)) return -1;
  return host_entry(opt, W, H, pixmap, timing, t0, kImageOom, false, nothing_more, [&](DevCtx& c) {
    return enqueue_camera(c, s, cam, &vw, W, H, opt, (uint8_t*)c.out.p, nullptr, nullptr,
                          c.stream);
  });
}

int rc_trace_rays_from_device(const rc_scene* s, const rc_options* opt, int64_t n,
                              const float* d_origins, const float* d_dirs,
                              const rc_ray_out* d_out, void* stream) {
  const char* who = "rc_trace_rays_from_device";
  if (!s || !opt || !d_origins || !d_dirs || !d_out) return say("Error: %s: a null pointer\n", who);
  if (rays_out_refused(who, d_out)) return -1;
  if ((uintptr_t)d_out->hits & 15u)
    return say("Error: %s: the records are not 16-byte aligned\n", who);
  if (rays_from_refused(who, opt, n)) return -1;
  const RayBatch rays{n, d_dirs, *d_out};
  return device_entry(opt, stream, nullptr, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_camera(c, s, nullptr, nullptr, 0, 0, opt, nullptr, &rays, d_origins, st);
  });
}

int rc_trace_rays_from(const rc_scene* s, const rc_options* opt, int64_t n, const float* origins,
                       const float* dirs, const rc_ray_out* out) {
  const char* who = "rc_trace_rays_from";
  if (!s || !opt || !origins || !dirs || !out) return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  if (rays_out_refused(who, out)) return -1;
  if (rays_from_refused(who, opt, n)) return -1;
  const size_t n3 = (size_t)n * 3, nhits = (size_t)n * sizeof(rc_hit);
  return host_entry(
      opt, 0, 0, nullptr, nullptr, t0, "Error: out of device memory for the ray batch\n", false,
      [&](DevCtx& c) {   // device copies of the rays and of the outputs asked for
        ViewFrame& v = c.view;
        return v.origins.ensure(n3 * sizeof(float)) || v.dirs.ensure(n3 * sizeof(float)) ||
               (out->rgb8 && v.rgb8.ensure(n3)) ||
               (out->rgb && v.rgb.ensure(n3 * sizeof(float))) ||
               (out->hits && v.hits.ensure(nhits));
      },
      [&](DevCtx& c) -> int {
        const ViewFrame& v = c.view;
        const RayBatch rays{n, (const float*)v.dirs.p,
                            rc_ray_out{out->rgb8 ? (uint8_t*)v.rgb8.p : nullptr,
                                       out->rgb ? (float*)v.rgb.p : nullptr,
                                       out->hits ? (rc_hit*)v.hits.p : nullptr, out->frame}};
        HIP_TRY(hipMemcpyAsync(v.origins.p, origins, n3 * sizeof(float), hipMemcpyHostToDevice,
                               c.stream));
        HIP_TRY(hipMemcpyAsync(v.dirs.p, dirs, n3 * sizeof(float), hipMemcpyHostToDevice,
                               c.stream));
        if (enqueue_camera(c, s, nullptr, nullptr, 0, 0, opt, nullptr, &rays,
                           (const float*)v.origins.p, c.stream))
          return -1;
        // behind the kernel on c.stream, in front of finish_host's wait
        auto back = [&](void* host, const void* dev, size_t bytes) -> int {
          if (host) HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c.stream));
          return 0;
        };
        return back(out->rgb8, rays.out.rgb8, n3) ||
               back(out->rgb, rays.out.rgb, n3 * sizeof(float)) ||
               back(out->hits, rays.out.hits, nhits);
      });
}

// No frame of the workspace: the resolve of an accumulator alone, on the current device.
int rc_accum_resolve_device(const rc_accum_px* d_acc, int W, int H, uint8_t* d_out, void* stream) {
  const char* who = "rc_accum_resolve_device";
  if (!d_acc || !d_out) return say("Error: %s: a null pointer\n", who);
  if ((uintptr_t)d_acc & 7u)
    return say("Error: %s: the accumulator is not 8-byte aligned\n", who);
  if (W <= 0 || H <= 0 ||
      ((unsigned long long)W * (unsigned long long)H + 255) / 256 > 0x7fffffffull)
    return say("Error: %s: %d x %d: both sides must be at least 1 and the image at most 2^39 - 256 "
               "pixels (one grid)\n", who, W, H);
  Entered e;
  if (enter(kCurrentDevice, false, e)) return -1;
  hipStream_t st = stream ? (hipStream_t)stream : e.c->stream;
  HIP_TRY(rc::launch_accum_resolve(d_acc, W, H, d_out, st));
  return 0;
}

int rc_render_accum(const rc_scene* s, int W, int H, const rc_options* opt,
                    const rc_sample_seq* seq, int dense, int threshold, uint8_t* pixmap,
                    rc_timing* timing) {
  const char* who = "rc_render_accum";
  if (!s || !opt || !seq || !pixmap) return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  // which kernels run is known once the sequence and dense have been checked; the limits of both
  // are tested here, a call that needs only one of them being a sub-case of no interest
  if (accum_refused(who, opt, W, H, seq, threshold, true, threshold > 0)) return -1;
  if (dense < 1 || dense > seq->nsamples)
    return say("Error: %s: dense %d is not 1..%d (the sequence's length)\n", who, dense,
               seq->nsamples);
  // samples [0, dense) for every pixel in chunks of at most 16, the first chunk resetting the
  // accumulator; then one single-sample pass for each of the others
  AccumPass passes[AccumFrame::kSlots];
  int np = 0;
  for (int k = 0; k < dense; k += 16)
    passes[np++] = {k, dense - k < 16 ? dense - k : 16, 0, k == 0};
  for (int k = dense; k < seq->nsamples; ++k) passes[np++] = {k, 1, threshold, false};
  return host_entry(
      opt, W, H, pixmap, timing, t0,
      "Error: out of device memory for the image and its accumulator (%d x %d)\n", false,
      [&](DevCtx& c) { return c.accum_px.ensure((size_t)W * H * sizeof(rc_accum_px)); },
      [&](DevCtx& c) {
        return enqueue_accum(c, s, W, H, opt, seq, passes, np, (rc_accum_px*)c.accum_px.p,
                             (uint8_t*)c.out.p, c.stream);
      });
}

// ------------------------------------------------ accumulation through a free camera --
int rc_accum_pass_camera_device(const rc_scene* s, const rc_camera* cams, int ncams,
                                const rc_window* win, int W, int H, const rc_options* opt,
                                const rc_sample_seq* seq, int first, int count, int threshold,
                                int reset, rc_accum_px* d_acc, uint8_t* d_out, void* stream,
                                rc_timing* timing) {
  const char* who = "rc_accum_pass_camera_device";
  if (!s || !cams || !opt || !seq || !d_acc || !d_out)
    return say("Error: %s: a null pointer\n", who);
  if ((uintptr_t)d_acc & 7u)
    return say("Error: %s: the accumulator is not 8-byte aligned\n", who);
  if (camera_accum_refused(who, opt, W, H, seq, threshold, threshold == 0, threshold > 0))
    return -1;
  const rc_window vw = win ? *win : rc_window{W, H, 0, 0};
  if (rc_window_check(&vw, W, H, seq->grid)) return -1;
  if (count < 1 || count > 16 || first < 0 || first > seq->nsamples - count)
    return say("Error: %s: samples [%d, %d + %d) of a sequence of %d: a pass takes 1..16 samples "
               "inside the sequence\n", who, first, first, count, seq->nsamples);
  if (reset && threshold > 0)
    return say("Error: %s: reset with threshold %d: a reset pass takes every pixel (there is no "
               "image yet to find edges in), leave the threshold at 0\n", who, threshold);
  if (cameras_refused(who, cams, ncams, count, "count")) return -1;
  const AccumPass pass{first, count, threshold, reset != 0};
  const int cam0 = 0;   // camera j of the pass is cams[j], whatever `first` is
  return device_entry(opt, stream, timing, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_accum_camera(c, s, cams, ncams, &vw, W, H, opt, seq, &pass, &cam0, 1, d_acc,
                                d_out, st);
  });
}

int rc_render_camera_accum(const rc_scene* s, const rc_camera* cams, int ncams,
                           const rc_window* win, int W, int H, const rc_options* opt,
                           const rc_sample_seq* seq, uint8_t* pixmap, rc_timing* timing) {
  const char* who = "rc_render_camera_accum";
  if (!s || !cams || !opt || !seq || !pixmap) return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  if (camera_accum_refused(who, opt, W, H, seq, 0, true, false)) return -1;
  const rc_window vw = win ? *win : rc_window{W, H, 0, 0};
  if (rc_window_check(&vw, W, H, seq->grid)) return -1;
  if (cameras_refused(who, cams, ncams, seq->nsamples, "the sequence's length")) return -1;
  // the whole sequence for every pixel in chunks of at most 16, the first one resetting; sample k
  // goes through cams[k]
  AccumPass passes[(RC_ACCUM_MAX_SAMPLES + 15) / 16];
  int cam0[(RC_ACCUM_MAX_SAMPLES + 15) / 16];
  int np = 0;
  for (int k = 0; k < seq->nsamples; k += 16) {
    cam0[np] = k;
    passes[np++] = {k, seq->nsamples - k < 16 ? seq->nsamples - k : 16, 0, k == 0};
  }
  return host_entry(
      opt, W, H, pixmap, timing, t0,
      "Error: out of device memory for the image and its accumulator (%d x %d)\n", false,
      [&](DevCtx& c) { return c.accum_px.ensure((size_t)W * H * sizeof(rc_accum_px)); },
      [&](DevCtx& c) {
        return enqueue_accum_camera(c, s, cams, ncams, &vw, W, H, opt, seq, passes, cam0, np,
                                    (rc_accum_px*)c.accum_px.p, (uint8_t*)c.out.p, c.stream);
      });
}

// ------------------------------------- any-hit visibility queries and ambient occlusion --
int rc_ao_dirs_check(const rc_ao_dirs* dirs) {
  const char* who = "rc_ao_dirs_check";
  if (!dirs) return say("Error: %s: a null direction set\n", who);
  char buf[96];
  const char* why = ao_dirs_problem(dirs, buf, sizeof buf);
  return why ? say("Error: %s: %s\n", who, why) : 0;
}

int rc_ao_stats_get(rc_ao_stats* out) {
  Entered e;
  if (!out || enter(kCurrentDevice, false, e) || !e.c->ao.valid) return -1;
  const AoFrame& a = e.c->ao;
  HIP_TRY(hipEventSynchronize(a.done));   // the call's stream, up to its last pass
  unsigned long long lines[rc::kAoStatSlots][rc::kAoStatStride];   // 32 KiB
  HIP_TRY(hipMemcpy(lines, a.count.p, sizeof lines, hipMemcpyDeviceToHost));
  unsigned long long n[3] = {0, 0, 0};    // launch_ao's counters, summed over its lines
  for (const auto& line : lines)
    for (int k = 0; k < 3; ++k) n[k] += line[k];
  out->hit_pixels = (int64_t)n[0];
  out->rays = (int64_t)n[0] * a.n;
  out->blocked = (int64_t)n[1];
  out->saturated = (int64_t)n[2];
  return 0;
}

int rc_ao_phase_ms(double ms[1]) {
  Entered e;
  if (!ms || enter(kCurrentDevice, false, e)) return -1;
  hipEvent_t* ev = e.c->span_ev[kSpanAo];
  return ev ? read_spans({ev[0], ev[1]}, ms) : -1;
}

static int occluded_rays_refused(const char* who, const rc_options* opt, int64_t n) {
  if (ao_refused(who, opt, [] { return 0; })) return -1;
  if (n < 1 || n > ((int64_t)1 << 24))
    return say("Error: %s: n %lld is not 1 .. 2^24 rays\n", who, (long long)n);
  return 0;
}

int rc_occluded_rays_device(const rc_scene* s, const rc_options* opt, int64_t n,
                            const float* d_origins, const float* d_dirs, const int32_t* d_skip,
                            const float* d_tmax, uint8_t* d_out, void* stream,
                            rc_timing* timing) {
  const char* who = "rc_occluded_rays_device";
  if (!s || !opt || !d_origins || !d_dirs || !d_out) return say("Error: %s: a null pointer\n", who);
  if (occluded_rays_refused(who, opt, n)) return -1;
  const OccludedBatch rays{n, d_origins, d_dirs, d_skip, d_tmax, d_out};
  return device_entry(opt, stream, timing, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_ao(c, s, nullptr, nullptr, 0, 0, nullptr, 0, false, nullptr, nullptr, &rays,
                      st);
  });
}

int rc_occluded_rays(const rc_scene* s, const rc_options* opt, int64_t n, const float* origins,
                     const float* dirs, const int32_t* skip, const float* tmax, uint8_t* out,
                     void* /*stream*/, rc_timing* timing) {
  const char* who = "rc_occluded_rays";
  if (!s || !opt || !origins || !dirs || !out) return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  if (occluded_rays_refused(who, opt, n)) return -1;
  const size_t n3 = (size_t)n * 3 * sizeof(float), n1 = (size_t)n * 4;
  return host_entry(
      opt, 0, 0, nullptr, timing, t0, "Error: out of device memory for the ray batch\n", false,
      [&](DevCtx& c) {   // device copies of the rays and of the bytes
        AoFrame& a = c.ao;
        return a.origins.ensure(n3) || a.dirs.ensure(n3) || (skip && a.skip.ensure(n1)) ||
               (tmax && a.tmax.ensure(n1)) || a.flags.ensure((size_t)n);
      },
      [&](DevCtx& c) -> int {
        const AoFrame& a = c.ao;
        auto in = [&](void* dev, const void* host, size_t bytes) -> int {
          if (host) HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c.stream));
          return 0;
        };
        if (in(a.origins.p, origins, n3) || in(a.dirs.p, dirs, n3) || in(a.skip.p, skip, n1) ||
            in(a.tmax.p, tmax, n1))
          return -1;
        const OccludedBatch rays{n, (const float*)a.origins.p, (const float*)a.dirs.p,
                                 skip ? (const int32_t*)a.skip.p : nullptr,
                                 tmax ? (const float*)a.tmax.p : nullptr, (uint8_t*)a.flags.p};
        if (enqueue_ao(c, s, nullptr, nullptr, 0, 0, nullptr, 0, false, nullptr, nullptr, &rays,
                       c.stream))
          return -1;
        // behind the kernel on c.stream, in front of finish_host's wait
        HIP_TRY(hipMemcpyAsync(out, a.flags.p, (size_t)n, hipMemcpyDeviceToHost, c.stream));
        return 0;
      });
}

// rc_ao_pass_device and rc_render_ao behind their null checks and the alignment: clauses 3 to 5
// of the documented order, and the window the pass is shot through (win null: the whole image)
static int ao_pass_refused(const char* who, const rc_options* opt, const rc_camera* cam,
                           const rc_window* win, int W, int H, rc_window* vw) {
  *vw = win ? *win : rc_window{W, H, 0, 0};
  if (ao_refused(who, opt, [&] { return rc_window_check(vw, W, H, 1); })) return -1;
  return rc_camera_check(cam);
}

int rc_ao_pass_device(const rc_scene* s, const rc_camera* cam, const rc_window* win, int W, int H,
                      const rc_options* opt, const rc_ao_dirs* dirs, int reset, rc_ao_px* d_ao,
                      uint8_t* d_out, void* stream, rc_timing* timing) {
  const char* who = "rc_ao_pass_device";
  if (!s || !cam || !opt || !dirs || !d_ao) return say("Error: %s: a null pointer\n", who);
  if ((uintptr_t)d_ao & 3u) return say("Error: %s: the state is not 4-byte aligned\n", who);
  rc_window vw;
  if (ao_pass_refused(who, opt, cam, win, W, H, &vw) || rc_ao_dirs_check(dirs)) return -1;
  return device_entry(opt, stream, timing, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_ao(c, s, cam, &vw, W, H, dirs, 1, reset != 0, d_ao, d_out, nullptr, st);
  });
}

// No frame of the workspace: the bytes of a state alone, on the current device.
int rc_ao_resolve_device(const rc_ao_px* d_ao, int W, int H, uint8_t* d_out, void* stream) {
  const char* who = "rc_ao_resolve_device";
  if (!d_ao || !d_out) return say("Error: %s: a null pointer\n", who);
  if ((uintptr_t)d_ao & 3u) return say("Error: %s: the state is not 4-byte aligned\n", who);
  if (W <= 0 || H <= 0 ||
      ((unsigned long long)W * (unsigned long long)H / 4 + 256) / 256 > 0x7fffffffull)
    return say("Error: %s: %d x %d: both sides must be at least 1 and the image within one grid of "
               "four pixels a lane (about 2^41 pixels)\n", who, W, H);
  Entered e;
  if (enter(kCurrentDevice, false, e)) return -1;
  hipStream_t st = stream ? (hipStream_t)stream : e.c->stream;
  HIP_TRY(rc::launch_ao_resolve(d_ao, W, H, d_out, st));
  return 0;
}

int rc_render_ao(const rc_scene* s, const rc_camera* cam, const rc_window* win, int W, int H,
                 const rc_options* opt, const rc_ao_dirs* sets, int nsets, uint8_t* pixmap,
                 rc_timing* timing) {
  const char* who = "rc_render_ao";
  if (!s || !cam || !opt || !sets || !pixmap) return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  rc_window vw;
  if (ao_pass_refused(who, opt, cam, win, W, H, &vw)) return -1;
  if (nsets < 1 || nsets > 1024)
    return say("Error: %s: nsets %d is not 1..1024: a reset pass and up to 1023 further ones (a "
               "record holds 65535 rays)\n", who, nsets);
  for (int k = 0; k < nsets; ++k) {
    char buf[96];
    if (const char* why = ao_dirs_problem(&sets[k], buf, sizeof buf))
      return say("Error: %s: sets[%d] fails rc_ao_dirs_check: %s\n", who, k, why);
  }
  const size_t px = (size_t)W * H;
  return host_entry(
      opt, W, H, nullptr, timing, t0,
      "Error: out of device memory for the occlusion plane and its state (%d x %d)\n", false,
      [&](DevCtx& c) { return c.ao.state.ensure(px * sizeof(rc_ao_px)) || c.ao.plane.ensure(px); },
      [&](DevCtx& c) -> int {
        if (enqueue_ao(c, s, cam, &vw, W, H, sets, nsets, true, (rc_ao_px*)c.ao.state.p,
                       (uint8_t*)c.ao.plane.p, nullptr, c.stream))
          return -1;
        // behind the last pass on c.stream, in front of finish_host's wait
        HIP_TRY(hipMemcpyAsync(pixmap, c.ao.plane.p, px, hipMemcpyDeviceToHost, c.stream));
        return 0;
      });
}

// ---------------- the G-buffer through a camera, the guided filter, the ambient compose --
// rc_render_camera_gbuffer* behind their null checks: clauses 2 to 5 of the documented order, and
// the window the frame is shot through (win null: the whole image)
static int camera_gbuffer_refused(const char* who, const rc_options* opt, const rc_camera* cam,
                                  const rc_window* win, int W, int H, const rc_gbuffer* planes,
                                  rc_window* vw) {
  if (!planes->id && !planes->t && !planes->P && !planes->N)
    return say("Error: %s: all four planes are null: ask for at least one of id, t, P and N\n",
               who);
  *vw = win ? *win : rc_window{W, H, 0, 0};
  if (one_ray_refused(kCameraGbufferRefusal, who, opt,
                      [&] { return rc_window_check(vw, W, H, 1); }))
    return -1;
  return rc_camera_check(cam);
}

int rc_render_camera_gbuffer_device(const rc_scene* s, const rc_camera* cam, const rc_window* win,
                                    int W, int H, const rc_options* opt,
                                    const rc_gbuffer* d_planes, void* stream, rc_timing* timing) {
  const char* who = "rc_render_camera_gbuffer_device";
  if (!s || !cam || !opt || !d_planes) return say("Error: %s: a null pointer\n", who);
  rc_window vw;
  if (camera_gbuffer_refused(who, opt, cam, win, W, H, d_planes, &vw)) return -1;
  return device_entry(opt, stream, timing, false, [&](DevCtx& c, hipStream_t st) {
    return enqueue_camera_gbuffer(c, s, cam, &vw, W, H, d_planes, st);
  });
}

int rc_render_camera_gbuffer(const rc_scene* s, const rc_camera* cam, const rc_window* win, int W,
                             int H, const rc_options* opt, const rc_gbuffer* planes,
                             rc_timing* timing) {
  const char* who = "rc_render_camera_gbuffer";
  if (!s || !cam || !opt || !planes) return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  rc_window vw;
  if (camera_gbuffer_refused(who, opt, cam, win, W, H, planes, &vw)) return -1;
  const size_t px = (size_t)W * H * sizeof(float);
  return host_entry(
      opt, W, H, nullptr, timing, t0,
      "Error: out of device memory for the G-buffer's planes (%d x %d)\n", false,
      [&](DevCtx& c) {   // device copies of the planes asked for (rc_render_gbuffer's)
        GbufFrame& g = c.gbuf;
        return (planes->id && g.id.ensure(px)) || (planes->t && g.t.ensure(px)) ||
               (planes->P && g.P.ensure(3 * px)) || (planes->N && g.N.ensure(3 * px));
      },
      [&](DevCtx& c) -> int {
        const GbufFrame& g = c.gbuf;
        const rc_gbuffer d{planes->id ? (int32_t*)g.id.p : nullptr,
                           planes->t ? (float*)g.t.p : nullptr,
                           planes->P ? (float*)g.P.p : nullptr,
                           planes->N ? (float*)g.N.p : nullptr};
        if (enqueue_camera_gbuffer(c, s, cam, &vw, W, H, &d, c.stream)) return -1;
        // behind the kernel on c.stream, in front of finish_host's wait
        auto back = [&](void* host, const void* dev, size_t bytes) -> int {
          if (host) HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c.stream));
          return 0;
        };
        return back(planes->id, d.id, px) || back(planes->t, d.t, px) ||
               back(planes->P, d.P, 3 * px) || back(planes->N, d.N, 3 * px);
      });
}

static int ao_filter_make(const char* who, int radius, rc_ao_filter* out, bool tent) {
  if (!out) return say("Error: %s: a null filter\n", who);
  if (radius < 0 || radius > RC_AO_FILTER_MAX_RADIUS)
    return say("Error: %s: radius %d is not 0..%d\n", who, radius, RC_AO_FILTER_MAX_RADIUS);
  std::memset(out, 0, sizeof *out);
  out->radius = radius;
  out->nmin = 0.9f;
  out->dplane = 0.05f;
  for (int d = 0; d <= radius; ++d) out->taps[d] = (uint16_t)(tent ? radius + 1 - d : 1);
  return 0;
}

int rc_ao_filter_box(int radius, rc_ao_filter* out) {
  return ao_filter_make("rc_ao_filter_box", radius, out, false);
}

int rc_ao_filter_tent(int radius, rc_ao_filter* out) {
  return ao_filter_make("rc_ao_filter_tent", radius, out, true);
}

int rc_ao_filter_check(const rc_ao_filter* f) {
  const char* who = "rc_ao_filter_check";
  if (!f) return say("Error: %s: a null filter\n", who);
  char buf[160];
  const char* why = ao_filter_problem(f, buf, sizeof buf);
  return why ? say("Error: %s: %s\n", who, why) : 0;
}

// No scene and no frame of the workspace, like rc_ao_resolve_device.
int rc_ao_filter_device(const rc_ao_px* d_ao, const rc_gbuffer* d_guide, int W, int H,
                        const rc_ao_filter* f, uint8_t* d_out, void* stream) {
  const char* who = "rc_ao_filter_device";
  if (!d_ao || !d_guide || !f || !d_out) return say("Error: %s: a null pointer\n", who);
  if (!d_guide->id || !d_guide->P || !d_guide->N)
    return say("Error: %s: the guide needs its id, P and N planes (t is not read)\n", who);
  if ((uintptr_t)d_ao & 3u) return say("Error: %s: the state is not 4-byte aligned\n", who);
  if (guided_image_refused(who, W, H) || rc_ao_filter_check(f)) return -1;
  Entered e;
  if (enter(kCurrentDevice, false, e)) return -1;
  hipStream_t st = stream ? (hipStream_t)stream : e.c->stream;
  HIP_TRY(rc::launch_ao_filter(d_ao, d_guide->id, d_guide->P, d_guide->N, W, H, ao_filter_arg(f),
                               d_out, st));
  return 0;
}

// clause 3 of the compose: every component finite and not negative (-0 passes)
static int ambient_refused(const char* who, const float ambient[3]) {
  for (int k = 0; k < 3; ++k)
    if (!__builtin_isfinite(ambient[k]) || ambient[k] < 0.0f)
      return say("Error: %s: ambient[%d] is %g: every component must be finite and not negative\n",
                 who, k, (double)ambient[k]);
  return 0;
}

int rc_ao_compose_device(const rc_scene* s, const rc_options* opt, const int32_t* d_id,
                         const uint8_t* d_ao, const float ambient[3], const uint8_t* d_rgb_in,
                         uint8_t* d_rgb_out, int W, int H, void* stream) {
  const char* who = "rc_ao_compose_device";
  if (!s || !opt || !d_id || !d_ao || !ambient || !d_rgb_in || !d_rgb_out)
    return say("Error: %s: a null pointer\n", who);
  if (one_ray_refused(kComposeRefusal, who, opt, [] { return 0; }) ||
      ambient_refused(who, ambient) || guided_image_refused(who, W, H))
    return -1;
  Entered e;
  if (enter(kCurrentDevice, true, e)) return -1;
  hipStream_t st = stream ? (hipStream_t)stream : e.c->stream;
  return enqueue_compose(*e.c, s, d_id, d_ao, ambient, d_rgb_in, d_rgb_out, W, H, st);
}

int rc_render_ambient(const rc_scene* s, const rc_camera* cam, const rc_window* win, int W, int H,
                      const rc_options* opt, const rc_ao_dirs* sets, int nsets,
                      const rc_ao_filter* filter, const float ambient[3], uint8_t* pixmap,
                      rc_timing* timing) {
  const char* who = "rc_render_ambient";
  if (!s || !cam || !opt || !sets || !filter || !ambient || !pixmap)
    return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  rc_window vw;
  if (ao_pass_refused(who, opt, cam, win, W, H, &vw)) return -1;
  if (nsets < 1 || nsets > 1024)
    return say("Error: %s: nsets %d is not 1..1024: a reset pass and up to 1023 further ones (a "
               "record holds 65535 rays)\n", who, nsets);
  for (int k = 0; k < nsets; ++k) {
    char buf[96];
    if (const char* why = ao_dirs_problem(&sets[k], buf, sizeof buf))
      return say("Error: %s: sets[%d] fails rc_ao_dirs_check: %s\n", who, k, why);
  }
  if (guided_image_refused(who, W, H) || rc_ao_filter_check(filter) ||
      ambient_refused(who, ambient))
    return -1;
  const size_t px = (size_t)W * H;
  return host_entry(
      opt, W, H, pixmap, timing, t0,
      "Error: out of device memory for the image, the occlusion state and the guide (%d x %d)\n",
      false,
      [&](DevCtx& c) {
        GuidedFrame& g = c.guided;
        return g.state.ensure(px * sizeof(rc_ao_px)) || g.id.ensure(px * 4) ||
               g.P.ensure(px * 12) || g.N.ensure(px * 12) || g.plane.ensure(px);
      },
      [&](DevCtx& c) {
        return enqueue_ambient(c, s, cam, &vw, W, H, opt, sets, nsets, filter, ambient);
      });
}

int rc_render_filtered_device(const rc_scene* s, int W, int H, const rc_options* opt,
                              const rc_filter* f, uint8_t* d_out, void* stream,
                              rc_timing* timing) {
  const char* who = "rc_render_filtered_device";
  if (!s || !opt || !f || !d_out) return say("Error: %s: a null pointer\n", who);
  if (filtered_refused(who, opt, W, H, f)) return -1;
  return device_entry(opt, stream, timing, true, [&](DevCtx& c, hipStream_t st) {
    return enqueue_render(c, s, W, H, 0, 1, H, opt, d_out, st, true, nullptr, nullptr, f);
  });
}

int rc_render_filtered(const rc_scene* s, int W, int H, const rc_options* opt, const rc_filter* f,
                       uint8_t* pixmap, rc_timing* timing) {
  const char* who = "rc_render_filtered";
  if (!s || !opt || !f || !pixmap) return say("Error: %s: a null pointer\n", who);
  const auto t0 = HostClock::now();
  if (filtered_refused(who, opt, W, H, f)) return -1;
  return host_entry(opt, W, H, pixmap, timing, t0, nullptr, true, nothing_more, [&](DevCtx& c) {
    return enqueue_render(c, s, W, H, 0, 1, H, opt, (uint8_t*)c.out.p, c.stream, true, nullptr,
                          nullptr, f);
  });
}

// No frame of the workspace either: the filter pass alone, on the current device.
int rc_filter_image_device(const uint8_t* d_src, int W, int H, int s, const rc_filter* f,
                           uint8_t* d_dst, void* stream) {
  const char* who = "rc_filter_image_device";
  if (!d_src || !d_dst || !f) return say("Error: %s: a null pointer\n", who);
  if (rc_filter_check(f, s)) return -1;
  if (W <= 0 || H <= 0 || W > (1 << 28) / s || H > (1 << 28) / s)
    return say("Error: %s: %d x %d at factor %d: both sides must be 1 .. 2^28 / s\n", who, W, H, s);
  const uintptr_t a = (uintptr_t)d_src, b = (uintptr_t)d_dst;
  const size_t nb = (size_t)W * H * 3, na = nb * (size_t)s * s;
  if (a < b + nb && b < a + na)
    return say("Error: %s: the source and the destination overlap: every output pixel reads its "
               "neighbours' subsamples\n", who);
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  DevCtx* c;
  if (ctx_get(dev, &c)) return -1;
  HIP_TRY(rc::launch_filter_down(d_src, W, H, s, f->taps, f->ntaps, d_dst,
                                 stream ? (hipStream_t)stream : c->stream));
  return 0;
}

}  // extern "C"

