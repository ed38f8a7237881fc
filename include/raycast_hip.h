/*
 * raycast_hip.h — C-ABI of the MI355X raycast library (libraycast_hip.so).
 *
 * Drop-in boundary: the reference's render entry point
 *     void raycast(json_data_t *json_struct, PPMFormat photo_data);   // C/raycast.h:8
 * is exported with the identical signature and by-value PPMFormat, so the reference's
 * own main (C/raycast.c:19-69) links against this library instead of C/raycast.c.
 *
 * The record layouts below are byte-identical to the reference's:
 *   shape_t  (104 B)  C/objects.h:15-49
 *   light_t  ( 72 B)  C/objects.h:51-61
 *   json_data_t       C/parse.h:11-18
 *   PPMFormat         C/ppm.h:6-12
 * They sit behind the reference's own include guards (objects_h, parse_h, ppm_h): include
 * the reference headers FIRST if both are used in one translation unit.
 *
 * Everything beyond raycast() is an extension: explicit options (mode, bounce depth, GPU
 * count), a reusable packed scene, and device-resident rendering for benchmarks and the
 * multi-GPU driver.  No torch types cross this boundary: plain pointers and sizes only.
 */
#ifndef RAYCAST_HIP_H
#define RAYCAST_HIP_H

#include <stdio.h>
#include <stdint.h>
#include <stdbool.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- reference record layouts (ABI) ------------------------------------------------- */
#ifndef objects_h
#define objects_h
typedef enum { SPHERE, PLANE, QUADRIC } shape_type_t;        /* C/objects.h:4-8   */
typedef enum { POINT, SPOTLIGHT } light_type_t;               /* C/objects.h:10-13 */

typedef struct shape_t {                                      /* C/objects.h:15-49 */
  float diffuse_color[3];
  float specular_color[3];
  float position[3];
  float reflectivity;
  float refractivity;
  float ior;
  union {
    struct { float normal[3]; };                              /* plane   */
    struct { float radius; };                                 /* sphere  */
    struct { float a, b, c, d, e, f, g, h, i, j; };           /* quadric */
  };
  shape_type_t type;
  struct shape_t *next;
} shape_t;

typedef struct light_t {                                      /* C/objects.h:51-61 */
  float position[3];
  float color[3];
  float radial_coef[3];
  float theta;
  float cos_theta;
  float a0;
  float direction[3];
  light_type_t type;
  struct light_t *next;
} light_t;

/* list builders of the host front end (same names/semantics as C/objects.c:20-221) */
shape_t *add_new_sphere(shape_t *head, float *diffuse, float *specular, float *position,
                        float radius, float reflectivity, float refractivity, float ior);
shape_t *add_new_plane(shape_t *head, float *diffuse, float *specular, float *position,
                       float *normal, float reflectivity);
shape_t *add_new_quadric(shape_t *head, float *diffuse, float *specular, float a, float b,
                         float c, float d, float e, float f, float g, float h, float i,
                         float j, float reflectivity);
shape_t *free_shape_list(shape_t *head);
light_t *free_light_list(light_t *head);
light_t *add_new_spot_light(light_t *head, float *color, float *position, float theta,
                            float a0, float *direction, float *radial_coef);
light_t *add_new_point_light(light_t *head, float *color, float *position, float *radial_coef);
#endif

#ifndef parse_h
#define parse_h
typedef struct json_data_t {                                  /* C/parse.h:11-18 */
  float camera_width;
  float camera_height;
  shape_t *shapes_list;
  light_t *lights_list;
  int num_shapes;
  int num_lights;
} json_data_t;

/* scene front end (same grammar, messages and exit(1) behaviour as C/parse.c:13-436) */
void parse_json(FILE *json, json_data_t *json_data);
void set_to_black(float *input);
#endif

#ifndef ppm_h
#define ppm_h
typedef struct PPMFormat {                                    /* C/ppm.h:6-12 */
  int width, height, size;
  uint8_t maxColor;
  uint8_t depth;
  char *tupleType;
  uint8_t *pixmap;
} PPMFormat;

void ppm_WriteOutP3(PPMFormat inData, FILE *outFile);        /* C/ppm.c:168-184 */
float ppm_clamp(float value, float lower_bound, float upper_bound);  /* C/ppm.c:350-359 */
#endif

_Static_assert(sizeof(shape_t) == 104, "shape_t must match C/objects.h layout");
_Static_assert(sizeof(light_t) == 72, "light_t must match C/objects.h layout");

/* ---- drop-in entry point ------------------------------------------------------------ */

/* Replaces C/raycast.c:79-130.  Consumes both lists exactly like the reference
 * (C/raycast.c:104-107: frees them; num_shapes/num_lights stay valid; the list pointers are
 * left NULL instead of dangling).  Writes every byte of photo_data.pixmap (W*H*3, RGB,
 * row-major, top row first).  Options come from the environment:
 *   RAYCAST_MODE   = parity (default) | fast
 *   RAYCAST_DEPTH  = bounce depth d, MAX_RECURSION = d+1 (default 6 == C/raycast.c:14)
 *   RAYCAST_GPUS   = number of GPUs for row-cyclic sharding over RCCL (default 1; both modes)
 *   RAYCAST_DEVICE = first HIP device ordinal (default 0)
 *   RAYCAST_SSAA   = supersampling factor 1 (default) | 2 | 4 | 8 (rc_options.ssaa; any other
 *                    value: a warning, then 1)
 *   RAYCAST_SSAA_ADAPTIVE = contrast threshold t, 1..255: supersample only the edge pixels
 *                    (RC_SSAA_ADAPTIVE below; fast mode, RAYCAST_SSAA 2, 4 or 8).  Any other
 *                    value: a warning, then off; set while the factor is 1: a warning, ignored
 *   RAYCAST_FILTER = box (default) | tent: the reconstruction filter of RAYCAST_SSAA 2, 4 or 8
 *                    (rc_filter below).  With RAYCAST_SSAA 1 or RAYCAST_SSAA_ADAPTIVE: a
 *                    warning, ignored; any other value: a warning, then box
 *   RAYCAST_PATTERN = name | name:t: a sparse sample pattern (rc_pattern below; diag2, rgss4,
 *                    checker8 or queens8) for every pixel, or with a contrast threshold t in
 *                    1..255 for the edge pixels only; fast and cuda mode, RAYCAST_SSAA unset or
 *                    1.  An unknown name, a bad t, parity mode or RAYCAST_SSAA 2, 4 or 8 set as
 *                    well: a warning, ignored
 *   RAYCAST_WINDOW = FWxFH+X0+Y0: the image asked for is the window at (X0, Y0) of the FW x FH
 *                    image (rc_window below; fast and cuda mode, RAYCAST_SSAA 1, 2, 4 or 8).
 *                    Malformed, parity mode, RAYCAST_SSAA_ADAPTIVE, RAYCAST_PATTERN,
 *                    RAYCAST_FILTER=tent, RAYCAST_GPUS > 1 or a window the image does not hold:
 *                    a warning, ignored
 *   RAYCAST_STATS = 1: one JSON metrics line on stderr
 * Any HIP failure prints a message to stderr and exit(1)s (reference error convention). */
void raycast(json_data_t *json_struct, PPMFormat photo_data);

/* ---- extended API ------------------------------------------------------------------- */

enum { RC_MODE_PARITY = 0,  /* byte-identical to gcc -O3 C/raycast.c (scan-order carry)   */
       RC_MODE_FAST   = 1,  /* reflection miss ends the bounce loop (CUDA/raycast.cu:224-237) */
       RC_MODE_CUDA   = 2   /* the CUDA port's semantics: fast's control flow, powf-on-float
                               arithmetic (CUDA/raycast.cu:455-634, v3math.cu:168), 50 bounces
                               by default (MAX_ITER, CUDA/raycast.cu:13); parity unpinned */ };

typedef struct rc_options {
  int max_recursion;   /* C/raycast.c:14 MAX_RECURSION; bounce depth = max_recursion - 1 */
  int mode;            /* RC_MODE_* */
  int num_gpus;        /* >= 1 */
  int device;          /* first device ordinal */
  int ssaa;            /* supersampling factor s: 1 (off; 0 means the same, so zero-initialised
                          options keep one ray per pixel), 2, 4 or 8, alone or with an adaptive
                          threshold t in bits 8..15 (RC_SSAA_ADAPTIVE(s, t), below); anything
                          else is refused */
} rc_options;
_Static_assert(sizeof(rc_options) == 20, "rc_options layout (ctypes binding)");

/* rc_options.ssaa = s | (t << 8): the factor s and the adaptive contrast threshold t (0: every
 * pixel is supersampled, the plain ssaa below).  A value decodes when s is 0, 1, 2, 4 or 8, t is
 * 0..255 and no higher bit is set; t > 0 needs s >= 2.  Everything else is refused. */
#define RC_SSAA_ADAPTIVE(s, t) ((int)(s) | ((int)(t) << 8))
#define RC_SSAA_FACTOR(v)      ((int)(v) & 0xff)
#define RC_SSAA_THRESHOLD(v)   (((int)(v) >> 8) & 0xff)

/* Supersampled anti-aliasing (ssaa = s > 1).  Let B be the s*W x s*H image the same scene,
 * mode and depth produce with ssaa = 1: the camera of that size (pw = cam_w / (float)(s*W),
 * ph = cam_h / (float)(s*H), C/raycast.c:109-110), quantised uint8 samples.  The W x H output
 * is B's box filter in integers, rounded to nearest:
 *     out[y][x][c] = (sum over j < s, i < s of B[s*y + j][s*x + i][c]  +  s*s/2) / (s*s)
 * so an anti-aliased image is an exact function of the reference's own s*W x s*H image.
 * In parity mode B is the reference's parity image of that size (scan-order carry and
 * phantom included); in fast / cuda mode it is that mode's image.  rc_timing.zero_normalize
 * and dep_pixels are those of B.  Fast mode shoots the s*s subsamples of a pixel on adjacent
 * lanes and reduces them in registers (B is never stored); parity and cuda modes render B
 * into a buffer of the device context and box-filter it on the device.
 * rc_render, rc_render_device and raycast() honour ssaa in every mode (rc_render_device's
 * row0 / row_step / nrows stay in output rows; parity and cuda need row_step == 1 with s > 1);
 * rc_frame_submit honours it in fast and cuda mode and refuses parity frames with s > 1;
 * num_gpus > 1 and rc_render_sharded refuse s > 1. */

/* Adaptive supersampling (ssaa = RC_SSAA_ADAPTIVE(s, t), s in {2, 4, 8}, t in 1..255; fast and
 * cuda mode).  Fix the scene, mode, depth, W and H, and let
 *   A  be the W x H image of that mode with ssaa = 1,
 *   F  be the W x H image of that mode with ssaa = s (the box filter above, t = 0),
 *   contrast(x, y) = the maximum over the three channels of max - min of A's bytes over the 3 x 3
 *                    window centred on (x, y), clipped to the image (a 1 x 1 image: 0).
 * Then  out[y][x] = F[y][x] if contrast(x, y) >= t, else A[y][x].
 * The contrast is computed on A's quantised bytes, in integers, so the output is an exact
 * function of two images the reference's arithmetic defines and does not depend on any
 * execution order.  On the device: A is rendered into the output, one kernel lists the pixels
 * with contrast >= t (in no particular order), and a third shoots the s*s subsamples of the
 * listed pixels only, on adjacent lanes, and stores their box filter over A's pixel.  The three
 * are separate launches on one stream: the list is complete before any pixel its neighbours'
 * contrast was read from is overwritten.  rc_timing.zero_normalize counts the rays actually
 * shot (A's and the refined subsamples').
 * rc_render, rc_render_device, raycast() and rc_frame_submit honour it in fast and cuda mode.
 * Refused, each with a message: parity mode (every pixel of its s*W x s*H image depends on the
 * scan-order carry of the whole image, so it cannot be shot sparsely; plain ssaa remains);
 * rc_render_device with anything but the whole image (row0 = 0, row_step = 1, nrows = H: the
 * contrast needs the neighbouring rows); t > 0 with s < 2; num_gpus > 1 and rc_render_sharded
 * (by the factor, like plain ssaa); W * H >= 2^32. */
typedef struct rc_adaptive_stats {
  int64_t refined_pixels;   /* pixels with contrast >= t          */
  int64_t rays;             /* W*H + s*s*refined_pixels           */
} rc_adaptive_stats;
/* The last adaptive frame enqueued on the current device: waits for that frame, then reads its
 * count.  Returns -1 if there was none. */
int rc_adaptive_stats_get(rc_adaptive_stats *out);
/* The kernel spans (ms, HIP events) of the last adaptive frame rendered with timing (rc_render,
 * rc_render_device with a timing record) on the current device: ms[0] the one-ray image, ms[1]
 * the edge list, ms[2] the refinement.  Returns -1 if there was none. */
int rc_adaptive_phase_ms(double ms[3]);

/* Variable-rate supersampling from the caller's per-pixel rate map (rc_render_rates,
 * rc_render_rates_device; fast and cuda mode).  Fix the scene, mode, depth, W and H, and let
 *   F_1  be the W x H image of that mode with ssaa = 1,
 *   F_s  for s in {2, 4, 8} be its image with ssaa = s (the box filter above),
 *   R    be the rate map: W*H bytes, row-major, top row first.
 * Then
 *   R[y][x] in {1, 2, 4, 8}:  out[y][x] = F_{R[y][x]}[y][x]
 *   R[y][x] == 0           :  the three bytes of out[y][x] are not stored to (they keep what
 *                             the caller's buffer held)
 *   any other value        :  invalid: rc_render_rates checks the map on the host before it
 *                             enqueues anything, prints a message and returns -1 with the
 *                             pixmap unchanged; rc_render_rates_device cannot see the bytes, so
 *                             such a pixel is treated as rate 0 and counted in
 *                             rc_rate_stats.invalid.
 * Every output byte is an exact function of images the reference's arithmetic defines and does
 * not depend on any execution order.  On the device: one kernel shoots the rate-1 pixels and
 * bins the others into one list per factor (in no particular order), then each list's pixels
 * get their s*s subsamples, on adjacent lanes, and the box filter of those is stored; all
 * launches go to one stream with no host wait in between, so a map written on that stream just
 * before the call is honoured.  The lists take 8 * W * H bytes of device memory.
 * rc_options: mode fast or cuda; ssaa 0 or 1 (the map carries the factor); max_recursion as
 * everywhere.  rc_timing.zero_normalize counts the rays actually shot, kernel_ms covers both
 * stages.  The refinement's grids follow rc_tuning.adaptive_blocks.
 * Refused, each with a message and -1: parity mode (every pixel of its s*W x s*H image depends
 * on the scan-order carry of the whole image, so it cannot be shot sparsely); an ssaa factor
 * above 1 or a threshold in the options; num_gpus > 1; null pointers; W * H >= 2^32, 8 * W or
 * 8 * H past INT_MAX, or more than 65535 rows of 16-pixel tiles.
 * raycast(), rc_render, rc_render_device and rc_frame_submit take no rate map. */
typedef struct rc_rate_stats {
  int64_t pixels[4];   /* pixels with rate 1, 2, 4, 8                          */
  int64_t invalid;     /* map bytes outside {0,1,2,4,8} (treated as 0)         */
  int64_t rays;        /* pixels[0] + 4*pixels[1] + 16*pixels[2] + 64*pixels[3] */
} rc_rate_stats;
_Static_assert(sizeof(rc_rate_stats) == 48, "rc_rate_stats layout (ctypes binding)");
/* The last rate-map frame enqueued on the current device: waits for that frame, then reads its
 * counters.  Returns -1 if there was none. */
int rc_rate_stats_get(rc_rate_stats *out);
/* The kernel spans (ms, HIP events) of the last rate-map frame on the current device: ms[0] the
 * rate-1 pass with the binning, ms[1] the refinement.  Returns -1 if there was none. */
int rc_rate_phase_ms(double ms[2]);

typedef struct rc_timing {
  double total_ms;       /* whole call, host wall clock                                 */
  double kernel_ms;      /* sum of kernel spans (HIP events)                            */
  double resolve_ms;     /* parity: carry-chain resolution span                        */
  double d2h_ms;         /* device -> host copy of the pixmap                          */
  int64_t dep_pixels;    /* parity: pixels whose first reflection missed               */
  int64_t zero_normalize;/* count of zero-length normalize events (C/v3math.c:183-187) */
  int64_t frames_checked;/* parity frames whose hand-off words were read back: rc_frames_wait
                            (every frame since the previous wait), rc_render_device with
                            timing (1)                                                  */
  int64_t frames_failed; /* of them, frames whose carry hand-off failed (image invalid)  */
} rc_timing;

/* Fill *opt with the defaults (ssaa = 1), then the RAYCAST_* environment overrides if use_env
 * (a RAYCAST_SSAA other than 1, 2, 4 or 8 prints a warning and leaves 1; RAYCAST_SSAA_ADAPTIVE =
 * 1..255 with a factor of 2, 4 or 8 gives RC_SSAA_ADAPTIVE(factor, t), any other value prints a
 * warning and means off, and with a factor of 1 it prints a warning and is ignored). */
void rc_default_options(rc_options *opt, int use_env);

/* Opaque packed scene: flattened shape/light arrays + the out-of-bounds "phantom" record
 * the reference reads as shapes_list[-1] (C/raycast.c:382).  Does NOT consume the lists. */
typedef struct rc_scene rc_scene;
rc_scene *rc_scene_create(const json_data_t *json_struct);
void rc_scene_destroy(rc_scene *scene);
/* 1 when the reference output is well defined for this scene (phantom reads only defined
 * bytes or is black), 0 when the reference itself is run-to-run nondeterministic. */
int rc_scene_parity_defined(const rc_scene *scene);

/* Render W x H into a host pixmap (W*H*3 bytes).  Returns 0 on success. */
int rc_render(const rc_scene *scene, int width, int height, const rc_options *opt,
              uint8_t *pixmap, rc_timing *timing);

/* Device-resident render on the current device: rows row0, row0+row_step, ... (nrows rows)
 * of a W x H image into d_out (nrows*W*3 bytes, device memory, compact row order) on the
 * given HIP stream (NULL = default stream).  Parity mode requires row0=0,row_step=1,nrows=H.
 * Asynchronous unless timing is requested.  Returns 0 on success. */
int rc_render_device(const rc_scene *scene, int width, int height, int row0, int row_step,
                     int nrows, const rc_options *opt, uint8_t *d_out, void *stream,
                     rc_timing *timing);

/* Variable-rate supersampling (the rate-map contract above, at rc_rate_stats).
 * rc_render_rates: host map (W*H bytes), host pixmap (W*H*3 bytes, in/out: the bytes of rate-0
 * pixels are unchanged on return); synchronous, on opt->device.
 * rc_render_rates_device: device map, device image, on the current device and the given HIP
 * stream (NULL = default stream); asynchronous unless timing is requested.
 * Both return 0 on success. */
int rc_render_rates(const rc_scene *scene, int width, int height, const rc_options *opt,
                    const uint8_t *rates, uint8_t *pixmap, rc_timing *timing);
int rc_render_rates_device(const rc_scene *scene, int width, int height, const rc_options *opt,
                           const uint8_t *d_rates, uint8_t *d_out, void *stream,
                           rc_timing *timing);

/* Separable reconstruction filters for supersampling (rc_render_filtered,
 * rc_render_filtered_device, rc_filter_image_device; every mode).  Plain ssaa ends in the box
 * filter over a pixel's own s x s subsamples; a wider filter lets a subsample contribute to the
 * neighbouring pixels as well, at no extra ray.  Fix the scene, mode, depth, W, H and s in
 * {2, 4, 8}, and let B be the s*W x s*H image of that mode with ssaa = 1 (the B of the ssaa
 * contract above: in parity mode the carry and the phantom included).  A filter is a 1-D integer
 * tap vector k[0..L):
 *     L = s + 2h with a halo 0 <= h <= s   (so s <= L <= 3s <= 24, and L - s is even)
 *     int16 taps, negative ones allowed;  S = sum k > 0;  sum |k| <= 2048
 * applied along x and along y, with B's coordinates clamped to the image (edge replicate):
 *     acc[y][x][c] = sum over j < L, i < L of
 *                    k[j] * k[i] * B[clamp(s*y - h + j, 0, s*H - 1)][clamp(s*x - h + i, 0, s*W - 1)][c]
 *     out[y][x][c] = clamp(floor((acc + S*S/2) / (S*S)), 0, 255)     (integers; S*S/2 rounds down)
 * so a filtered image is still an exact integer function of the reference's own s*W x s*H image.
 * The bound on sum |k| keeps it in int32: a horizontal sum is at most 2048 * 255 < 2^19 in
 * magnitude, acc + S*S/2 at most 2048^2 * 255 + 2^21 < 2^31, so the separable evaluation (rows,
 * then columns) is exact.  A negative acc + S*S/2 clamps to 0 whatever the division's rounding.
 * Built-in vectors: box, h = 0, k = [1]*s (the output equals rc_options.ssaa = s byte for byte);
 * tent, h = s/2, k = [1, 3, .., 2s-1, 2s-1, .., 3, 1], S = 2*s*s (the tent of radius one output
 * pixel sampled at the subsample centres, times 2).  Anything else is the caller's.
 * On the device: B is rendered into a buffer of the device context in every mode (two passes;
 * fast mode's fused kernel has no counterpart here), then one kernel stages each output tile's
 * subsamples and halo in LDS once, filters the rows into int32 partial sums and then the
 * columns.  rc_timing.zero_normalize and dep_pixels are those of B.
 * rc_options: ssaa = s, a plain factor of 2, 4 or 8; mode and max_recursion as everywhere.
 * Whole images only (the halo needs the neighbouring rows).
 * Refused, each with a message and -1, from the arguments alone (before any device work): a
 * filter that fails rc_filter_check; a factor other than 2, 4 or 8; an adaptive threshold in
 * opt->ssaa; num_gpus > 1; null pointers; W or H above 2^28 / s; rc_filter_image_device with
 * overlapping source and destination (d_src == d_dst included).
 * rc_render, rc_render_device, rc_frame_submit, rc_render_sharded, adaptive supersampling and
 * rate maps take no filter and stay as they are: a refined pixel's filter footprint would
 * reach its unrefined neighbours' subsamples, which those paths never shoot.  raycast() takes
 * the tent through RAYCAST_FILTER:
 *   RAYCAST_FILTER = box (default) | tent: the reconstruction filter of RAYCAST_SSAA 2, 4 or 8.
 *                    With RAYCAST_SSAA 1 or with RAYCAST_SSAA_ADAPTIVE: a warning, ignored.  Any
 *                    other value: a warning, then box. */
#define RC_FILTER_MAX_TAPS 24
typedef struct rc_filter {
  int32_t ntaps;                       /* L                             */
  int16_t taps[RC_FILTER_MAX_TAPS];    /* k[0..L); the rest is ignored   */
} rc_filter;
_Static_assert(sizeof(rc_filter) == 52, "rc_filter layout (ctypes binding)");
/* The built-in tap vectors for s = 2, 4 or 8 (-1 for any other s, or a null out). */
int rc_filter_box(int s, rc_filter *out);
int rc_filter_tent(int s, rc_filter *out);
/* 0 when *f is a valid filter at factor s, else -1 with a message naming the rule broken. */
int rc_filter_check(const rc_filter *f, int s);
/* raycast()'s reading of RAYCAST_FILTER against the options rc_default_options(.., 1) gave: 1
 * and the tent of the options' factor in *out when the frame goes through rc_render_filtered, 0
 * when it goes through rc_render (unset, box, or ignored with one of the warnings above). */
int rc_filter_env(const rc_options *opt, rc_filter *out);
/* rc_render_filtered: host pixmap (W*H*3 bytes), synchronous, on opt->device.
 * rc_render_filtered_device: device image on the current device and the given HIP stream (NULL:
 * the library's stream of that device, as rc_render_device); asynchronous unless timing is
 * requested.  Both return 0 on success. */
int rc_render_filtered(const rc_scene *scene, int width, int height, const rc_options *opt,
                       const rc_filter *filter, uint8_t *pixmap, rc_timing *timing);
int rc_render_filtered_device(const rc_scene *scene, int width, int height,
                              const rc_options *opt, const rc_filter *filter, uint8_t *d_out,
                              void *stream, rc_timing *timing);
/* The filter pass alone, on any device image whatever rendered it: d_dst (W x H x 3 bytes) <-
 * d_src (s*W x s*H x 3 bytes), both compact RGB in device memory, on the given stream (NULL as
 * above); asynchronous.  A caller that keeps B can filter it again with other taps. */
int rc_filter_image_device(const uint8_t *d_src, int width, int height, int s,
                           const rc_filter *filter, uint8_t *d_dst, void *stream);
/* The kernel spans (ms, HIP events) of the last timed two-pass supersampled frame on the current
 * device — a filtered frame, or a plain ssaa frame of the two-pass path (parity and cuda mode,
 * fast mode with rc_tuning.ssaa_fused = 0), whose second pass is the box filter: ms[0] B's
 * render, ms[1] the filter.  Returns -1 if there was none. */
int rc_filter_phase_ms(double ms[2]);

/* Sparse sample patterns for supersampling (rc_render_pattern, rc_render_pattern_device; fast and
 * cuda mode).  Plain ssaa, adaptive refinement and the rate map shoot the full s x s ordered grid
 * of every pixel they refine.  A rotated-grid or N-rooks pattern takes n samples of a g x g
 * subsample lattice with no two in one row or column: on a near-horizontal or near-vertical edge
 * it resolves g coverage levels with n rays where the ordered grid needs g*g.
 * Fix the scene, mode, depth, W and H.  A pattern is (g, n, px[0..n), py[0..n)) with
 *     g in {2, 4, 8};  n in {2, 4, 8, 16} and n <= g*g;  every px[k] < g and py[k] < g;
 *     the n pairs (px[k], py[k]) pairwise distinct
 * (x to the right and y downwards, as image coordinates).  Let B_g be that mode's g*W x g*H image
 * with ssaa = 1 (the B of the ssaa contract above, at s = g).  Then
 *     P[y][x][c] = (sum over k < n of B_g[g*y + py[k]][g*x + px[k]][c]  +  n/2) / n    (integers)
 * so a pattern image is still an exact integer function of the reference's own g*W x g*H image.
 * A threshold t in 0..255 selects the pixels: t = 0: out = P.  t > 0: out = P where
 * contrast(x, y) >= t, else A, with A the one-ray image and contrast exactly the adaptive
 * contract's above (rc_adaptive_stats).  The full patterns (every lattice point once: g = 2 with
 * n = 4, g = 4 with n = 16) give the bytes of rc_options.ssaa = g.
 * Built-in patterns (rc_pattern_builtin), as (x, y) pairs:
 *     diag2     g 2   (0,0) (1,1)
 *     rgss4     g 4   (1,0) (3,1) (0,2) (2,3)                      rotated-grid supersampling
 *     checker8  g 4   the eight (i, j) with i + j even, row by row
 *     queens8   g 8   row r has column [3,6,2,7,1,4,0,5][r]       no shared row, column, diagonal
 * On the device: n lanes a pixel, a lane's lattice position out of two 64-bit words of 4-bit
 * entries held in scalar registers, the quantised channels summed over the n lanes in registers;
 * B_g is never stored.  t = 0 is one kernel over tiles of 256 / n output pixels.  t > 0 is three
 * launches on one stream with no host wait: A by the plain kernel, the adaptive path's edge list,
 * then the pattern kernel striding over the list (its grid follows rc_tuning.adaptive_blocks).
 * rc_options: mode fast or cuda; ssaa 0 or 1 (the pattern carries the grid, as the rate map
 * does); max_recursion as everywhere.  rc_timing.zero_normalize counts the rays actually shot.
 * Whole images only.
 * Refused, each with a message and -1, from the arguments alone (before any device work): parity
 * mode (every pixel of its g*W x g*H image depends on the scan-order carry of the whole image, so
 * it cannot be shot sparsely; plain ssaa remains); a pattern that fails rc_pattern_check; a factor
 * above 1 or a threshold in opt->ssaa; a threshold outside 0..255; num_gpus > 1; null pointers;
 * W or H above 2^28 / g (or below 1); with t > 0, W * H >= 2^32; an image of more than 65535
 * rows of tiles (t = 0: tiles of 8, 8, 4, 4 rows at n = 2, 4, 8, 16; t > 0: of 16 rows).
 * rc_render, rc_render_device, rc_frame_submit, rc_render_sharded, the rate-map and the filtered
 * entry points take no pattern and stay as they are.  raycast() takes a built-in one through
 *   RAYCAST_PATTERN = name | name:t   (name: diag2, rgss4, checker8, queens8; t: 0..255, default 0)
 *                    in fast and cuda mode with RAYCAST_SSAA unset or 1.  An unknown name, a bad
 *                    t, parity mode, or RAYCAST_SSAA 2, 4 or 8 set as well: a warning, ignored. */
#define RC_PATTERN_MAX_SAMPLES 16
typedef struct rc_pattern {
  int32_t grid, nsamples;                 /* g and n                                  */
  uint8_t x[RC_PATTERN_MAX_SAMPLES];      /* px[0..n); the rest is ignored            */
  uint8_t y[RC_PATTERN_MAX_SAMPLES];      /* py[0..n)                                 */
} rc_pattern;
_Static_assert(sizeof(rc_pattern) == 40, "rc_pattern layout (ctypes binding)");
/* The built-in pattern of that name into *out: 0, or -1 for an unknown name or a null pointer. */
int rc_pattern_builtin(const char *name, rc_pattern *out);
/* 0 when *p is a valid pattern, else -1 with a message naming the rule broken. */
int rc_pattern_check(const rc_pattern *p);
/* raycast()'s reading of RAYCAST_PATTERN against the options rc_default_options(.., 1) gave: 1,
 * the pattern in *out and the threshold in *threshold when the frame goes through
 * rc_render_pattern; 0 when it goes through rc_render (unset, or ignored with one of the warnings
 * above). */
int rc_pattern_env(const rc_options *opt, rc_pattern *out, int *threshold);
/* rc_render_pattern: host pixmap (W*H*3 bytes), synchronous, on opt->device.
 * rc_render_pattern_device: device image on the current device and the given HIP stream (NULL:
 * the library's stream of that device, as rc_render_device); asynchronous unless timing is
 * requested.  Both return 0 on success. */
int rc_render_pattern(const rc_scene *scene, int width, int height, const rc_options *opt,
                      const rc_pattern *pattern, int threshold, uint8_t *pixmap,
                      rc_timing *timing);
int rc_render_pattern_device(const rc_scene *scene, int width, int height, const rc_options *opt,
                             const rc_pattern *pattern, int threshold, uint8_t *d_out,
                             void *stream, rc_timing *timing);
typedef struct rc_pattern_stats {
  int64_t refined_pixels;   /* t = 0: W*H; t > 0: pixels with contrast >= t              */
  int64_t rays;             /* t = 0: n*W*H; t > 0: W*H + n*refined_pixels               */
} rc_pattern_stats;
/* The last pattern frame enqueued on the current device; with a threshold it waits for that
 * frame, then reads its count.  Returns -1 if there was none. */
int rc_pattern_stats_get(rc_pattern_stats *out);
/* The kernel spans (ms, HIP events) of the last pattern frame on the current device.  t = 0:
 * ms[0] the pattern kernel, ms[1] = ms[2] = 0.  t > 0: ms[0] the one-ray image, ms[1] the edge
 * list, ms[2] the refinement.  Returns -1 if there was none. */
int rc_pattern_phase_ms(double ms[3]);

/* Progressive supersampling: samples accumulated across calls (rc_accum_pass_device,
 * rc_render_accum; fast and cuda mode).  Every other sampling entry shoots all of a pixel's
 * samples in one call, stores the rounded mean and keeps nothing.  Here the caller keeps the sums,
 * so a one-ray image exists after one ray a pixel and every later pass refines it, by any number
 * of samples (3, 5, 11, ...), everywhere or only where the image as it stands has an edge.
 * Fix the scene, the mode, the depth, W, H and a lattice g in {2, 4, 8}.  Let B_g be that mode's
 * g*W x g*H image with ssaa = 1 (the B of the ssaa contract above, at s = g).
 * State: one rc_accum_px per pixel, row-major, top row first, owned by the caller (device memory,
 *     8-byte aligned).  sum[c] is the sum of the n sample bytes taken so far; n <= 256, so
 *     sum <= 256 * 255 = 65280 fits.  The layout is public: save it, restore it, inspect it.
 * Resolve: res(sum, n)[c] = (sum[c] + n/2) / n in integers (n/2 rounds down); n = 0: (0, 0, 0).
 * Sample sequence: rc_sample_seq, (g, nsamples, x[], y[]) with g in {2, 4, 8},
 *     1 <= nsamples <= min(64, g*g), every point on the lattice and the points pairwise distinct
 *     (x to the right, y downwards).  Built in (rc_sample_seq_builtin): the four pattern names
 *     (diag2, rgss4, checker8, queens8: rc_pattern_builtin's points in its order) and hier2,
 *     hier4, hier8, the whole lattice coarse to fine: with lg = log2 g, point k is the
 *     bit-reversal r of k over 2*lg bits, x takes r's even bits (bit 2i of r is bit i of x) and y
 *     its odd bits.  hier2: (0,0) (0,1) (1,0) (1,1).  hier4: (0,0) (0,2) (2,0) (2,2) (0,1) (0,3)
 *     (2,1) (2,3) ...  hier8: (0,0) (0,4) (4,0) (4,4) (0,2) (0,6) (4,2) (4,6) ...
 * A pass is (seq, first, count, threshold t, reset) on (acc, out), with 1 <= count <= 16 and
 *     first + count <= nsamples.  The active set M is fixed once, from what `out` holds on entry:
 *       reset = 1:            M is every pixel, acc is not read and counts as zero, t must be 0;
 *       reset = 0, t = 0:     M is every pixel;
 *       reset = 0, t 1..255:  M = {contrast(out on entry)(x, y) >= t}, contrast exactly the
 *                             adaptive contract's above (3 x 3 window clipped to the image, the
 *                             maximum over the three channels).
 *     For each pixel p of M: if n + count > 256, p is saturated: nothing of it changes and it is
 *     counted.  Otherwise
 *       sum[c] += sum over k in [first, first + count) of B_g[g*y + y[k]][g*x + x[k]][c],
 *       n += count, and out[p] = res(sum, n).
 *     Pixels outside M keep their acc and out bytes; they are not stored to.
 * So after a reset pass and further t = 0 passes that together cover seq[0..k), in any split into
 * calls, out is the k-sample mean; for a pattern's own n that is rc_render_pattern's image, and
 * for all g*g points of hier<g> it is the ssaa = g image.  Every byte stays an exact integer
 * function of the reference's own g*W x g*H image.
 * On the device: one lane a pixel shoots the pass's samples one after the other (the positions in
 * scalar registers, as the pattern kernels'), then one 8-byte load, the add and one 8-byte store
 * of the record.  t = 0 is one kernel over k_render's tiles.  t > 0 is two launches on one stream
 * with no host wait: the adaptive path's edge list over `out`, then the accumulation kernel
 * striding over the list (its grid follows rc_tuning.adaptive_blocks), so an acc or out written
 * on that stream just before the call is honoured.
 * rc_options: mode fast or cuda; ssaa 0 or 1 (the sequence carries the grid); max_recursion as
 * everywhere.  rc_timing.zero_normalize counts the rays actually shot.  Whole images only.
 * Refused, each with a message and -1, from the arguments alone (before any device work): parity
 * mode (every pixel of its g*W x g*H image depends on the scan-order carry of the whole image, so
 * it cannot be shot sparsely); a factor above 1 or a threshold in opt->ssaa; num_gpus > 1; a
 * sequence that fails rc_sample_seq_check; first, count or dense out of range; a threshold outside
 * 0..255; reset with t > 0; null pointers, or an accumulator that is not 8-byte aligned; W or H
 * below 1 or above 2^28 / g; with t > 0, W * H >= 2^32; an image of more than 65535 rows of tiles
 * (16 rows each).
 * raycast(), rc_render, rc_frame_submit, rc_render_sharded and the other sampling entries take no
 * accumulator, and no RAYCAST_* variable selects one: state that lives across calls has no
 * meaning for the one-call drop-in. */
typedef struct rc_accum_px {
  uint16_t sum[3];   /* per channel, the sum of the n sample bytes */
  uint16_t n;        /* samples taken, 0..256                      */
} rc_accum_px;
_Static_assert(sizeof(rc_accum_px) == 8, "rc_accum_px layout (the kernels' 8-byte record)");
#define RC_ACCUM_MAX_SAMPLES 64
typedef struct rc_sample_seq {
  int32_t grid, nsamples;                /* g and the sequence's length        */
  uint8_t x[RC_ACCUM_MAX_SAMPLES];       /* x[0..nsamples); the rest is ignored */
  uint8_t y[RC_ACCUM_MAX_SAMPLES];       /* y[0..nsamples)                      */
} rc_sample_seq;
_Static_assert(sizeof(rc_sample_seq) == 136, "rc_sample_seq layout (ctypes binding)");
/* The built-in sequence of that name into *out: 0, or -1 for an unknown name or a null pointer. */
int rc_sample_seq_builtin(const char *name, rc_sample_seq *out);
/* 0 when *s is a valid sequence, else -1 with a message naming the rule broken. */
int rc_sample_seq_check(const rc_sample_seq *s);
/* One pass on the current device and the given HIP stream (NULL: the library's stream of that
 * device, as rc_render_device); asynchronous unless timing is requested.  d_acc: W*H records,
 * d_out: W*H*3 bytes, both device memory. */
int rc_accum_pass_device(const rc_scene *scene, int width, int height, const rc_options *opt,
                         const rc_sample_seq *seq, int first, int count, int threshold, int reset,
                         rc_accum_px *d_acc, uint8_t *d_out, void *stream, rc_timing *timing);
/* out = res(acc) for every pixel, nothing shot: for a restored state.  Asynchronous, on the
 * current device and the given stream (NULL as above). */
int rc_accum_resolve_device(const rc_accum_px *d_acc, int width, int height, uint8_t *d_out,
                            void *stream);
/* The host-pixmap form, synchronous on opt->device, the accumulator owned by the library:
 * samples [0, dense) go to every pixel (a reset pass, in chunks of at most 16), then one
 * single-sample pass with threshold t for each of seq[dense..nsamples) (t = 0: every pass takes
 * every pixel).  1 <= dense <= nsamples. */
int rc_render_accum(const rc_scene *scene, int width, int height, const rc_options *opt,
                    const rc_sample_seq *seq, int dense, int threshold, uint8_t *pixmap,
                    rc_timing *timing);
typedef struct rc_accum_stats {
  int64_t passes;          /* launch groups of the call (rc_accum_pass_device: 1)          */
  int64_t active_pixels;   /* |M| of the last pass                                         */
  int64_t saturated;       /* the pixels of M the last pass left alone (n + count > 256)   */
  int64_t rays;            /* shot by the whole call: sum of (|M| - saturated) * count     */
} rc_accum_stats;
_Static_assert(sizeof(rc_accum_stats) == 32, "rc_accum_stats layout (ctypes binding)");
/* The last accumulation call enqueued on the current device: waits for it, then reads its device
 * counters (one slot a pass, so the passes never wait for the host).  -1 if there was none.  A
 * call without a pass (rc_accum_scroll_device with nothing exposed) gives four zeros. */
int rc_accum_stats_get(rc_accum_stats *out);
/* The kernel spans (ms, HIP events) of the last pass of the last accumulation call on the current
 * device: ms[0] the edge list (0 for a pass that takes every pixel), ms[1] the samples.  Returns
 * -1 if there was none. */
int rc_accum_phase_ms(double ms[2]);

/* Windows of a virtual image: pan, zoom and tiles (rc_render_window, rc_render_window_device,
 * rc_accum_pass_window_device; fast and cuda mode).  Every other entry renders the whole picture
 * the scene's camera defines (origin (0,0,0), view plane camera_width x camera_height at z = -1,
 * C/raycast.c:80-81,115-117).  A window is a rectangle of a virtual full_w x full_h image: the
 * caller chooses which part of the picture to look at and at which magnification, and only that
 * part is shot.  A 7x zoom of a W x H frame is a W x H window of the 7W x 7H image; a poster too
 * large for the device is rendered tile by tile; tiles go to any number of streams or devices.
 * Fix the scene, the mode (fast or cuda) and the depth.
 * Plain rendering.  Let V_s be that mode's full_w x full_h image with ssaa = s, s in {1, 2, 4, 8}:
 *     the box filter of the s*full_w x s*full_h image B, as in rc_options.ssaa's contract above.
 *     A window call with output size W x H stores  out[y][x] = V_s[y0 + y][x0 + x].
 *     The virtual pixel is (x0 + x, y0 + y) and the pixel size is cam / (float)(s*full_w) (and
 *     full_h): nothing else changes, so a window is a crop of the image the reference produces
 *     at that size, whatever the size (full_w = 33 554 433 is as good as 97).
 * Accumulation.  rc_accum_pass_device's contract above holds word for word with one substitution:
 *     B_g is the g*full_w x g*full_h image, and sample k of window pixel (x, y) is
 *     B_g[g*(y0 + y) + y[k]][g*(x0 + x) + x[k]].  The active set, the contrast (3 x 3, clipped to
 *     the window, read from `out` as it stands), saturation, res, reset and the counters are
 *     unchanged; acc and out are the window's own W x H.
 * Window independence.  After a reset pass and t = 0 passes covering seq[0..k), the record of
 *     virtual pixel (X, Y) does not depend on the window it was rendered through.  So a viewer that
 *     pans by whole pixels keeps the overlap's records, moving them itself, and renders only the
 *     exposed strip, as a window of its own.  With t > 0 the contrast of a window's border pixels
 *     is clipped to the window, so their membership in the active set depends on the window.
 * Identity window.  full = (W, H), origin (0, 0) gives the bytes of rc_render_device (whole image,
 *     the same ssaa) and of rc_accum_pass_device.
 * rc_timing.zero_normalize counts the rays actually shot (the window's).
 * On the device: one kernel over the window's own subsample grid, one lane per subsample, the
 * s x s subsamples of a pixel on adjacent lanes of a wave, reduced in registers; the subsample
 * image is never stored, in cuda mode either (whose plain ssaa stores it).  The accumulation
 * kernels are rc_accum_pass_device's with the origin added to the pixel.
 * rc_options: mode fast or cuda; ssaa a plain factor 0, 1, 2, 4 or 8 (accumulation: 0 or 1, the
 * sequence carries g); max_recursion as everywhere.
 * Refused, each with a message and -1, from the arguments alone (before any device work): parity
 * mode (a window of its image depends on the scan-order carry of every pixel before it); a
 * threshold in opt->ssaa (adaptive refinement of a window is an accumulation pass with t > 0); a
 * factor outside 0, 1, 2, 4, 8; num_gpus > 1; null pointers; full_w, full_h, W or H below 1; x0 or
 * y0 negative; x0 + W > full_w or y0 + H > full_h (tested without overflow); s*full_w or s*full_h
 * (g for accumulation) above 2^31 - 1; more than 65535 rows of 16-subsample tiles in the window's
 * own s*H subsample rows (or 2^31 - 1 tiles in all).  For accumulation every refusal of
 * rc_accum_pass_device applies as it does there, on W and H.
 * rc_frame_submit, rc_render_sharded, the rate-map, pattern and filtered entries, rc_render_accum
 * (it owns a whole-image state) and rc_accum_resolve_device (it has no camera in it) take no
 * window.  raycast() takes one through
 *   RAYCAST_WINDOW = FWxFH+X0+Y0   (four decimal numbers): the W x H image raycast() is asked for
 *                    is the window at (X0, Y0) of the FW x FH image, in fast and cuda mode with
 *                    RAYCAST_SSAA 1, 2, 4 or 8, so bin/raytrace writes the tiles of a poster one
 *                    at a time.  Malformed, parity mode, RAYCAST_SSAA_ADAPTIVE, RAYCAST_PATTERN,
 *                    RAYCAST_FILTER=tent, RAYCAST_GPUS > 1 or a window that fails
 *                    rc_window_check: a warning, ignored (the whole frame is rendered). */
typedef struct rc_window {
  int32_t full_w, full_h;   /* the virtual image                      */
  int32_t x0, y0;           /* the window's top left pixel inside it   */
} rc_window;
_Static_assert(sizeof(rc_window) == 16, "rc_window layout (ctypes binding)");
/* 0 when a W x H window at *w can be rendered at factor s (0 counts as 1), else -1 with a message
 * naming the rule broken. */
int rc_window_check(const rc_window *w, int width, int height, int s);
/* raycast()'s reading of RAYCAST_WINDOW for a width x height frame against the options
 * rc_default_options(.., 1) gave: 1 and the window in *out when the frame goes through
 * rc_render_window; 0 when unset, and 0 after one of the warnings above. */
int rc_window_env(const rc_options *opt, int width, int height, rc_window *out);
/* rc_render_window: host pixmap (W*H*3 bytes), synchronous, on opt->device.
 * rc_render_window_device: device image on the current device and the given HIP stream (NULL: the
 * library's stream of that device, as rc_render_device); asynchronous unless timing is requested.
 * Both return 0 on success. */
int rc_render_window(const rc_scene *scene, const rc_window *win, int width, int height,
                     const rc_options *opt, uint8_t *pixmap, rc_timing *timing);
int rc_render_window_device(const rc_scene *scene, const rc_window *win, int width, int height,
                            const rc_options *opt, uint8_t *d_out, void *stream,
                            rc_timing *timing);
/* rc_accum_pass_device through a window: d_acc (W*H records) and d_out (W*H*3 bytes) are the
 * window's own.  Its stats and phase getters are the accumulation family's (rc_accum_stats_get,
 * rc_accum_phase_ms). */
int rc_accum_pass_window_device(const rc_scene *scene, const rc_window *win, int width, int height,
                                const rc_options *opt, const rc_sample_seq *seq, int first,
                                int count, int threshold, int reset, rc_accum_px *d_acc,
                                uint8_t *d_out, void *stream, rc_timing *timing);

/* Scrolling an accumulated view: a pan that keeps the overlap and shoots only the exposed strips
 * (rc_accum_scroll_device; fast and cuda mode).  `win` is the NEW window and (dx, dy) is the new
 * origin minus the old one, in whole pixels of the virtual image; either sign and any magnitude
 * (all arithmetic on them is done in 64 bits).  Source and destination are two states (records
 * and image) of the same W x H: a viewer keeps two and swaps them.
 * For every destination pixel (x, y) let (sx, sy) = (x + dx, y + dy).
 * Kept:     0 <= sx < W and 0 <= sy < H.  acc_dst[y][x] = acc_src[sy][sx] and
 *           out_dst[y][x] = out_src[sy][sx], verbatim, whatever the record holds: any n, 0 too, a
 *           state left by masked passes too.
 * Exposed:  every other pixel gets exactly what a reset pass followed by t = 0 passes over
 *           seq[0..count) would give window pixel (x, y) of `win`:
 *             sum[c] = sum over k < count of B_g[g*(y0 + y) + y[k]][g*(x0 + x) + x[k]][c],
 *             n = count, out = res(sum, n),
 *           B_g the mode's g*full_w x g*full_h image: the accumulation contract through a window,
 *           word for word.  1 <= count <= seq->nsamples (up to 64); the library shoots it in
 *           chunks of at most 16, the first one resetting, as rc_render_accum does for its dense
 *           part.
 * Every destination pixel is stored to exactly once per array; the source is not written.
 * |dx| >= W or |dy| >= H: nothing is kept, the call is a reset pass of the whole window into the
 * destination.  dx = dy = 0: nothing is exposed, the call is a copy.
 * So when the source was built through the old window by a reset pass and t = 0 passes covering
 * seq[0..count), the destination equals, record for record and byte for byte, the state built
 * from scratch through `win` (window independence, above).  With any other history the kept
 * records are simply moved.  The old window is not an argument and is not checked: only kept
 * pixels come from it, and they lie inside `win` as well.
 * E = W*H - max(0, W - |dx|) * max(0, H - |dy|) pixels are exposed.
 * On the device: the move is one memory-bound kernel over the kept rectangle (one 8-byte record
 * and three bytes a pixel, nothing shot); the exposed set is the complement of that rectangle, at
 * most four rectangles whose sizes the host knows, so the sample kernel needs no list: a fixed
 * number of workgroups strides over [0, E), one lane an exposed pixel, and a strip three pixels
 * wide fills whole waves.  On the current device and the caller's stream (NULL: the library's
 * stream, as rc_accum_pass_device); asynchronous unless timing is requested; nothing waits for
 * the host, so a source written on that stream just before the call is honoured.
 * rc_options: mode fast or cuda; ssaa 0 or 1; max_recursion as everywhere.  rc_timing.kernel_ms
 * covers the move and the samples, zero_normalize counts the exposed pixels' rays only.
 * Stats and spans are the accumulation family's: rc_accum_stats_get gives passes = the number of
 * chunks, active_pixels = E, saturated = 0 and rays = E * count (all four 0 when E = 0);
 * rc_accum_phase_ms gives ms[0] = the move and ms[1] = all the sample chunks.
 * Refused, each with one message and -1, from the arguments alone (before any device work), in
 * this order: a null pointer; an accumulator (either one) that is not 8-byte aligned; every
 * refusal of rc_accum_pass_window_device with t = 0, on W and H (the options, the sequence, the
 * sides, the kernels' grids, then rc_window_check at the sequence's g); W * H >= 2^32; count
 * outside 1..nsamples; the byte ranges of d_acc_src and d_acc_dst overlapping (equal pointers
 * included); those of d_out_src and d_out_dst overlapping.
 * Out of scope: no host-pixmap form and no RAYCAST_* variable (state across calls has no meaning
 * for the one-call drop-in); no threshold (follow with rc_accum_pass_window_device, t > 0, on the
 * new window); no in-place form; no reuse across a zoom. */
int rc_accum_scroll_device(const rc_scene *scene, const rc_window *win, int width, int height,
                           const rc_options *opt, const rc_sample_seq *seq, int count,
                           int dx, int dy,
                           const rc_accum_px *d_acc_src, const uint8_t *d_out_src,
                           rc_accum_px *d_acc_dst, uint8_t *d_out_dst,
                           void *stream, rc_timing *timing);

/* The primary-visibility G-buffer: object id, depth, hit point and normal per pixel
 * (rc_render_gbuffer, rc_render_gbuffer_device, rc_pick, rc_pick_device, rc_id_edge_rates_device;
 * fast, parity and cuda mode).  Every other entry returns colours.  These return what the pixel
 * kernels know about a pixel before they shade it: which shape the primary ray hits, how far away,
 * where and with which normal.  That is picking (what is under the cursor), depth and id planes for
 * compositing and debugging, and a geometric edge criterion for anti-aliasing: the boundary between
 * two equally coloured shapes has no colour contrast, but it has two ids.
 * Values.  For virtual pixel (X, Y) = (x0 + x, y0 + y) of the full_w x full_h image let d be the
 *     reference's primary ray, pixel size cam / (float)full_w and cam / (float)full_h as for a
 *     window at s = 1 (above).  In fast and parity mode (the C port's arithmetic, C/raycast.c)
 *     (id, t, P, N) is what its scan accepts from the origin with no shape skipped, the hit point
 *     O + D*t and the normal of C/raycast.c:461-523: the oracle's rco_prim_nearest(O = 0, D = d,
 *     skip = -1, shadow = 0).  In cuda mode id and t are the CUDA port's (rco_prim_nearest_cuda;
 *     its direction is normalised with a float sum, so t differs in bits on most pixels while the
 *     ids agree).  Every stored float is bit-identical to the oracle's.  id indexes the scene's
 *     shape list in file order.  On a miss id = -1 and everything else is +0.0f.
 * Parity mode is accepted: the primary hit does not involve the scan-order carry, so its planes
 *     are fast mode's, byte for byte.  These are the first window-taking entries that parity mode
 *     does not refuse.
 * P and N in cuda mode (rc_gbuffer.P or .N non-null, frame = 1 in rc_pick*) are refused: the oracle
 *     exports no CUDA-port hit frame, so they could not be pinned.
 * max_recursion is ignored: nothing bounces.
 * rc_render_gbuffer*: win = NULL is the whole W x H image (full = (W, H), origin (0, 0)).  Any
 *     plane pointer may be null (the plane is not wanted and costs nothing), at least one is not.
 *     rc_render_gbuffer takes host planes, is synchronous and runs on opt->device;
 *     rc_render_gbuffer_device takes device planes (the struct itself is host memory), runs on the
 *     current device and the caller's stream (NULL: the library's) and is asynchronous unless
 *     timing is requested.  One kernel, one lane per pixel, k_window's grid at s = 1.
 * rc_pick*: point k is the virtual pixel (xy[2k], xy[2k + 1]) of the full_w x full_h image (any
 *     size up to 2^31 - 1: no grid is laid over it) and hits[k] is its record; duplicates are fine;
 *     n in 1 .. 2^24.  frame = 0 stores +0.0f in P and N.  rc_pick (host arrays) validates the
 *     points before any device work and refuses one outside the image, leaving hits untouched.
 *     rc_pick_device cannot see the points: it shoots no ray for an outside point and stores
 *     id = -2 with everything else +0.0f.  d_hits is 16-byte aligned (a record leaves as two
 *     16-byte stores).
 * rc_id_edge_rates_device: rates[y][x] = s if any pixel of the 3 x 3 neighbourhood of (x, y),
 *     clipped to the image, has an id different from id[y][x], else base; s in {2, 4, 8}, base in
 *     {0, 1}.  One memory-bound kernel on the caller's stream, outside the workspace, like
 *     rc_filter_image_device.  The output is exactly the map rc_render_rates_device takes, so
 *     "anti-alias the object boundaries" is three enqueues on one stream with no host wait:
 *     rc_render_gbuffer_device (id), rc_id_edge_rates_device, rc_render_rates_device; the image is
 *     the rate-map contract's under that map.
 * rc_timing: kernel_ms is the one kernel's span; zero_normalize counts the zero-length
 *     normalisations of the directions and, with P or N (frame = 1), of the normals, as the oracle
 *     counts them (cuda mode counts none, as everywhere); everything parity-specific is 0.
 * rc_gbuffer_phase_ms: ms[0] = the kernel span of the last G-buffer or pick frame enqueued on the
 *     current device (it waits for it); -1 when there is none or another frame has reused its
 *     events.  A G-buffer frame touches no other feature's record: their stats survive it.
 * Refused, each with one message and -1, from the arguments alone (before any device work), in
 * this order: a null scene, options, planes struct or (pick) array; all four planes null; hits not
 * 16-byte aligned (rc_pick_device); a factor outside 0, 1, 2, 4, 8; a threshold in opt->ssaa or a
 * factor above 1 (a G-buffer of the s x s image is a window of the s*full_w x s*full_h image);
 * num_gpus > 1; P, N or frame in cuda mode; whatever rc_window_check(win, W, H, 1) refuses (for
 * pick: a side of the image below 1); for pick, n outside 1 .. 2^24, then (rc_pick) the first point
 * outside the image.  rc_id_edge_rates_device: a null pointer; s not 2, 4 or 8; base not 0 or 1; W
 * or H below 1; W * H >= 2^32.
 * Out of scope: a RAYCAST_* variable or a CLI format for the planes; G-buffers in
 * rc_render_sharded; any criterion beyond the id edge (depth or normal discontinuities are the
 * caller's own map, from the planes it now has). */
typedef struct rc_gbuffer {   /* any pointer may be NULL (plane not wanted); at least one is not */
  int32_t *id;                /* W*H   : index into the scene's shape list, -1 = no primary hit    */
  float   *t;                 /* W*H   : the accepted hit's distance, +0.0f on a miss              */
  float   *P;                 /* W*H*3 : hit point,  +0.0f x 3 on a miss                           */
  float   *N;                 /* W*H*3 : hit normal, +0.0f x 3 on a miss                           */
} rc_gbuffer;                 /* row-major, top row first                                          */
typedef struct rc_hit { int32_t id; float t; float P[3]; float N[3]; } rc_hit;
_Static_assert(sizeof(rc_gbuffer) == 32, "rc_gbuffer layout (ctypes binding)");
_Static_assert(sizeof(rc_hit) == 32, "rc_hit layout (ctypes binding, the kernel's two stores)");
int rc_render_gbuffer(const rc_scene *scene, const rc_window *win /* NULL: the whole image */,
                      int width, int height, const rc_options *opt,
                      const rc_gbuffer *planes /* host */, rc_timing *timing);
int rc_render_gbuffer_device(const rc_scene *scene, const rc_window *win, int width, int height,
                             const rc_options *opt, const rc_gbuffer *d_planes, void *stream,
                             rc_timing *timing);
int rc_pick(const rc_scene *scene, int full_w, int full_h, const rc_options *opt, int frame,
            int64_t n, const int32_t *xy /* n pairs */, rc_hit *hits);
int rc_pick_device(const rc_scene *scene, int full_w, int full_h, const rc_options *opt, int frame,
                   int64_t n, const int32_t *d_xy, rc_hit *d_hits, void *stream);
int rc_id_edge_rates_device(const int32_t *d_id, int width, int height, int s, int base,
                            uint8_t *d_rates, void *stream);
int rc_gbuffer_phase_ms(double ms[1]);

/* Rotated camera views and caller-supplied ray batches (rc_render_view, rc_render_view_device,
 * rc_trace_rays, rc_trace_rays_device; fast and cuda mode).  Every other entry shoots the
 * reference camera's rays: eye at the origin, looking down -z, one ray per pixel of a regular
 * grid.  A view turns that camera about the eye; a ray batch shoots whatever directions the caller
 * supplies (a fisheye or equirectangular probe, a cube-map face, a stereo pair, the ray under the
 * cursor of a turned view).
 * The view contract.  rc_view.m is a 3 x 3 matrix M, row-major.  For virtual pixel (X, Y) of the
 *     full_w x full_h image (with ssaa = s: subsample (X, Y) of the s*full_w x s*full_h image, as
 *     for a window) let p = (px, py, -1) be the reference's unnormalised primary vector,
 *         px = (float)(hx + (double)pw * ((double)X + 0.5)),
 *         py = (float)(hy - (double)ph * ((double)Y + 0.5)),
 *     hx = 0.0 - cam_w / 2.0, hy = 0.0 + cam_h / 2.0 in double, pw = cam_w / (float)full_w and
 *     ph = cam_h / (float)full_h in float (C/raycast.c:109-118).  Then
 *         q_i = (m[3i] * p.x + m[3i + 1] * p.y) + m[3i + 2] * p.z      (i = 0, 1, 2)
 *     in float, every operation rounded once and nothing contracted, and the ray's direction D is
 *     the mode's own normalize of q: the C port's (double sum of squares, a zero length leaves q
 *     as it is and counts a zero_normalize event) in fast mode, the CUDA port's (float sum, no
 *     guard) in cuda mode.  The matrix is applied before the single normalisation, so M need not
 *     be orthonormal: an anamorphic or a mirrored view is legal, and M = identity gives the plain
 *     camera's direction bit for bit.  The pixel's colour is the mode's bounce loop for D from the
 *     origin, the oracle's rco_prim_shoot(D) / rco_prim_shoot_cuda(D); ssaa, the window and the
 *     byte rounding are the window contract's: out = crop(box_s(view image at s*full)).
 * The eye stays at the origin here; rc_render_camera (below) moves it.
 * rc_view_check: 0 when every entry of m is finite; otherwise (or for a null view) a message and
 *     -1.  Nothing else is refused: a singular M gives zero or repeated directions, not an error.
 * rc_render_view*: win = NULL is the whole W x H image, otherwise the W x H window of rc_window
 *     (rc_window_check at the options' factor).  opt->ssaa is 0, 1, 2, 4 or 8.  rc_render_view
 *     takes a host pixmap, is synchronous and runs on opt->device; rc_render_view_device takes
 *     device memory (W*H*3 bytes), runs on the current device and the caller's stream (NULL: the
 *     library's) and is asynchronous unless timing is requested.  One kernel, k_window's grid.
 * rc_trace_rays*: ray k leaves the origin along (dirs[3k], dirs[3k + 1], dirs[3k + 2]), USED AS
 *     GIVEN: it is not normalised, because the oracle's export does not normalise either; n in
 *     1 .. 2^24.  rc_ray_out: any pointer may be null, at least one is not.  rgb (n x 3 floats) is
 *     the colour before quantisation, rco_prim_shoot's bit for bit (what tone mapping and
 *     compositing need); rgb8 (n x 3 bytes) is its quantisation, the bytes a frame stores; hits (n
 *     records) is the G-buffer's rc_hit for that direction, rco_prim_nearest(O = 0, D, skip = -1):
 *     id and t, and with frame = 1 P and N (+0.0f without; refused in cuda mode, as for rc_pick).
 *     Picking in a turned view is rc_trace_rays of the cursor pixel's view direction.
 *     rc_trace_rays takes host arrays; rc_trace_rays_device device arrays (the struct itself is
 *     host memory, d_hits 16-byte aligned) and is asynchronous.
 * rc_timing / zero_normalize: the events of the directions' normalisations and of the rays, as
 *     the oracle counts them (cuda mode counts none).
 * rc_view_phase_ms: ms[0] = the kernel span of the last view or ray frame enqueued on the current
 *     device (it waits for it); -1 when there is none or another frame has reused its events.  A
 *     view or ray frame touches no other feature's record: their stats survive it.
 * Refused, each with one message and -1, from the arguments alone, in this order.  rc_render_view*:
 *     a null scene, view, options or image; a factor outside 0, 1, 2, 4, 8; an adaptive threshold;
 *     parity mode (its image is defined by the scan-order carry of the reference's own camera);
 *     num_gpus > 1; what rc_view_check refuses; what rc_window_check refuses.  rc_trace_rays*: a
 *     null scene, options, dirs or out; all three outputs null; d_hits not 16-byte aligned; a bad
 *     factor; a threshold or a factor above 1 (a ray is one sample); parity mode; num_gpus > 1;
 *     frame in cuda mode; n outside 1 .. 2^24.
 * Out of scope: accumulation and scrolling through a view (a rotation is not a pan); a RAYCAST_*
 *     variable or a CLI option for the view; parity mode; multi-GPU. */
typedef struct rc_view { float m[9]; } rc_view;   /* row-major: q = M p */
_Static_assert(sizeof(rc_view) == 36, "rc_view layout (ctypes binding)");
typedef struct rc_ray_out {   /* any pointer may be NULL (not wanted); at least one is not */
  uint8_t *rgb8;              /* n*3 : the quantised colour                                 */
  float   *rgb;               /* n*3 : the colour before quantisation                       */
  rc_hit  *hits;              /* n   : the primary hit's record                             */
  int32_t  frame;             /* 1: P and N in the records too (fast mode only)             */
} rc_ray_out;
_Static_assert(sizeof(rc_ray_out) == 32, "rc_ray_out layout (ctypes binding)");
int rc_view_check(const rc_view *view);
int rc_render_view(const rc_scene *scene, const rc_view *view,
                   const rc_window *win /* NULL: the whole image */, int width, int height,
                   const rc_options *opt, uint8_t *pixmap, rc_timing *timing);
int rc_render_view_device(const rc_scene *scene, const rc_view *view, const rc_window *win,
                          int width, int height, const rc_options *opt, uint8_t *d_out,
                          void *stream, rc_timing *timing);
int rc_trace_rays(const rc_scene *scene, const rc_options *opt, int64_t n,
                  const float *dirs /* n x 3 */, const rc_ray_out *out /* host */);
int rc_trace_rays_device(const rc_scene *scene, const rc_options *opt, int64_t n,
                         const float *d_dirs, const rc_ray_out *d_out, void *stream);
int rc_view_phase_ms(double ms[1]);

/* A free camera and rays with origins (rc_render_camera, rc_render_camera_device,
 * rc_trace_rays_from, rc_trace_rays_from_device; fast mode).  The view family with an origin: a
 * fly-through camera, a stereo pair with a real baseline, a thin-lens bundle, and secondary rays
 * of the caller's own that leave the hit points rc_render_gbuffer and rc_trace_rays hand out.
 * The camera contract.  rc_camera is an eye and a view.  The direction of every ray is the view
 *     contract's D for cam->view (above), unchanged: moving the eye does not touch the direction
 *     arithmetic.  The origin of every ray is cam->eye, used as given (a -0 component stays -0).
 *     The ray's colour is the fast-mode bounce loop from (eye, D): with the oracle's exports,
 *         (i, t) = rco_prim_nearest(eye, D, skip = -1); a miss is black;
 *         (P, N) = the hit frame of i at eye + t D; obj = S = i; T = refl[i]; out = 0;
 *         for level 1 .. max_recursion - 1: stop unless refl[obj] > 0;
 *             D = normalize(reflect(D, N))      (float; the length is (float)sqrt of the double
 *                                                sum of squares, a zero length leaves D);
 *             (i, t) = rco_prim_nearest(P, D, skip = S); stop at a miss; (P, N) = its frame;
 *             out += rco_prim_shade(i, P, N, D) * T; T *= refl[i]; obj = S = i;
 *         colour = out + rco_prim_shade of the primary hit.
 *     At eye = +0 this is rco_prim_shoot(D) bit for bit (tests/test_camera.py), so eye = 0 with
 *     the matrix M is rc_render_view(M), and with the identity the plain fast-mode image.  ssaa,
 *     the window and the byte rounding are the window contract's.
 * rc_camera_check: 0 when every component of eye and every entry of view.m is finite; otherwise
 *     (or for a null camera) one message and -1.
 * rc_render_camera*: the arguments, the stream semantics, rc_timing and the spans are
 *     rc_render_view*'s.  One kernel, k_window's grid.  Nothing is kept between calls and nothing
 *     is shared between two calls in flight: the eye is a kernel argument, and no scratch buffer
 *     in device memory holds anything derived from it.
 * rc_trace_rays_from*: rc_trace_rays* with ray k leaving (origins[3k], origins[3k + 1],
 *     origins[3k + 2]).  rc_ray_out as there; hits is rco_prim_nearest(O, D, skip = -1), with
 *     frame = 1 P and N too.  Origins are data (device data for the _device entry) and are not
 *     checked: a non-finite origin gives what the oracle gives, a miss.
 * rc_view_phase_ms also reads the span of the last camera or origin-ray frame: the four entries
 *     record the view family's event set.
 * Refused, each with one message and -1, before any device work.  rc_render_camera*: a null
 *     scene, camera, options or image; what rc_render_view refuses, in its order, with cuda mode
 *     refused after num_gpus (the oracle exports no hit frame for the CUDA port, so nothing could
 *     pin a colour there); what rc_camera_check refuses; what rc_window_check refuses.
 *     rc_trace_rays_from*: a null scene, options, origins, dirs or out; then what rc_trace_rays
 *     refuses, with cuda mode refused after num_gpus.
 * Out of scope: cuda and parity mode; scrolling with a camera (accumulation with one is
 *     rc_accum_pass_camera_device, below); a G-buffer plane
 *     entry for cameras (rc_trace_rays_from with hits alone is the pick); multi-GPU.  Any-hit
 *     queries with a distance bound are rc_occluded_rays, below. */
typedef struct rc_camera { float eye[3]; rc_view view; } rc_camera;
_Static_assert(sizeof(rc_camera) == 48, "rc_camera layout (ctypes binding)");
int rc_camera_check(const rc_camera *cam);
int rc_render_camera(const rc_scene *scene, const rc_camera *cam,
                     const rc_window *win /* NULL: the whole image */, int width, int height,
                     const rc_options *opt, uint8_t *pixmap, rc_timing *timing);
int rc_render_camera_device(const rc_scene *scene, const rc_camera *cam, const rc_window *win,
                            int width, int height, const rc_options *opt, uint8_t *d_out,
                            void *stream, rc_timing *timing);
int rc_trace_rays_from(const rc_scene *scene, const rc_options *opt, int64_t n,
                       const float *origins /* n x 3 */, const float *dirs /* n x 3 */,
                       const rc_ray_out *out /* host */);
int rc_trace_rays_from_device(const rc_scene *scene, const rc_options *opt, int64_t n,
                              const float *d_origins, const float *d_dirs,
                              const rc_ray_out *d_out, void *stream);

/* Accumulation through a free camera: progressive anti-aliasing of a camera frame, depth of field
 * and camera motion blur (rc_accum_pass_camera_device, rc_render_camera_accum; fast mode).  The
 * accumulation family above shoots the reference camera's rays from the origin; these two entries
 * take the samples through rc_camera values instead.  A pass takes one camera for all its samples
 * (a still camera refines) or one camera for each sample (16 lens points or 16 instants cost one
 * launch and one read-modify-write of the record).  The state is the caller's rc_accum_px array as
 * before: nothing in a record says which camera a sample came through, so cameras may change
 * between passes and the passes of the other accumulation entries may be mixed in.
 * Contract.  rc_accum_pass_window_device's contract holds word for word, with one substitution:
 *     the active set, the contrast, saturation, res, reset, first and count (1 <= count <= 16),
 *     the stats and the spans are unchanged.  Let C_g(c) be the image rc_render_camera defines for
 *     camera c at g*full_w x g*full_h with ssaa = 1 (the view contract's directions, every ray
 *     leaving c.eye, the fast-mode bounce loop of the camera contract, the byte rounding).  Sample
 *     first + j of window pixel (x, y), 0 <= j < count, is
 *         C_g(cams[ncams == 1 ? 0 : j])[g*(y0 + y) + y[first + j]][g*(x0 + x) + x[first + j]].
 *     ncams is 1 or count; camera j belongs to the j-th sample of the pass, whatever `first` is.
 *     The cameras are host memory and are copied at the call.  win = NULL is the whole W x H image.
 *     A camera with eye = +0 and the identity view gives rc_accum_pass_window_device's records and
 *     bytes exactly, and with win = NULL rc_accum_pass_device's.  Window independence holds per
 *     camera, as in the window contract.
 * rc_render_camera_accum: the host-pixmap form, synchronous on opt->device, the accumulator owned
 *     by the library.  The whole sequence goes to every pixel: a reset pass, in chunks of at most
 *     16.  ncams is 1 or seq->nsamples, and sample k goes through cams[ncams == 1 ? 0 : k].  With
 *     hier<g> and one camera the image is rc_render_camera's at ssaa = g.
 * The stats, the spans and rc_timing are the accumulation family's (rc_accum_stats_get,
 *     rc_accum_phase_ms), as rc_accum_pass_window_device documents them.
 * On the device: the accumulation kernels' layout (one lane a pixel, the samples one after the
 *     other, one 8-byte load and one 8-byte store of the record) with each sample shot as
 *     rc_render_camera shoots a subsample.  The cameras are a kernel argument read with the uniform
 *     sample index: nothing derived from a camera lives in device memory, and two passes in flight
 *     share nothing.  t > 0 is the edge list and the list kernel on one stream with no host wait.
 * Refused, each with one message and -1, from the arguments alone (before any device work), in
 *     this order:
 *       1. a null scene, cams, options, sequence, accumulator or image (win may be null);
 *       2. (pass) an accumulator that is not 8-byte aligned;
 *       3. what rc_accum_pass_window_device refuses, in its order, on W and H: a factor above 1 or
 *          a threshold in opt->ssaa; parity mode; num_gpus > 1; then cuda mode (as in the camera
 *          family: the oracle exports no hit frame for the CUDA port); a sequence that fails
 *          rc_sample_seq_check; a threshold outside 0..255; W or H below 1 or above 2^28 / g; with
 *          t > 0, W * H >= 2^32; more than 65535 rows of tiles; what rc_window_check refuses at g;
 *          (pass) first or count out of range; reset with t > 0;
 *       4. ncams outside {1, count} (the host form: {1, nsamples});
 *       5. the first camera that rc_camera_check would refuse, named by its index.
 * Out of scope: scrolling with a camera (rc_accum_scroll_device moves records of the reference
 *     camera's pan; a camera's turn is not a pan); cuda and parity mode; a threshold in the host
 *     form (follow with rc_accum_pass_camera_device, t > 0); a RAYCAST_* variable; multi-GPU. */
int rc_accum_pass_camera_device(const rc_scene *scene, const rc_camera *cams, int ncams,
                                const rc_window *win /* NULL: the whole image */,
                                int width, int height, const rc_options *opt,
                                const rc_sample_seq *seq, int first, int count, int threshold,
                                int reset, rc_accum_px *d_acc, uint8_t *d_out,
                                void *stream, rc_timing *timing);
int rc_render_camera_accum(const rc_scene *scene, const rc_camera *cams, int ncams,
                           const rc_window *win, int width, int height, const rc_options *opt,
                           const rc_sample_seq *seq, uint8_t *pixmap, rc_timing *timing);

/* Any-hit visibility queries and ambient occlusion (rc_occluded_rays, rc_occluded_rays_device,
 * rc_ao_pass_device, rc_ao_resolve_device, rc_render_ao; fast mode).  The question a shadow ray
 * asks, for the caller's own rays: is anything in the way, within this distance?  And the pass
 * that asks it for a set of directions around every primary hit of a camera frame and counts the
 * answers, in one kernel: an ambient-occlusion plane, accumulated across calls.
 * The occlusion rule for one ray (O, D, skip, tmax).  With (hit_k, t_k) = rco_prim_shape(shape k,
 *     O, D, skip) of the oracle,
 *         blocked = any over k != skip of (hit_k and t_k > 0 and t_k < tmax).
 *     D is used as given, not normalised: t and tmax are in units of |D|.  skip = -1 skips nothing
 *     and switches the quadrics' z rule off; any other value switches it on (a bounce ray's
 *     quadric hit below the origin's z is ignored), which is exactly the reference's use of skip.
 *     With tmax = +inf the rule is the reference's shadow test: blocked equals
 *     rco_prim_nearest(O, D, skip, shadow = 1).idx >= 0.  A tmax that is NaN, <= 0 or -inf blocks
 *     nothing (t < tmax fails).  On the device tmax = +inf takes the shade path's own shadow scan
 *     and a finite tmax the nearest scan's tests with the bound in the place of the best t; both
 *     stop at the first accepted shape.
 * rc_occluded_rays*: n rays (1 .. 2^24); origins and dirs as in rc_trace_rays_from; skip: int32[n]
 *     or NULL for -1 everywhere; tmax: float[n] or NULL for +inf everywhere; out: one byte a ray,
 *     1 blocked, 0 open.  Per-ray data is data (device data for the _device entry) and is not
 *     inspected: a non-finite origin or direction blocks nothing, as in the oracle; a skip outside
 *     [-1, n_shapes) skips nothing but switches the z rule on.  One lane a ray.  The two entries
 *     take the same arguments: the _device entry is enqueued on the stream and timing (may be
 *     NULL) is rc_render_view_device's; the host form is synchronous on opt->device, ignores
 *     `stream` and fills timing as rc_render_view does.
 * Ambient occlusion through a camera.  The state is the caller's array of rc_ao_px, one a pixel,
 *     row-major, 4-byte aligned device memory: `rays` occlusion rays have been counted for the
 *     pixel, `open` of them were not blocked.  A direction set (rc_ao_dirs) travels by value: n
 *     directions u[0..n), used as given, and one tmax in units of |u|.
 *     rc_ao_dirs_check: 0, or one message and -1 for a null set, n outside 1..64, a tmax that is
 *     not in (0, +inf] (NaN included), and the first direction that has a non-finite component or
 *     is (+-0, +-0, +-0), named by its index.
 *     rc_ao_pass_device does this for window pixel (x, y) (win = NULL: the whole image):
 *       1. the primary ray is rc_render_camera's for cam at ssaa = 1: the view contract's
 *          direction d, the origin cam->eye, (id, t, P, N) = rco_prim_nearest(eye, d, skip = -1).
 *          The general scan is used at every eye, +0 included (bit-equal to the origin forms);
 *       2. a miss: open_add = n;
 *       3. a hit: direction j is D_j = dot(N, u_j) < 0 ? u_j * -1.0f : u_j (the oracle's float dot,
 *          (N0 u0 + N1 u1) + N2 u2; a NaN dot does not flip), the ray is (P, D_j, skip = id,
 *          dirs.tmax), and open_add = the number of j whose ray is not blocked.  skip = id carries
 *          the reference's z rule for rays that leave a surface, as its own shadow rays do: a
 *          quadric hit below P's z does not block;
 *       4. (open, rays) = reset ? (0, 0) : d_ao[pixel].  If rays + n > 65535 the record stays as
 *          it is: the pixel is saturated and none of its rays are shot, the primary ray included.
 *          Otherwise open += open_add, rays += n;
 *       5. d_out (W*H bytes, may be NULL) gets rc_ao_byte(open, rays) of the record as it now is.
 *     rc_ao_byte(open, rays) = rays ? (510 * open + rays) / (2 * rays) : 255 in integer
 *     arithmetic: 255 * open / rays rounded half up.
 *     rc_ao_resolve_device: step 5 alone, for every record; no scene, no workspace.
 *     rc_render_ao: the host form, synchronous on opt->device, the state owned by the library: a
 *     reset pass with sets[0], one further pass for each of sets[1..nsets), then the W*H bytes.
 *     rc_ao_stats_get: the last pass of the current device: hit_pixels (unsaturated pixels whose
 *     primary ray hit), rays (occlusion rays shot: n * hit_pixels), blocked (those that were
 *     blocked) and saturated (pixels left as they were).  rc_ao_phase_ms: the span of the last
 *     call's kernels (every pass of rc_render_ao; a ray batch too).
 * On the device: one kernel a pass, rc_render_camera's grid, one lane a pixel.  The direction loop
 *     is uniform, so u_j and tmax are read from the kernel's arguments with scalar loads and only
 *     the hit point, the skip index and the flip are per lane: neighbouring lanes test the same
 *     direction from neighbouring points, so the early exit diverges little.  The record is one
 *     4-byte load and one 4-byte store a lane.  Nothing is kept on the device between passes but
 *     the caller's state, and two passes in flight on two states share nothing.
 * Refused, each with one message and -1, from the arguments alone (before any device work), in
 *     this order:
 *       1. a null scene, camera, options, direction set or state (win and d_out may be null;
 *          rc_render_ao: the pixmap may not; rc_occluded_rays*: a null scene, options, origins,
 *          dirs or out);
 *       2. a d_ao that is not 4-byte aligned;
 *       3. the camera family's clauses in their order: parity mode, num_gpus > 1, cuda mode, then
 *          what rc_window_check refuses for W, H and the window at factor 1 (rc_occluded_rays*: the
 *          three mode clauses);
 *       4. an opt->ssaa other than 0 or 1;
 *       5. what rc_camera_check refuses (rc_occluded_rays*: n outside 1 .. 2^24);
 *       6. what rc_ao_dirs_check refuses (rc_render_ao: nsets outside 1..1024, then the first set
 *          that fails, named by its index).
 *     rc_ao_resolve_device: a null pointer, a misaligned d_ao, W or H below 1 or an image past
 *     one grid.
 * Out of scope: cosine or per-direction weights; supersampled primary rays; cuda and parity mode;
 *     multi-GPU.  Filtering the plane and adding it to a colour image are rc_ao_filter_device and
 *     rc_ao_compose_device, below. */
#define RC_AO_MAX_DIRS 64
typedef struct rc_ao_px { uint16_t open, rays; } rc_ao_px;
typedef struct rc_ao_dirs { int32_t n; float tmax; float u[RC_AO_MAX_DIRS][3]; } rc_ao_dirs;
typedef struct rc_ao_stats { int64_t hit_pixels, rays, blocked, saturated; } rc_ao_stats;
_Static_assert(sizeof(rc_ao_px) == 4, "rc_ao_px layout (the kernels' 4-byte record)");
_Static_assert(sizeof(rc_ao_dirs) == 776, "rc_ao_dirs layout (a kernel argument, ctypes binding)");
int rc_ao_dirs_check(const rc_ao_dirs *dirs);
int rc_occluded_rays(const rc_scene *scene, const rc_options *opt, int64_t n,
                     const float *origins /* n x 3 */, const float *dirs /* n x 3 */,
                     const int32_t *skip /* n, or NULL */, const float *tmax /* n, or NULL */,
                     uint8_t *out /* n */, void *stream /* ignored */, rc_timing *timing);
int rc_occluded_rays_device(const rc_scene *scene, const rc_options *opt, int64_t n,
                            const float *d_origins, const float *d_dirs, const int32_t *d_skip,
                            const float *d_tmax, uint8_t *d_out, void *stream, rc_timing *timing);
int rc_ao_pass_device(const rc_scene *scene, const rc_camera *cam,
                      const rc_window *win /* NULL: the whole image */, int width, int height,
                      const rc_options *opt, const rc_ao_dirs *dirs, int reset, rc_ao_px *d_ao,
                      uint8_t *d_out /* W*H bytes, or NULL */, void *stream, rc_timing *timing);
int rc_ao_resolve_device(const rc_ao_px *d_ao, int width, int height, uint8_t *d_out,
                         void *stream);
int rc_render_ao(const rc_scene *scene, const rc_camera *cam, const rc_window *win, int width,
                 int height, const rc_options *opt, const rc_ao_dirs *sets, int nsets,
                 uint8_t *pixmap /* W*H bytes */, rc_timing *timing);
int rc_ao_stats_get(rc_ao_stats *out);
int rc_ao_phase_ms(double ms[1]);

/* The G-buffer through a camera, the guided filter of the occlusion records and the ambient
 * compose (rc_render_camera_gbuffer, rc_render_camera_gbuffer_device, rc_ao_filter_device,
 * rc_ao_compose_device, rc_render_ambient; fast mode).  What turns the occlusion plane above into
 * part of a picture: the guide for a moved eye, an edge-aware blur of the records that pools
 * neighbouring pixels of the same surface, and an ambient term modulated by the result.
 * rc_render_camera_gbuffer*: step 1 of rc_ao_pass_device, stored.  For window pixel (x, y) the
 *     direction d is rc_render_camera's at ssaa = 1 (the view contract's), and
 *     (id, t, P, N) = rco_prim_nearest(cam->eye, d, skip = -1, shadow = 0) and its frame; the
 *     general scan is used at every eye, +0 included.  The planes are rc_gbuffer's, any may be
 *     null; a miss is id = -1 and +0.0f everywhere else; every stored float is bit-identical to
 *     the oracle's.  zero_normalize counts as in rc_render_gbuffer (the normal's events only when
 *     P or N is asked for).  The two entries take the same arguments as rc_render_gbuffer*'s with
 *     the camera in front of the window.
 *     Refused, in this order: 1. a null scene, camera, options or planes struct; 2. all four
 *     planes null; 3. the camera family's mode clauses (parity mode, num_gpus > 1, cuda mode), then
 *     what rc_window_check refuses at factor 1; 4. an opt->ssaa other than 0 or 1; 5. what
 *     rc_camera_check refuses.
 * rc_ao_filter: the pooling window and its thresholds, by value (32 bytes).  radius 0..8 (0 pools
 *     nothing), taps[|d|] for d = 0..radius, pad = 0.  rc_ao_filter_box (taps 1) and
 *     rc_ao_filter_tent (taps[d] = radius + 1 - d) fill one with nmin = 0.9f, dplane = 0.05f.
 *     rc_ao_filter_check: 0, or one message and -1 for, in this order: 1. a null struct; 2. a
 *     radius outside 0..8; 3. pad != 0; 4. taps[0] == 0; 5. (taps[0] + 2 * sum taps[1..radius])^2
 *     > 32768; 6. an nmin that is NaN; 7. a dplane that is NaN or negative.  With clause 5 the
 *     sums below stay under 2^31 (32768 * 65535 < 2^31).  nmin = -inf with dplane = +inf pools
 *     every neighbour of the same id; nmin = 2 pools nothing.
 * rc_ao_filter_device: the rule, for p = (x, y) and every q = (x + dx, y + dy) with |dx|, |dy| <=
 *     radius inside the W x H plane; every float operation is one float32 operation in this
 *     order, nothing contracted:
 *         e         = P_q - P_p                                   (componentwise)
 *         pd        = (N_p[0]*e[0] + N_p[1]*e[1]) + N_p[2]*e[2]   (the oracle's dot)
 *         nd        = (N_p[0]*N_q[0] + N_p[1]*N_q[1]) + N_p[2]*N_q[2]
 *         accept(q) = q == p or (id_q == id_p and nd >= nmin and fabsf(pd) <= dplane)
 *         w(q)      = taps[|dx|] * taps[|dy|]
 *         O = sum over accepted q of w(q) * open_q     R = sum over accepted q of w(q) * rays_q
 *         out[p]    = id_p < 0 ? rc_ao_byte(open_p, rays_p) : (R ? (510*O + R) / (2*R) : 255)
 *     A comparison with a NaN is false, so such a q is rejected; the centre is always accepted, so
 *     a pixel that stands alone keeps its own byte; a miss (id_p < 0) keeps its own byte and is
 *     pooled into nothing.  Guide and records are data (device memory: d_ao W*H records, 4-byte
 *     aligned; the guide's id, P and N planes, t is not read) and are not inspected; records with
 *     open > rays are outside the contract (no fault, the byte is unspecified).  The plane has no
 *     window: a window's filtered plane is not the crop of the whole image's, because the pixels
 *     next to the window's edge pool neighbours outside it; a tiling caller supplies its own halo
 *     (filter a window grown by `radius` and keep the middle).  No scene and no workspace, like
 *     rc_ao_resolve_device; d_out: W*H bytes of any alignment.
 *     Refused, in this order: 1. a null d_ao, guide, filter or d_out; 2. a guide without id, P or
 *     N; 3. a d_ao that is not 4-byte aligned; 4. W or H below 1; 5. an image past one grid (a
 *     side above 16 * 65535); 6. what rc_ao_filter_check refuses.
 * rc_ao_compose_device: with a[k][c] = quant(ambient[c] * diffuse_color_k[c]) for shape k and
 *     channel c (one float32 product, then rco_prim_quant), a pixel with 0 <= id < n_shapes gets
 *         out[c] = min(255, in[c] + (a[id][c] * ao + 127) / 255)     in integers,
 *     and any other id leaves out = in.  d_id: W*H int32; d_ao: W*H bytes (a filtered or a plain
 *     plane); d_rgb_in, d_rgb_out: W*H*3 bytes of any alignment, equal or disjoint.
 *     Refused, in this order: 1. a null pointer; 2. parity mode, num_gpus > 1, cuda mode; 3. an
 *     ambient component that is not finite or is negative; 4. W or H below 1; 5. an image past
 *     one grid.
 * rc_render_ambient: the host form, synchronous on opt->device, everything on the library's
 *     stream with state and planes owned by the library: rc_render_camera at ssaa = 1,
 *     rc_render_ao's passes (a reset pass, then one pass a further set), the camera's G-buffer,
 *     the filter, the compose, one copy out.  Its image is by definition the composition of the
 *     device entries above.  timing covers all its kernels, zero_normalize their sum;
 *     rc_ao_stats_get reads its last pass.  Refused, in this order: a null pointer (win may be
 *     null); what rc_render_ao refuses; an image past one grid; what rc_ao_filter_check refuses;
 *     the compose's ambient clause.
 * Out of scope: iterated (a-trous) passes and a record output of the filter; cosine or
 *     per-direction weights; filtering colours; cuda and parity mode; multi-GPU; a RAYCAST_*
 *     variable or CLI format for any of it. */
#define RC_AO_FILTER_MAX_RADIUS 8
typedef struct rc_ao_filter {
  int32_t  radius;                              /* 0 .. 8; 0 pools nothing                    */
  float    nmin;                                /* accept q when dot(N_p, N_q) >= nmin        */
  float    dplane;                              /* ... and |dot(N_p, P_q - P_p)| <= dplane    */
  uint16_t taps[RC_AO_FILTER_MAX_RADIUS + 1];   /* taps[|d|], d = 0 .. radius                 */
  uint16_t pad;                                 /* 0                                          */
} rc_ao_filter;                                 /* 32 bytes, by value, a kernel argument      */
_Static_assert(sizeof(rc_ao_filter) == 32, "rc_ao_filter layout (a kernel argument, ctypes binding)");
int rc_render_camera_gbuffer(const rc_scene *scene, const rc_camera *cam, const rc_window *win,
                             int width, int height, const rc_options *opt,
                             const rc_gbuffer *planes, rc_timing *timing);
int rc_render_camera_gbuffer_device(const rc_scene *scene, const rc_camera *cam,
                                    const rc_window *win, int width, int height,
                                    const rc_options *opt, const rc_gbuffer *d_planes,
                                    void *stream, rc_timing *timing);
int rc_ao_filter_box(int radius, rc_ao_filter *out);    /* taps 1                    */
int rc_ao_filter_tent(int radius, rc_ao_filter *out);   /* taps[d] = radius + 1 - d  */
int rc_ao_filter_check(const rc_ao_filter *f);
int rc_ao_filter_device(const rc_ao_px *d_ao, const rc_gbuffer *d_guide /* id, P, N non-null */,
                        int width, int height, const rc_ao_filter *f, uint8_t *d_out /* W*H */,
                        void *stream);
int rc_ao_compose_device(const rc_scene *scene, const rc_options *opt, const int32_t *d_id,
                         const uint8_t *d_ao /* W*H */, const float ambient[3],
                         const uint8_t *d_rgb_in, uint8_t *d_rgb_out /* may equal d_rgb_in */,
                         int width, int height, void *stream);
int rc_render_ambient(const rc_scene *scene, const rc_camera *cam, const rc_window *win, int width,
                      int height, const rc_options *opt, const rc_ao_dirs *sets, int nsets,
                      const rc_ao_filter *filter, const float ambient[3],
                      uint8_t *pixmap /* W*H*3 */, rc_timing *timing);

/* Frames in flight(an extension for rendering frame sequences; no reference
 * counterpart).  rc_frame_submit enqueues one whole W x H image of `scene` into d_out
 * (W*H*3 bytes, device memory, ready for use: synchronise the stream that produced it
 * first) and returns.  It is byte-identical to rc_render_device's.  In parity mode up to
 * two frames are in flight on the current device.  The device's CUs are split in two
 * partitions (hipExtStreamCreateWithCUMask; RC_PIPE_RES_CUS sets the resolver's share).
 * One runs the frames' carry resolvers in submission order.  The other runs the next frame's
 * phase A and compaction and the previous frame's phase C beside it.  A frame then costs
 * about its resolver's time instead of the sum of its phases.  Fast mode (no serial stage)
 * renders the frames back to back on the whole device.
 * Completion: rc_frames_wait is the only completion point for submitted parity frames.  The
 * last submitted frame's phase C is held back until the next rc_frame_submit (on its lane's
 * stream) or rc_frames_wait (on every CU), so synchronising a stream or the device after
 * rc_frame_submit does NOT complete that frame: its DEP pixels may still hold phase A's
 * bytes.  rc_lone_frames_check, rc_render_device and rc_render launch a pending phase C
 * first, so a later device synchronisation completes it; rc_pipe_reset waits for it.
 * rc_frames_wait blocks until every
 * submitted frame is complete.  It reports a failed resolver hand-off (returns -1) and fills
 * *timing (may be NULL): resolve_ms = mean resolver span; dep_pixels and zero_normalize of
 * the last frame. */
int rc_frame_submit(const rc_scene *scene, int width, int height, const rc_options *opt,
                    uint8_t *d_out);
int rc_frames_wait(rc_timing *timing);
/* Every parity frame is verified: after its last kernel the words its bounded carry
 * hand-offs set on a failure (timed-out spin: code, workgroup, details) are copied on the
 * frame's own stream into a pinned per-frame ring, before the frame's workspace can be reused.
 * rc_frames_wait reads back every frame since the previous wait (frames_checked /
 * frames_failed in *timing) and returns -1 if any failed; rc_frame_submit refuses new frames
 * once a frame in flight is known to have failed.  One-frame-at-a-time renders
 * (rc_render_device, rc_render) are read back at the next call on the device (which then
 * returns -1) or by rc_lone_frames_check, which synchronises the current device and returns
 * the count since its previous call (-1 if any failed). */
int rc_lone_frames_check(int64_t *checked, int64_t *failed);
/* Test aid: the nth_frame-th parity frame from now (0 = the next, any entry point, any
 * device) fails its hand-off as a timed-out spin would (error code 4); -1 cancels. */
int rc_debug_inject_error(int nth_frame);
/* Test aid (no GPU needed): rc_render's in-frame scatter of the mapped colour patch against a
 * host thread standing in for phase C — ndep entries stored in shuffled batches, each batch in
 * pieces, over an earlier frame's marks; skip != 0 leaves entries j % |skip| == 0 unstored,
 * and skip < 0 then ends the frame with a failure (-2).  Returns the number of wrong pixmap bytes (0) or the
 * sweep's failure status (< 0); -1 for ndep outside 1 .. 2^24. */
int rc_debug_scatter_selftest(int64_t ndep, int64_t seed, int skip);
/* Test aid: what the carry resolver published in the current device's last one-frame-at-a-time
 * parity frame (rc_render on one GPU, rc_render_device), copied out of that frame's workspace
 * once the device is idle.  *ndep: its DEP pixels.  With cap >= *ndep also pix (the DEP pixels'
 * indices y * W + x in scan order), carry (3 floats per entry: the carry-in the entry was
 * resolved to, decoded from its three tagged granules) and hit (1 where some bounce level hit at
 * that carry-in: the tags' bit 31); with a smaller cap only *ndep is written.  *first_bad
 * (optional): the first entry whose three tags are not all the frame's epoch, -1 when every one
 * is.  Returns 0; -1 when the workspace holds no parity frame; -2 when the frame's hand-off
 * failed.  No kernel runs and no render path changes. */
int rc_debug_carry_ins(int64_t cap, int64_t *ndep, int64_t *pix, float *carry, uint8_t *hit,
                       int64_t *first_bad);
/* Wait for every submitted frame, then release the current device's frame pipeline (its
 * CU-partitioned streams and events; the frame workspaces stay allocated).  The next
 * rc_frame_submit builds it again, re-reading RC_PIPE_* from the environment.  Returns what
 * rc_frames_wait would. */
int rc_pipe_reset(void);

/* Resolver diagnostics of the current device (a slow frame's own record): lone = 1 covers the
 * one-frame-at-a-time renders read back since the previous call with lone = 1 (reset), lone =
 * 0 the last rc_frames_wait window.  resolve_ms_* per frame from the resolver's HIP events (frames
 * in flight; 0 for lone frames); grid / res_cus = the last frame's resolver workgroups and the CUs
 * its stream may use; wg_per_cu = workgroups per CU of that placement, wg_per_cu_max = what one
 * CU can hold with k_resolve's registers and LDS reservation (occupancy API): fewer than the
 * placement needs would leave the grid partly queued behind resident workgroups; team rounds
 * = the most rounds of each kind one frame's team made; spin_wait_us_max[site] = the longest
 * bounded wait of any frame (sites: team hand-off, phase C carry-in, ready queue, helper
 * queue; waits under 10 us are not recorded); clock_mhz_* = the shader clock each frame's
 * resolver ran at (a throttled box explains a slow frame). */
typedef struct rc_resolver_stats {
  int64_t frames;
  double resolve_ms_min, resolve_ms_max, resolve_ms_mean;
  int32_t grid, res_cus, wg_per_cu, wg_per_cu_max;
  int32_t regs, scratch_bytes, lds_bytes, team_blocks;
  int32_t scan_rounds_max, cscan_rounds_max, resolve_rounds_max, pad;
  double spin_wait_us_max[4];
  int32_t clock_mhz_min, clock_mhz_max;   /* shader clock over each frame's resolver run
                                             (s_memtime vs s_memrealtime in workgroup 0) */
} rc_resolver_stats;
_Static_assert(sizeof(rc_resolver_stats) == 120, "rc_resolver_stats layout (ctypes binding)");
int rc_resolver_stats_get(int lone, rc_resolver_stats *out);

/* Duration (ms) of the last call's dominant kernel on the current device (the carry
 * resolver in parity mode, the render kernel otherwise), from HIP events on its stream. */
double rc_last_kernel_ms(void);

/* Per-phase kernel timing averaged over every render of the current device issued between
 * rc_profile_begin() and rc_profile_end() (HIP events on the render stream; no extra
 * synchronisation inside the window; at most 64 calls are kept). */
typedef struct rc_phase_stats {
  int calls;
  int parity;
  double phase_a_ms;    /* parity: phase A (all pixels, first-bounce-miss pixels deferred) */
  double compact_ms;    /* parity: scan-order DEP compaction + segment table               */
  double resolve_ms;    /* parity: carry-chain resolver                                    */
  double phase_c_ms;    /* parity: shading of the deferred pixels                          */
  double render_ms;     /* fast / depth 0: the single render kernel                        */
  double total_ms;      /* first kernel start to last kernel end                           */
} rc_phase_stats;
int rc_profile_begin(void);
int rc_profile_end(rc_phase_stats *out);

/* ---- schedule tuning (process-wide) -------------------------------------------------
 * The product's schedule is fixed by rc_default_tuning(); these fields exist so tests and
 * experiments can select the measured alternatives explicitly instead of
 * through the environment.  rc_set_tuning validates every field (returns -1 and changes
 * nothing when one is out of range); the resolver's co-residency limits are enforced on
 * top of it.  Takes effect at the next render (the frame pipeline's layout at its next
 * build: rc_pipe_reset). */
typedef struct rc_tuning {
  int side;               /* a lone parity frame's phase C: 0 after the resolver, 1 beside
                             it (k_side), 2 beside it for images of >= 8 Mpixel, 3 inside
                             the resolver (its idle waves shade ready batches; default), 4
                             inside it until its own work is over (k_finish: the rest)    */
  int split_shade;        /* 1: phase A's colours move beside the resolver (needs side)    */
  int resolve_shared;     /* 1: no one-resolver-workgroup-per-CU LDS reservation           */
  int resolve_lds_kb;     /* resolver LDS reservation in KiB, 0 = by path (96 / 56)        */
  int resolve_grid;       /* resolver workgroups, 0 = resident capacity (>= 8 otherwise)   */
  int team_blocks;        /* long-segment team workgroups, -1 = by path (128 / 3/8 grid)   */
  int helpers;            /* dense-run helper workgroups of a lone frame (0..64; pipeline lanes use none) */
  int hand_run;           /* changes in a row before a wave hands its run to a helper       */
  int long_len;           /* segments of >= long_len entries go to the team                 */
  int wave_k;             /* clean cooperative steps before a wave window returns to LANE   */
  int resolve_k;          /* the same for the team leader's block window                     */
  int coop;               /* 1: cooperative (lanes per entry) evaluator                      */
  int dep_fast;           /* 1: clean DEP entries take phase A's primary shade               */
  int o0;                 /* 1: primary rays through the origin-zero intersection forms      */
  int phase_c_finish;     /* 1: phase C after the resolver through k_finish's batch claims   */
  int single_res_cus;     /* lone frames: resolver sized for this many CUs, 0 = all          */
  int pipe_res_cus;       /* frames in flight: resolver partition CUs, 0 = by image size     */
  int pipe_resolvers;     /* frames in flight: resolver lanes (1..4)                          */
  int pipe_slots;         /* frames in flight: frame workspaces (lanes+1 .. 8)                */
  int pipe_timing;        /* 1: resolver timing events per pipelined frame                   */
  int pipe_slotstreams;   /* 1: one stream per slot (A, compaction, C in turn)               */
  int overlap_d2h;        /* 1: rc_render's copy overlaps the resolver (parity)              */
  int staged_d2h;         /* 1: pinned bounce buffers + host pool; 0: runtime pageable copy  */
  int prefault;           /* 1: fault the caller's pixmap in while the GPU renders           */
  int copy_threads;       /* host copy pool threads (1..32; fixed at the pool's first use)   */
  int side_blocks;        /* lone parity frames: at most this many k_side workgroups (phase C
                             beside the resolver), 0 = one per CU                            */
  int comp_stream;        /* frames in flight: compaction on an unmasked top-priority stream
                             (0 never, 1 always, 2 for images of >= 32 Mpixel)              */
  int block_min;          /* regular carry segments of >= block_min entries are resolved by a
                             whole resolver workgroup (block windows) when the grid has a
                             workgroup for each of them, 0 = never (default 3000)            */
  int pipe_inres;         /* frames in flight: phase C inside the resolver lanes (their idle
                             waves shade ready batches) instead of on the pixel partition:
                             0 never (default), 1 until the queue is drained, 2 until the
                             lane's own resolver work is over (k_finish shades the rest)     */
  int x0;                 /* 1: quadrics whose d, e, f are all zero are tested without their
                             cross terms (bit-identical, rc_device.hpp quad_abc; default 1) */
  int resolve_clean;      /* clean 256-entry windows in a row before the team leader hands a
                             RESOLVE round back to the team's SCAN (1..64)                   */
  int shard_lone;         /* 1: a one-rank group renders its image as a lone frame (default);
                             0: through the sharded exchange (wire records, gathers, the
                             root's resolver) like a multi-rank group — test and measurement */
  int team_cscan;         /* 1: the team leader hands a RESOLVE round back after resolve_k clean
                             cooperative steps and the team's next SCAN round is one
                             cooperative step of every team wave (default); 0: the leader's
                             LANE passes and LANE-only SCAN rounds                            */
  int pipe_order;         /* frames in flight: creation order of the CU-masked streams (the
                             runtime maps streams onto hardware queues in creation order): 0
                             lane by lane (resolver, phase C), then the pixel streams; 1
                             resolvers, pixel streams, phase C; 2 pixel streams, phase C,
                             resolvers; 3 each resolver lane on a hardware queue of its own
                             (placeholder streams fill the others; needs two lanes and the
                             default stream layout, else order 2 with a warning); 4 (default)
                             one phase C stream for both lanes and each resolver lane beside
                             an idle placeholder (same conditions as 3; order 0 where they do
                             not hold, and from 32 Mpixel, where order 0's lanes have their
                             compaction streams)                                            */
  int pipe_helpers;       /* frames in flight: dense-run helper workgroups per resolver lane
                             (default 4; 0 = none)                                            */
  int patch_host;         /* rc_render (parity, overlap_d2h): phase C writes the DEP entries'
                             packed colours straight into pinned host memory (zero-copy), so
                             nothing is left to copy when the frame ends, and the host
                             scatters each entry as it arrives, during the frame (default 2);
                             1: scattered after the frame; 0: a device buffer copied after
                             phase C                                                          */
  int share_device;       /* rc_render / raycast() with num_gpus > 1: 0 one device per rank
                             (devices device .. device+num_gpus-1, RCCL; fewer if the box has
                             fewer, with a warning); 1 every rank on `device` with device
                             copies between the ranks (the multi-GPU path on one GPU: tests) */
  int headb_first;        /* one frame at a time: resolver workgroups that skip the whole-
                             workgroup queue of long regular segments and start at once on the
                             per-wave queue, whose front holds the runs that can be dense    */
  int pipe_last_whole;    /* rc_frames_wait runs the window's last frame's phase C on every CU
                             instead of the pixel partition (1, default; 0 = the partition)   */
  int ssaa_fused;         /* fast mode with rc_options.ssaa > 1: 1 the fused kernel (default:
                             subsamples on adjacent lanes, reduced in registers); 0 the two-pass
                             path of the other modes (the s*W x s*H image, then the box filter)
                             — the same bytes, kept for the measurement (scripts/ssaa_ab.py)   */
  int adaptive_blocks;    /* adaptive supersampling: workgroups of the refinement kernel, which
                             stride over the edge list.  0 (default): sized from the CU count;
                             1..4096: exactly that many (1 walks the whole list with one
                             workgroup: tests, scripts/adaptive_ab.py)                         */
  int pin;                /* parity, dep_fast scenes of at most 8 shapes and 16 lights with
                             shapes * lights <= 64: bit 0 (default 1): a phase C wave whose
                             carry-ins all have the same bits computes what depends on the
                             carry point alone once, into a per-wave table;
                             bit 1 is reserved for the resolver's LANE windows and changes
                             nothing yet.  0 = every wave on the per-lane code; the same bytes
                             either way                                                        */
} rc_tuning;
void rc_default_tuning(rc_tuning *t);
int rc_set_tuning(const rc_tuning *t);
void rc_get_tuning(rc_tuning *t);

/* ---- multi-GPU row shards ----------------------------------------------
 * Rows are dealt cyclically (image row y -> rank y % G).  Every rank renders its rows; the
 * root (rank 0) gathers the row blocks over RCCL (ncclGather over xGMI) and undoes the
 * interleave on its device.  Parity mode adds the carry chain's exchange: every rank runs
 * phase A on its rows, the root receives the other ranks' DEP entries and row blocks
 * (ncclSend/ncclRecv; its own are read in place), rebuilds the scan-order DEP list, and its
 * resolver resolves the carry chain and shades every DEP entry (phase C) straight into the
 * image: nothing returns to the ranks.  The output is byte-identical to rc_render on one
 * device. */
#define RC_GROUP_ID_BYTES 128          /* == sizeof(ncclUniqueId) */
enum { RC_XFER_AUTO = 0,   /* RCCL when every rank has its own device, else RC_XFER_COPY */
       RC_XFER_RCCL = 1,   /* RCCL communicators (xGMI)                                 */
       RC_XFER_COPY = 2    /* device copies between the ranks' buffers (one process)    */ };
typedef struct rc_group rc_group;

/* A fresh RCCL unique id: rank 0 of a multi-process job makes one and shares it. */
int rc_group_unique_id(unsigned char id[RC_GROUP_ID_BYTES]);
/* One rank of a multi-process job (one process per GPU) on `device`; collective over the
 * nranks processes (ncclCommInitRank).  NULL on failure. */
rc_group *rc_group_create_rank(int nranks, int rank, const unsigned char id[RC_GROUP_ID_BYTES],
                               int device);
/* All nranks ranks in this process, rank i on devices[i] (ranks may share a device only with
 * RC_XFER_COPY; RC_XFER_AUTO picks).  NULL on failure. */
rc_group *rc_group_create_local(int nranks, const int *devices, int transport);
void rc_group_destroy(rc_group *group);
int rc_group_size(const rc_group *group);
int rc_group_transport(const rc_group *group);   /* RC_XFER_RCCL or RC_XFER_COPY */

/* Render W x H row-sharded over the group: collective (every rank's process calls it with
 * the same arguments).  The image lands in d_image (W*H*3 bytes, device memory of rank 0's
 * device; NULL = a buffer of the group's own) on the root; other ranks ignore d_image.
 * Synchronous.  timing (may be NULL): total_ms (host), kernel_ms (root's device span),
 * resolve_ms, dep_pixels and zero_normalize of the whole image (root).  Returns 0 on
 * success. */
int rc_render_sharded(rc_group *group, const rc_scene *scene, int width, int height,
                      const rc_options *opt, uint8_t *d_image, rc_timing *timing);

typedef struct rc_shard_stats {   /* the last rc_render_sharded, on the root */
  int ranks;
  double total_ms;        /* host wall clock of the call                                   */
  double device_ms;       /* root's stream: first kernel to the de-interleaved image        */
  double local_ms;        /* root's own rows: fast: render; parity: phase A + packing       */
  double exchange_in_ms;  /* parity: end of the root's phase A to the resolver's start (entry
                             and row-block gathers, de-interleave, scan-order rebuild)       */
  double resolve_ms;      /* parity: image-wide carry resolver on the root                  */
  double phase_c_ms;      /* parity: the phase C tail after the root's resolver (phase C runs
                             inside the resolver on the root)                                */
  double image_ms;        /* fast: row-block gather + de-interleave; parity: the image's copy
                             into the caller's buffer (the row blocks are gathered before the
                             resolver, inside exchange_in_ms)                                */
  int64_t dep_pixels;
  int64_t zero_normalize;
  int64_t entry_bytes;    /* DEP entries moved to the root                                  */
  int64_t carry_bytes;    /* carry-ins moved back (0: phase C runs on the root)              */
  int64_t image_bytes;    /* row blocks moved to the root (padded to ceil(H/G) rows)        */
} rc_shard_stats;
int rc_group_last_stats(const rc_group *group, rc_shard_stats *out);
/* One rank's own timeline of the last rc_render_sharded (every rank, root or not; -1 if this
 * process does not drive `rank`): local_ms = its rows (fast: render; parity: phase A + wire
 * records), exchange_ms = from there until its row blocks (and parity entries) have left,
 * total_ms = the whole frame on its stream. */
typedef struct rc_rank_stats {
  int rank;
  int rows;
  double local_ms;
  double exchange_ms;
  double total_ms;
  int64_t dep_pixels;     /* parity: the rank's own DEP entries */
} rc_rank_stats;
int rc_group_rank_stats(const rc_group *group, int rank, rc_rank_stats *out);
/* Parity frames exchange the DEP entries in fixed-size per-rank blocks (no host
 * synchronisation inside the frame) once a frame of the same scene and size has given the
 * per-rank count; a frame that exceeds it is rendered again with exact sizes.  Test aid: set
 * that bound (entries per rank; -1 forgets it). */
int rc_group_debug_bound(rc_group *group, long long per_rank);

/* Library version / build string. */
const char *rc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RAYCAST_HIP_H */
