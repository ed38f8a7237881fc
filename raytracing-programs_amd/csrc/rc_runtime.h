// rc_runtime.h — internal host-runtime state of libraycast_hip.so shared by rc_api.hip (one
// device: rc_render, frames in flight), rc_sampling.hip (the sampling features' entry points)
// and rc_shard.hip (row shards over several devices).
// Not part of the C-ABI (include/raycast_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <mutex>

#include "raycast_hip.h"
#include "rc_kernels.h"
#include "rc_scene.h"

namespace rcrt {

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      std::fprintf(stderr, "Error: HIP call failed: %s (%s) at %s:%d\n", #expr,        \
                   hipGetErrorString(e_), __FILE__, __LINE__);                          \
      return -1;                                                                        \
    }                                                                                   \
  } while (0)

constexpr int kMaxDevices = 16;

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int ensure(size_t need) {
    if (need <= bytes) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    if (hipMalloc(&p, need) != hipSuccess) return -1;
    bytes = need;
    return 0;
  }
};

// One frame's device state: the uploaded scene, the zero-normalize counter and the parity
// workspace.  The plain path has one (DevCtx::fb); pipelined frames alternate two (Pipe).
struct FrameBufs {
  unsigned epoch = 0;   // carry-in tag of the last parity frame in this workspace
  DevBuf zcount;        // zero-normalize counter
  DevBuf scene;         // uploaded packed scene
  const void* scene_src = nullptr;   // host image last uploaded
  DevBuf cls, wcarry, deprec, rows, dep_pix, seg_key, seg_start, seg_order, batch_state, cin,
      counters, team, trace;
};

// Per-frame verification of parity frames.  A frame's carry hand-offs (the resolver team's
// granules, phase C's carry-ins, the helper queue) are bounded spins that record the first
// failure in the frame's TeamState (rc_kernels.hip); the next frame in the same workspace
// resets that state.  So after every parity frame's last kernel the TeamState's first four
// words are copied, on the frame's own stream, into a pinned ring entry the host pre-filled
// with kPending: once the copy has run the entry holds 0 (every hand-off completed) or the
// failure's code, workgroup and details.  The copy precedes the event that gates the
// workspace's next use, so no later frame can erase a failure before the host has read it.
struct FrameLog {
  static constexpr int kRing = 4096;
  static constexpr int kPending = 0x7fffffff;
  struct Entry {
    int code, block, info, info2;   // TeamState.error, err_block, err_info, err_info2
    int rq_prod, rq_cons, helpers_out;
    int n_scan, n_cscan, n_resolve; // the frame's team rounds by kind
    int spin_ticks[4];              // its longest bounded waits per spin site (10 ns ticks)
    int clock_mhz;                  // shader clock over its resolver's run (0: not measured)
    int team_row;                   // TeamState::team_row: 1 + last row of a long segment
  };
  // Frame diagnostics of the entries read back since the last diag_take(): frames, the most
  // team rounds of each kind in one frame, the longest wait per spin site.
  struct Diag {
    long long frames = 0;
    int scan_max = 0, cscan_max = 0, resolve_max = 0;
    int spin_ticks_max[4] = {0, 0, 0, 0};
    int clock_min = 0, clock_max = 0;   // MHz, over the frames that measured it
  };
  Diag diag;
  Entry* ring = nullptr;     // pinned host memory, kRing entries
  long long head = 0;        // frames logged
  long long tail = 0;        // frames whose entry has been read back (in order)
  long long checked = 0;     // entries read back since the last take()
  long long failed = 0;      // of them, frames whose hand-off failed
  const char* what = "";
  // Log the frame whose TeamState is `team` (device) on `st`, after its last kernel.
  int enqueue(const void* team, hipStream_t st);
  // Read back the entries whose copy has run (in order, stopping at the first still
  // pending); reports each failure on stderr.  Returns the failures found.
  long long poll();
  // After the frames' streams are synchronised: every entry must have run (a pending one
  // counts as a failure).  Returns the failures found.
  long long drain();
  // A failure read back now or earlier and not yet taken (poll() first).
  bool earlier_failed();
  // Entry k (a frame's index at its enqueue) has run and its hand-off failed.  Only for an
  // entry whose stream has been synchronised and that poll() has not read back yet.
  bool entry_failed(long long k) const;
  // checked / failed since the last take(), then reset.
  void take(long long* c, long long* f);
  // the diagnostics since the last diag_take(), then reset
  Diag diag_take() {
    Diag d = diag;
    diag = Diag{};
    return d;
  }
};

// Pipelined parity frames (rc_frame_submit).  The device's CUs are split in two partitions
// (hipExtStreamCreateWithCUMask).  Partition A runs the carry resolvers: kLanes resolver
// streams, each resolver grid sized to A/kLanes CUs (one workgroup per CU), so the resolvers in
// flight are always wholly resident side by side (a team spins on co-resident workgroups;
// at most kLanes resolvers are in flight since each stream runs its resolvers in order).
// Partition B runs the pixel phases: the frames' phase A one at a time in submission order
// (each waits for the previous frame's, adone), so the frame whose resolver comes next always
// has the whole partition; two streams (pix[0], pix[1]) alternate so a frame's compaction —
// a chain of small latency-bound kernels — overlaps the next frame's phase A; each lane's
// phase C runs on a stream of its own (pc[lane], after the frame's resolver); a slot's next
// phase A waits for the slot's previous phase C (cdone).  A resolver is
// latency-bound (its carry chains), so overlapping kLanes of them multiplies the frame rate
// until partition B's pixel work becomes the bound.  (RC_PIPE_SLOTSTREAMS: the earlier form,
// one stream per slot running A, compaction and C in turn.)
struct Pipe {
  static constexpr int kSlots = 8;   // frame workspaces (a frame re-uses slot k after k's end)
  static constexpr int kLanes = 4;   // resolvers in flight (at most)
  bool init = false;
  int res_cus = 0;                   // CUs in partition A
  int lanes = 2;                     // resolver streams in use (RC_PIPE_RESOLVERS)
  int slots = 4;                     // workspaces / pixel streams in use (RC_PIPE_SLOTS)
  hipStream_t pix[kSlots] = {}, res[kLanes] = {};
  hipStream_t comp[2] = {};          // compaction: no CU mask, highest priority (comp_stream)
  hipEvent_t ready[kSlots] = {}, done[kSlots] = {};
  bool fifo = true;                  // pa = pix[0] + pc[] (false: RC_PIPE_SLOTSTREAMS)
  hipStream_t pc[kLanes] = {};
  hipStream_t spare[2] = {};         // pipe_order 3/4: placeholders that keep a queue per lane
  bool pc_shared = false;            // pipe_order 4: both lanes' phase C on one stream (pc[0])
  hipEvent_t cdone[kSlots] = {};
  bool cpend[kSlots] = {};           // slot k's phase C is enqueued and not yet synchronised
  hipEvent_t adone[kSlots] = {};     // after slot k's phase A
  static constexpr int kEv = 64;     // resolver timing events of the last kEv frames
  hipEvent_t rt[kEv][2] = {};
  FrameBufs fb[kSlots];
  long long submitted = 0;           // parity frames since the last rc_frames_wait
  long long frames = 0;              // frames of any mode since the last rc_frames_wait
  long long total = 0;               // parity frames ever (slot / stream rotation)
  long long last = -1;               // slot of the last parity frame
  bool used[kSlots] = {};
  bool rt_on = true;                 // resolver timing events recorded (RC_PIPE_NO_RT: off)
  int built_lanes = 0, built_slots = 0, built_res = 0, built_order = 0;   // the tuning it was built with
  FrameLog log;                      // every pipelined parity frame, in submission order
  // the last submitted parity frame's phase C: launched at the next submit (on its lane's
  // phase C stream) or by rc_frames_wait (on every CU: nothing else is left to run beside it)
  bool cdefer = false;
  int cdefer_lane = 0, cdefer_k = 0, cdefer_W = 0, cdefer_H = 0, cdefer_maxrec = 0;
  rc::LaunchScene cdefer_ls{};
  rc::ParityWork cdefer_w{};
  uint8_t* cdefer_out = nullptr;
  unsigned long long* cdefer_zc = nullptr;
};

// The sampling features whose frames leave phase spans behind (DevCtx::span_ev).
enum SpanOwner {
  kSpanAdaptive, kSpanRates, kSpanFilter, kSpanPattern, kSpanAccum, kSpanWindow, kSpanGbuffer,
  kSpanView, kSpanAo, kSpanOwners
};

// The sampling features' frame records.  Each documents the events its rc_*_phase_ms reads out
// of the event set it owns (DevCtx::span_ev), an accumulation pass through a window being an
// accumulation call that records as one.
//
// The last list-refined frame of one feature on a device (adaptive supersampling, a pattern
// frame with a threshold): what its stats getter reads.  Adaptive spans: [0] start, [2] one-ray
// image, [3] list, [1] refinement.
struct ListFrame {
  DevBuf count;                // 8-byte counter block (word 0: entries), zeroed on the frame's
                               // stream before the list is made
  hipEvent_t done = nullptr;   // behind the frame's refinement
  bool valid = false;          // such a frame has been enqueued on this device
  long long pixels = 0;        // its W*H
  int rays = 0;                // rays per refined pixel
};

// Sparse sample patterns (rc_render_pattern*): the edge list of a frame with a threshold lives in
// DevCtx::aa_list; the record keeps a counter block of its own so that rc_pattern_stats_get
// outlives a later adaptive frame.  Without a threshold (threshold = 0) every pixel is refined
// and neither the counter nor `done` is used.  Spans: [0] start, [1] end, and with a threshold
// (ev_listed) [2] [3] as adaptive.
struct PatternFrame : ListFrame {
  int threshold = 0;
  bool ev_listed = false;
};

// Rate-map supersampling (rc_render_rates*): the rate-4 list lives in DevCtx::aa_list; `list`
// holds the rate-2 list (upwards from its start) and the rate-8 list (downwards from its end),
// W*H entries; `count` is the counter block (five words, launch_rates_render), zeroed on the
// frame's stream; `map` is rc_render_rates' device copy of the host map.  Spans: [0] start, [2]
// the rate-1 pass, [1] the refinement.
struct RateFrame {
  DevBuf list, count, map;
  hipEvent_t done = nullptr;   // behind the last rate-map frame's refinement
  bool valid = false;          // a rate-map frame has been enqueued on this device
};

// A timed two-pass supersampled frame (enqueue_render_two_pass).  Spans: [0] start, `mid`
// between the s*W x s*H image and its filter, [end] behind the filter.
struct FilterFrame {
  hipEvent_t mid = nullptr;
  int end = 1;
};

// The last accumulation call of a device (rc_accum_pass_device: one pass; rc_render_accum: all
// of its passes): what rc_accum_stats_get reads.  Pass k owns slot k of the counter block, two
// words {pixels listed by the edge list, saturated pixels}, so no pass waits for the host; the
// block is the call's own, so the counts outlive the other sampling features' frames.  Spans:
// [0] start and [1] end of the call, [ev_first] the start of its last pass and, when that pass
// ran over the edge list (ev_listed), [3] behind the list.
struct AccumFrame {
  static constexpr int kSlots = 128;   // >= 4 dense chunks + 63 single-sample passes
  DevBuf count;                // kSlots * 8 bytes, zeroed on the call's stream before its passes
  hipEvent_t done = nullptr;   // behind the call's last pass
  bool valid = false;          // such a call has been enqueued on this device
  long long pixels = 0;        // its W*H
  int passes = 0;
  uint8_t samples[kSlots] = {};   // per pass: its sample count
  bool listed[kSlots] = {};       // per pass: it ran over the edge list (threshold > 0)
  int ev_first = 0;
  bool ev_listed = false;
};

// The primary-visibility G-buffer (rc_render_gbuffer*, rc_pick*): the host entries' device copies
// of the planes they were asked for, of the points and of the records; the *_device entries use
// the caller's memory and nothing of this.  Spans: [0] start, [1] end of the one kernel.
struct GbufFrame {
  DevBuf id, t, P, N;   // rc_render_gbuffer's planes
  DevBuf xy, hits;      // rc_pick's points and records
};

// Rotated views and ray batches (rc_render_view*, rc_trace_rays*): the host entry's device copies
// of the directions and of the outputs it was asked for; rc_render_view uses DevCtx::out and the
// *_device entries the caller's memory.  Spans: [0] start, [1] end of the one kernel.
struct ViewFrame {
  DevBuf dirs, rgb8, rgb, hits;   // rc_trace_rays' arrays
  DevBuf origins;                 // rc_trace_rays_from's second input
};

// Any-hit visibility and ambient occlusion (rc_ao_pass_device, rc_render_ao, rc_occluded_rays*):
// `count` is the last pass's counter block (launch_ao's lines, rc::kAoStatBytes), zeroed on the
// call's stream in front of every pass, so that it holds the last pass's counts; `n`: that pass's
// directions.
// The host forms' device copies: rc_render_ao's state and plane, rc_occluded_rays' arrays.
// Spans: [0] start, [1] end of the call's kernels.
struct AoFrame {
  DevBuf count;
  hipEvent_t done = nullptr;   // behind the call's last pass
  bool valid = false;          // a pass has been enqueued on this device
  int n = 0;
  DevBuf state, plane;
  DevBuf origins, dirs, skip, tmax, flags;
};

// rc_render_ambient's device copies (the host form of the guided family): the occlusion state, the
// guide's id, P and N planes and the filtered plane; the image is c.out.  The camera G-buffer and
// the compose keep nothing on the device, the filter not even a workspace frame.
struct GuidedFrame {
  DevBuf state, id, P, N, plane;
};

struct DevCtx {
  bool init = false;
  int device = 0;
  hipStream_t side = nullptr;   // phase C's side stream
  hipEvent_t fork = nullptr, join = nullptr;
  int side_blocks = 0, side_lds = 0;
  int side_for_lds = -1;        // the resolver LDS reservation side_lds / side_blocks were sized for
  int cus = 256;
  hipStream_t stream = nullptr;
  // event sets: [0] start, then per phase ends (fast: [1] = render; parity: [1] phase A,
  // [2] compaction, [3] resolver, [4] phase C; adaptive supersampling: [2] the one-ray image,
  // [3] the edge list, [1] the refinement; the other sampling features: at their records
  // above).  Set 0 serves plain calls; inside an
  // rc_profile_begin/end window every call takes the next set of the pool.
  static constexpr int kEvSets = 64;
  hipEvent_t ev[kEvSets][5] = {};
  int prof_active = 0, prof_calls = 0, prof_parity = 0;
  DevBuf out;          // rc_render output pixmap
  DevBuf ssaa;         // two-pass supersampling: the s*W x s*H image before the box filter
  // adaptive supersampling: the edge list (uint32 pixel index, W*H entries of room); its frame
  // record is `aa`
  DevBuf aa_list;
  ListFrame aa;
  RateFrame rates;     // rate-map supersampling
  PatternFrame pat;    // sparse sample patterns
  FilterFrame filt;    // two-pass supersampling's timed frames
  // progressive supersampling: rc_render_accum's accumulator (rc_accum_pass_device's is the
  // caller's); a masked pass's edge list lives in aa_list; `acc` is the last call's record
  DevBuf accum_px;
  AccumFrame acc;
  GbufFrame gbuf;      // the G-buffer's host entries
  ViewFrame view;      // rc_trace_rays' arrays
  AoFrame ao;          // ambient occlusion's last pass and the host forms' arrays
  GuidedFrame guided;  // rc_render_ambient's planes
  // The event set whose spans each sampling feature's rc_*_phase_ms may still read, null once
  // another frame has recorded that set anew (claim_event_set).  Which events of the set a
  // feature reads is documented at its record above; window (rc_render_window*): [0] start,
  // [1] end; the G-buffer and pick frames and the view and ray frames likewise.
  hipEvent_t* span_ev[kSpanOwners] = {};
  uint8_t* stage[2] = {nullptr, nullptr};   // pinned bounce buffers of copy_to_host
  hipEvent_t stage_ev[2] = {nullptr, nullptr};
  FrameBufs fb;        // scene, counter and parity workspace of the plain path
  Pipe pipe;
  int resident_blocks = 0;
  int resident_lds = -1;
  static constexpr int kResCache = 4;   // resident resolver grids per LDS reservation
  int res_lds[kResCache] = {};
  int res_blocks[kResCache] = {};
  size_t parity_pixels = 0;
  int parity_rows = 0;
  // rc_render's overlapped copy (parity): the framebuffer leaves on `d2h` while the resolver
  // runs, then only the DEP entries' colours (`patch`, packed RGB per entry) follow
  hipStream_t d2h = nullptr;
  DevBuf patch;
  uint8_t* pin_pix = nullptr;     // pinned: DEP pixel indices (int64 per entry)
  uint8_t* pin_patch = nullptr;   // pinned: DEP entries' packed RGB
  size_t pin_bytes = 0;           // capacity of each pinned buffer, in entries
  int* pin_cnt = nullptr;         // pinned: counters[0..3]
  uint8_t* pin_tail = nullptr;    // pinned: rc_render's frame counts (fill_device_timing)
  uint32_t* host_patch = nullptr;     // pinned, mapped: phase C's packed RGB per DEP entry
  uint32_t* host_patch_dev = nullptr; // its device address (patch_host)
  size_t host_patch_entries = 0;
  size_t host_patch_dirty = 0;       // entries below it may hold a mark since the last clear
  unsigned host_patch_epoch0 = 0;    // epoch before the first frame since that clear
  FrameLog lone_log;   // every parity frame rendered in `fb` (rc_render, rc_render_device)
  // rc_resolver_stats: the last rc_frames_wait window's record (frames in flight), and the
  // resolver placement of the last frame of each kind (grid, CUs it may use)
  rc_resolver_stats pipe_stats{};
  int lone_grid = 0, lone_res_cus = 0, lone_lds = 0, lone_team = 0;
  int pipe_grid = 0, pipe_res_cus = 0, pipe_lds = 0, pipe_team = 0;
  // `fb` is shared by every one-frame-at-a-time call on this device, and rc_render_device
  // returns before its frame has run: the next enqueue on `fb` from another stream waits for
  // the previous one (ws_ev, recorded after it on ws_stream).
  hipEvent_t ws_ev = nullptr;
  hipStream_t ws_stream = nullptr;
  bool ws_valid = false;
  // One render at a time per device: the workspace, TeamState, events and streams above are
  // shared by every call on this device (rc_render, rc_render_device, rc_frame_submit).
  std::mutex mu;
};

extern DevCtx g_ctx[kMaxDevices];

// process-wide schedule tuning (rc_set_tuning; defaults = the product's schedule): a copy
// taken under the tuning lock, so a render reads one consistent set of fields
rc_tuning tune();
int ctx_get(int device, DevCtx** out);
int fill_resolver_stats(DevCtx& c, const FrameLog::Diag& d, int grid, int res_cus, int lds,
                        int team, rc_resolver_stats* r);
// the host-side copy helpers take the caller's one tuning snapshot (rc_render)
int copy_to_host(DevCtx& c, uint8_t* host, const uint8_t* dev, size_t bytes, hipStream_t st,
                 const rc_tuning& tu);
int ensure_host_patch(DevCtx& c, size_t entries, unsigned epoch);
void prefault(DevCtx& c, uint8_t* p, size_t n, const rc_tuning& tu);
int upload_scene(FrameBufs& b, hipStream_t stream, const rc_scene* s, rc::LaunchScene& ls);
int ensure_parity(DevCtx& c, FrameBufs& b, int W, int H, rc::ParityWork& w, int res_cus,
                  int piped_lane = -1);
int report_spin_error(const FrameBufs& b, const char* where);
double event_ms(hipEvent_t a, hipEvent_t b);
// One render of rows row0 + k*row_step into d_out on `stream` through the device's one-frame
// workspace (rc_render_device's path; the caller holds c.mu).  timed: phase events c.ev[0].
int enqueue_render(DevCtx& c, const rc_scene* s, int W, int H, int row0, int row_step, int nrows,
                   const rc_options* opt, uint8_t* d_out, hipStream_t stream, bool timed,
                   uint32_t* patch = nullptr, hipEvent_t** evset = nullptr,
                   const rc_filter* filt = nullptr);
// filt (with a plain factor of 2, 4 or 8 in opt->ssaa, every mode): the s*W x s*H image through
// the two-pass path and filt's taps instead of the box (the caller has passed rc_filter_check)
// rc_options.ssaa as a factor: 1 (0 and 1 are both off), 2, 4 or 8; -1 and a message naming
// `who` for any other value
int ssaa_factor(const rc_options* opt, const char* who);
// rc_options.ssaa's adaptive threshold t: 0 (off) or 1..255 with a factor of 2, 4 or 8; -1 and
// a message naming `who` otherwise (ssaa_factor's refusals included)
int ssaa_threshold(const rc_options* opt, const char* who);
int check_spin_error(FrameBufs& b, const rc_options* opt);
void fill_device_timing(DevCtx& c, const rc_options* opt, rc_timing* t,
                        const uint8_t* tail = nullptr);

// ------------------------------------------- the frame scaffold (rc_api.hip) --
// A device call's context with its lock held (one render at a time per device, DevCtx::mu).
struct Entered {
  DevCtx* c = nullptr;
  std::unique_lock<std::mutex> lk;
};
constexpr int kCurrentDevice = -1;

// Enter a call on `device` (made current) or on the current one (kCurrentDevice).  The lock
// covers the workspace from its (re)allocation on: a concurrent caller's ensure() could
// otherwise free the buffer another caller is rendering into.  render: an earlier frame of this
// workspace whose hand-off failed (rc_render_device on another stream) is reported by the next
// render call, before its own frame is enqueued (once: the report consumes the counts).
int enter(int device, bool render, Entered& e);
// a host-pixmap render entry: on opt->device
int enter_host(const rc_options* opt, Entered& e);
// ms[i] = the span marks[i] -> marks[i + 1], once the last mark has completed
int read_spans(std::initializer_list<hipEvent_t> marks, double* ms);
// the listed pixels of f's frame, from its counter block once its refinement has run
int list_frame_refined(const ListFrame& f, int64_t* refined);

// The pending phase C (Pipe::cdefer) of the last submitted frame: on its lane's phase C
// stream, or with `whole` on the device stream over every CU — the window's last frame, whose
// phase C otherwise ran alone on the pixel partition after the last resolver (0.8 ms of a
// 20-frame window's drain at quadric 4096^2 against ~0.47 ms on every CU).
int flush_phase_c(DevCtx& c, bool whole);

// The workspace bracket of a frame on `stream` through the device's one-frame workspace c.fb:
// after the previous frame that used it, whatever its stream.  prepare() is what the frame
// allocates before it waits for the workspace (a failure there leaves the stream untouched),
// body() enqueues the frame.
template <class Prepare, class Body>
int ws_frame(DevCtx& c, hipStream_t stream, Prepare prepare, Body body) {
  // a frame in flight's held-back phase C goes out first, so that a device synchronisation
  // after this call completes it (rc_frames_wait stays the frames' completion point)
  if (flush_phase_c(c, false) || prepare()) return -1;
  if (c.ws_valid && c.ws_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, c.ws_ev, 0));
  const int rc = body();
  // recorded even after a failed enqueue: whatever was enqueued stays ordered
  HIP_TRY(hipEventRecord(c.ws_ev, stream));
  c.ws_stream = stream;
  c.ws_valid = true;
  return rc;
}

// The event set of the frame being enqueued: set 0, or inside an rc_profile_begin/end window
// the next set of the pool.  The ownership rule of the sets' spans (DevCtx::span_ev) is here and
// nowhere else: a frame that records the set anew (`records`) takes it from every feature that
// still points at it, so no rc_*_phase_ms reads another frame's spans; `owner` (or kSpanOwners
// for none) loses its own spans whatever set they were in, until the frame's enqueue has
// succeeded and stores the set in span_ev[owner].  Under profiling consecutive frames record
// different sets, so several owners can stay valid at once.
hipEvent_t* claim_event_set(DevCtx& c, int owner, bool parity, bool records);

constexpr long long kNoLog = -1;   // `own` of a frame that logs no hand-off entry

// The tail of a device-resident call: without a timing record it returns with its frame
// enqueued; with one it waits for the frame.  own (or kNoLog): the frame's entry in lone_log,
// for the calls whose frame may be a parity frame.
int finish_device(DevCtx& c, const rc_options* opt, hipStream_t st, rc_timing* timing,
                  long long own);

using HostClock = std::chrono::steady_clock;

// The tail of a host-pixmap call whose frame is enqueued on c.stream with its image in c.out:
// the copy into the caller's pixmap, the wait, the timing record (t0: the call's entry).
// What the entry points do differently is explicit: tail_counts (the frame's counts through
// pin_tail rather than two copies after the frame), prefault (the pixmap is faulted in while the
// GPU renders), own (or kNoLog: the frame's hand-off entry is verified).
struct HostTail {
  bool tail_counts, prefault;
  long long own;
};
int finish_host(DevCtx& c, const rc_options* opt, uint8_t* pixmap, size_t bytes,
                const rc_tuning& tu, const HostTail& how, rc_timing* timing,
                HostClock::time_point t0);

// rc_shard.hip: rc_render's multi-GPU path (a cached in-process group over devices
// first..first+n-1, or n ranks sharing device `first` with device copies between them when
// `share`); *d_image = the root's de-interleaved image.  The caller holds no lock.
int render_local_group(int first, int n, bool share, const rc_scene* s, int W, int H,
                       const rc_options* opt, uint8_t** d_image, rc_timing* timing);

}  // namespace rcrt

// the packed scene behind the opaque rc_scene handle
struct rc_scene {
  rc_packed_header* img;   // host packed image
};
