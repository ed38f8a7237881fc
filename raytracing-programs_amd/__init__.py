"""raytracing-programs_amd — Python host bindings of the MI355X raycaster.

The product is C: ``lib/libraycast_hip.so`` (HIP kernels + the C-ABI declared in
``include/raycast_hip.h``) and ``lib/libraycast_front.so`` (scene parser / P3 writer with the
reference's names and behaviour, C/parse.c, C/objects.c, C/ppm.c).  This module only binds
them with ctypes so tests and ``bench.py`` can drive the same entry points the C CLI uses:

    scene = Scene.from_file("tests/golden/scenes/quadric.scene")   # parse_json (C/parse.c:13)
    img = render(scene, 4096, 4096, depth=6, mode="parity")       # raycast (C/raycast.h:8)

There is no CPU fallback: loading fails loudly if the shared libraries are missing, and a
render fails if no GPU is present.  Import name: ``raytracing_programs_amd`` (the directory
name has a hyphen; ``__graft_entry__`` and tests load it by path).
"""
import contextlib
import ctypes
import os
import sys
import threading

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(PKG_DIR, "lib")
BIN_DIR = os.path.join(PKG_DIR, "bin")
ROOT_DIR = os.path.dirname(PKG_DIR)

MODE_PARITY = 0
MODE_FAST = 1
MODE_CUDA = 2   # the CUDA port's semantics (include/raycast_hip.h RC_MODE_CUDA)
MODES = {"parity": MODE_PARITY, "fast": MODE_FAST, "cuda": MODE_CUDA}


# ------------------------------------------------------------------ ABI structs --
class ShapeT(ctypes.Structure):
    """shape_t, C/objects.h:15-49 (104 bytes)."""
    _fields_ = [("diffuse_color", ctypes.c_float * 3), ("specular_color", ctypes.c_float * 3),
                ("position", ctypes.c_float * 3), ("reflectivity", ctypes.c_float),
                ("refractivity", ctypes.c_float), ("ior", ctypes.c_float),
                ("u", ctypes.c_float * 10), ("type", ctypes.c_int),
                ("next", ctypes.c_void_p)]


class LightT(ctypes.Structure):
    """light_t, C/objects.h:51-61 (72 bytes)."""
    _fields_ = [("position", ctypes.c_float * 3), ("color", ctypes.c_float * 3),
                ("radial_coef", ctypes.c_float * 3), ("theta", ctypes.c_float),
                ("cos_theta", ctypes.c_float), ("a0", ctypes.c_float),
                ("direction", ctypes.c_float * 3), ("type", ctypes.c_int),
                ("next", ctypes.c_void_p)]


class JsonDataT(ctypes.Structure):
    """json_data_t, C/parse.h:11-18."""
    _fields_ = [("camera_width", ctypes.c_float), ("camera_height", ctypes.c_float),
                ("shapes_list", ctypes.POINTER(ShapeT)), ("lights_list", ctypes.POINTER(LightT)),
                ("num_shapes", ctypes.c_int), ("num_lights", ctypes.c_int)]


class PPMFormat(ctypes.Structure):
    """PPMFormat, C/ppm.h:6-12."""
    _fields_ = [("width", ctypes.c_int), ("height", ctypes.c_int), ("size", ctypes.c_int),
                ("maxColor", ctypes.c_uint8), ("depth", ctypes.c_uint8),
                ("tupleType", ctypes.c_char_p), ("pixmap", ctypes.c_void_p)]


class RcOptions(ctypes.Structure):
    _fields_ = [("max_recursion", ctypes.c_int), ("mode", ctypes.c_int),
                ("num_gpus", ctypes.c_int), ("device", ctypes.c_int), ("ssaa", ctypes.c_int)]


class RcTiming(ctypes.Structure):
    _fields_ = [("total_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("resolve_ms", ctypes.c_double), ("d2h_ms", ctypes.c_double),
                ("dep_pixels", ctypes.c_int64), ("zero_normalize", ctypes.c_int64),
                ("frames_checked", ctypes.c_int64), ("frames_failed", ctypes.c_int64)]


class RcAdaptiveStats(ctypes.Structure):
    _fields_ = [("refined_pixels", ctypes.c_int64), ("rays", ctypes.c_int64)]


class RcRateStats(ctypes.Structure):
    """rc_rate_stats (48 bytes): pixels with rate 1, 2, 4, 8; invalid map bytes; rays shot."""
    _fields_ = [("pixels", ctypes.c_int64 * 4), ("invalid", ctypes.c_int64),
                ("rays", ctypes.c_int64)]


FILTER_MAX_TAPS = 24


class RcFilter(ctypes.Structure):
    """rc_filter (52 bytes): the tap count L and the int16 taps k[0..L)."""
    _fields_ = [("ntaps", ctypes.c_int32), ("taps", ctypes.c_int16 * FILTER_MAX_TAPS)]


# the output tile (width, height) one workgroup of the filter kernel owns, per factor
# (csrc/rc_kernels.h filter_tile_w / filter_tile_h)
FILTER_TILES = {2: (32, 16), 4: (32, 8), 8: (16, 8)}


PATTERN_MAX_SAMPLES = 16


class RcPattern(ctypes.Structure):
    """rc_pattern (40 bytes): the lattice g, the sample count n and the positions px, py."""
    _fields_ = [("grid", ctypes.c_int32), ("nsamples", ctypes.c_int32),
                ("x", ctypes.c_uint8 * PATTERN_MAX_SAMPLES),
                ("y", ctypes.c_uint8 * PATTERN_MAX_SAMPLES)]


class RcPatternStats(ctypes.Structure):
    _fields_ = [("refined_pixels", ctypes.c_int64), ("rays", ctypes.c_int64)]


# the built-in sample patterns (rc_pattern_builtin): name -> (g, [(x, y), ...]), x to the right
# and y downwards on the g x g subsample lattice of a pixel
PATTERNS = {
    "diag2": (2, [(0, 0), (1, 1)]),
    "rgss4": (4, [(1, 0), (3, 1), (0, 2), (2, 3)]),
    "checker8": (4, [(i, j) for j in range(4) for i in range(4) if (i + j) % 2 == 0]),
    "queens8": (8, [(c, r) for r, c in enumerate([3, 6, 2, 7, 1, 4, 0, 5])]),
}

ACCUM_MAX_SAMPLES = 64    # a sample sequence's length at most
ACCUM_MAX_N = 256         # samples a pixel's record can hold
ACCUM_MAX_COUNT = 16      # samples a pass adds at most


class RcAccumPx(ctypes.Structure):
    """rc_accum_px (8 bytes): a pixel's sums of the n sample bytes taken so far, and n."""
    _fields_ = [("sum", ctypes.c_uint16 * 3), ("n", ctypes.c_uint16)]


class RcSampleSeq(ctypes.Structure):
    """rc_sample_seq (136 bytes): the lattice g, the length and the positions x, y."""
    _fields_ = [("grid", ctypes.c_int32), ("nsamples", ctypes.c_int32),
                ("x", ctypes.c_uint8 * ACCUM_MAX_SAMPLES),
                ("y", ctypes.c_uint8 * ACCUM_MAX_SAMPLES)]


class RcAccumStats(ctypes.Structure):
    _fields_ = [("passes", ctypes.c_int64), ("active_pixels", ctypes.c_int64),
                ("saturated", ctypes.c_int64), ("rays", ctypes.c_int64)]


class RcWindow(ctypes.Structure):
    """rc_window (16 bytes): the virtual image and the window's top left pixel inside it."""
    _fields_ = [("full_w", ctypes.c_int32), ("full_h", ctypes.c_int32),
                ("x0", ctypes.c_int32), ("y0", ctypes.c_int32)]


class RcGbuffer(ctypes.Structure):
    """rc_gbuffer (32 bytes): the four plane pointers, null for a plane that is not wanted."""
    _fields_ = [("id", ctypes.c_void_p), ("t", ctypes.c_void_p), ("P", ctypes.c_void_p),
                ("N", ctypes.c_void_p)]


class RcHit(ctypes.Structure):
    """rc_hit (32 bytes): one picked point's record."""
    _fields_ = [("id", ctypes.c_int32), ("t", ctypes.c_float), ("P", ctypes.c_float * 3),
                ("N", ctypes.c_float * 3)]


# the planes of a G-buffer in rc_gbuffer's order: name -> (dtype, components)
GBUFFER_PLANES = {"id": (np.int32, 1), "t": (np.float32, 1), "P": (np.float32, 3),
                  "N": (np.float32, 3)}
# rc_hit as a numpy record; id -1: no primary hit, -2 (pick_device only): a point outside the image
HIT_DTYPE = np.dtype([("id", np.int32), ("t", np.float32), ("P", np.float32, 3),
                      ("N", np.float32, 3)])
assert HIT_DTYPE.itemsize == ctypes.sizeof(RcHit) == ctypes.sizeof(RcGbuffer) == 32
PICK_MAX_POINTS = 1 << 24


class RcView(ctypes.Structure):
    """rc_view (36 bytes): the 3 x 3 view matrix, row-major."""
    _fields_ = [("m", ctypes.c_float * 9)]


class RcRayOut(ctypes.Structure):
    """rc_ray_out (32 bytes): the three output pointers of a ray batch, null for one that is not
    wanted, and the frame flag (P and N in the records)."""
    _fields_ = [("rgb8", ctypes.c_void_p), ("rgb", ctypes.c_void_p), ("hits", ctypes.c_void_p),
                ("frame", ctypes.c_int32)]


class RcCamera(ctypes.Structure):
    """rc_camera (48 bytes): the eye and the view."""
    _fields_ = [("eye", ctypes.c_float * 3), ("view", RcView)]


assert ctypes.sizeof(RcView) == 36 and ctypes.sizeof(RcRayOut) == 32
assert ctypes.sizeof(RcCamera) == 48
RAYS_MAX = 1 << 24
# the outputs of a ray batch in rc_ray_out's order: name -> (dtype, trailing shape)
RAY_OUTPUTS = {"rgb8": (np.uint8, (3,)), "rgb": (np.float32, (3,)), "hits": (HIT_DTYPE, ())}

AO_MAX_DIRS = 64          # directions of one set at most
AO_MAX_RAYS = 65535       # occlusion rays a pixel's record can hold
AO_MAX_SETS = 1024        # sets of one render_ao call at most


class RcAoDirs(ctypes.Structure):
    """rc_ao_dirs (776 bytes): n directions, used as given, and one tmax in units of their length."""
    _fields_ = [("n", ctypes.c_int32), ("tmax", ctypes.c_float),
                ("u", (ctypes.c_float * 3) * AO_MAX_DIRS)]


class RcAoStats(ctypes.Structure):
    _fields_ = [("hit_pixels", ctypes.c_int64), ("rays", ctypes.c_int64),
                ("blocked", ctypes.c_int64), ("saturated", ctypes.c_int64)]


# rc_ao_px as a numpy record: `rays` occlusion rays counted for the pixel, `open` of them not blocked
AO_DTYPE = np.dtype([("open", np.uint16), ("rays", np.uint16)])
assert ctypes.sizeof(RcAoDirs) == 776 and AO_DTYPE.itemsize == 4

AO_FILTER_MAX_RADIUS = 8      # the guided filter pools up to 17 x 17 neighbours
AO_FILTER_MAX_WEIGHT = 32768  # the weights of one window sum to this at most


class RcAoFilter(ctypes.Structure):
    """rc_ao_filter (32 bytes): the pooling window's radius, the two thresholds and taps[|d|]."""
    _fields_ = [("radius", ctypes.c_int32), ("nmin", ctypes.c_float), ("dplane", ctypes.c_float),
                ("taps", ctypes.c_uint16 * (AO_FILTER_MAX_RADIUS + 1)), ("pad", ctypes.c_uint16)]


assert ctypes.sizeof(RcAoFilter) == 32


def _hier_points(g):
    """hier<g> (include/raycast_hip.h, rc_sample_seq): point k is the bit-reversal r of k over
    2 * log2 g bits; x takes r's even bits and y its odd bits."""
    lg = g.bit_length() - 1
    pts = []
    for k in range(g * g):
        r = sum(((k >> b) & 1) << (2 * lg - 1 - b) for b in range(2 * lg))
        pts.append((sum(((r >> (2 * i)) & 1) << i for i in range(lg)),
                    sum(((r >> (2 * i + 1)) & 1) << i for i in range(lg))))
    return pts


# the built-in sample sequences (rc_sample_seq_builtin): name -> (g, [(x, y), ...]); the patterns
# in their own order and the whole lattice coarse to fine
SAMPLE_SEQS = dict({name: (g, list(pts)) for name, (g, pts) in PATTERNS.items()},
                   **{f"hier{g}": (g, _hier_points(g)) for g in (2, 4, 8)})


# the values a rate map's bytes may take (rc_render_rates): 0 leaves the pixel alone
RATE_VALUES = (0, 1, 2, 4, 8)


class RcPhaseStats(ctypes.Structure):
    _fields_ = [("calls", ctypes.c_int), ("parity", ctypes.c_int), ("phase_a_ms", ctypes.c_double),
                ("compact_ms", ctypes.c_double), ("resolve_ms", ctypes.c_double),
                ("phase_c_ms", ctypes.c_double), ("render_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double)]


class RcShardStats(ctypes.Structure):
    _fields_ = [("ranks", ctypes.c_int), ("total_ms", ctypes.c_double),
                ("device_ms", ctypes.c_double), ("local_ms", ctypes.c_double),
                ("exchange_in_ms", ctypes.c_double), ("resolve_ms", ctypes.c_double),
                ("phase_c_ms", ctypes.c_double), ("image_ms", ctypes.c_double),
                ("dep_pixels", ctypes.c_int64), ("zero_normalize", ctypes.c_int64),
                ("entry_bytes", ctypes.c_int64), ("carry_bytes", ctypes.c_int64),
                ("image_bytes", ctypes.c_int64)]


class RcRankStats(ctypes.Structure):
    _fields_ = [("rank", ctypes.c_int), ("rows", ctypes.c_int), ("local_ms", ctypes.c_double),
                ("exchange_ms", ctypes.c_double), ("total_ms", ctypes.c_double),
                ("dep_pixels", ctypes.c_int64)]


class RcResolverStats(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_int64), ("resolve_ms_min", ctypes.c_double),
                ("resolve_ms_max", ctypes.c_double), ("resolve_ms_mean", ctypes.c_double),
                ("grid", ctypes.c_int32), ("res_cus", ctypes.c_int32),
                ("wg_per_cu", ctypes.c_int32), ("wg_per_cu_max", ctypes.c_int32),
                ("regs", ctypes.c_int32), ("scratch_bytes", ctypes.c_int32),
                ("lds_bytes", ctypes.c_int32), ("team_blocks", ctypes.c_int32),
                ("scan_rounds_max", ctypes.c_int32), ("cscan_rounds_max", ctypes.c_int32),
                ("resolve_rounds_max", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("spin_wait_us_max", ctypes.c_double * 4),
                ("clock_mhz_min", ctypes.c_int32), ("clock_mhz_max", ctypes.c_int32)]


TUNING_FIELDS = ["side", "split_shade", "resolve_shared", "resolve_lds_kb", "resolve_grid",
                 "team_blocks", "helpers", "hand_run", "long_len", "wave_k", "resolve_k", "coop",
                 "dep_fast", "o0", "phase_c_finish", "single_res_cus", "pipe_res_cus",
                 "pipe_resolvers", "pipe_slots", "pipe_timing", "pipe_slotstreams", "overlap_d2h",
                 "staged_d2h", "prefault", "copy_threads", "side_blocks", "comp_stream",
                 "block_min", "pipe_inres", "x0", "resolve_clean",
                 "shard_lone", "team_cscan", "pipe_order", "pipe_helpers", "patch_host",
                 "share_device", "headb_first", "pipe_last_whole", "ssaa_fused",
                 "adaptive_blocks"]


# fields appended to rc_tuning after the list above was closed (its last name is pinned by tests)
TUNING_TAIL = ["pin"]


class RcTuning(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in TUNING_FIELDS + TUNING_TAIL]


assert ctypes.sizeof(ShapeT) == 104 and ctypes.sizeof(LightT) == 72

# the functions include/raycast_hip.h declares, per library
HIP_EXPORTS = ["raycast", "rc_default_options", "rc_scene_create", "rc_scene_destroy",
               "rc_scene_parity_defined", "rc_render", "rc_render_device", "rc_last_kernel_ms",
               "rc_profile_begin", "rc_profile_end", "rc_version", "rc_frame_submit",
               "rc_frames_wait", "rc_pipe_reset", "rc_group_unique_id", "rc_group_create_rank",
               "rc_group_create_local", "rc_group_destroy", "rc_group_size",
               "rc_group_transport", "rc_render_sharded", "rc_group_last_stats",
               "rc_default_tuning", "rc_set_tuning", "rc_get_tuning", "rc_lone_frames_check",
               "rc_debug_inject_error", "rc_group_debug_bound", "rc_resolver_stats_get",
               "rc_group_rank_stats", "rc_debug_scatter_selftest", "rc_debug_carry_ins",
               "rc_adaptive_stats_get",
               "rc_adaptive_phase_ms", "rc_render_rates", "rc_render_rates_device",
               "rc_rate_stats_get", "rc_rate_phase_ms", "rc_filter_box", "rc_filter_tent",
               "rc_filter_check", "rc_filter_env", "rc_render_filtered",
               "rc_render_filtered_device", "rc_filter_image_device", "rc_filter_phase_ms",
               "rc_pattern_builtin", "rc_pattern_check", "rc_pattern_env", "rc_render_pattern",
               "rc_render_pattern_device", "rc_pattern_stats_get", "rc_pattern_phase_ms",
               "rc_sample_seq_builtin", "rc_sample_seq_check", "rc_accum_pass_device",
               "rc_accum_resolve_device", "rc_render_accum", "rc_accum_stats_get",
               "rc_accum_phase_ms", "rc_window_check", "rc_window_env", "rc_render_window",
               "rc_render_window_device", "rc_accum_pass_window_device",
               "rc_render_gbuffer", "rc_render_gbuffer_device", "rc_pick", "rc_pick_device",
               "rc_id_edge_rates_device", "rc_gbuffer_phase_ms", "rc_view_check",
               "rc_render_view", "rc_render_view_device", "rc_trace_rays",
               "rc_trace_rays_device", "rc_view_phase_ms", "rc_camera_check",
               "rc_render_camera", "rc_render_camera_device", "rc_trace_rays_from",
               "rc_trace_rays_from_device", "rc_accum_pass_camera_device",
               "rc_render_camera_accum", "rc_ao_dirs_check", "rc_occluded_rays",
               "rc_occluded_rays_device", "rc_ao_pass_device", "rc_ao_resolve_device",
               "rc_render_ao", "rc_ao_stats_get", "rc_ao_phase_ms", "rc_render_camera_gbuffer",
               "rc_render_camera_gbuffer_device", "rc_ao_filter_box", "rc_ao_filter_tent",
               "rc_ao_filter_check", "rc_ao_filter_device", "rc_ao_compose_device",
               "rc_render_ambient"]
FRONT_EXPORTS = ["add_new_sphere", "add_new_plane", "add_new_quadric", "free_shape_list",
                 "free_light_list", "add_new_spot_light", "add_new_point_light", "parse_json",
                 "set_to_black", "ppm_WriteOutP3", "ppm_clamp"]

_libs = {}


def _load(name):
    if name not in _libs:
        path = os.path.join(LIB_DIR, name)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build with `make` (or __graft_entry__.build())")
        _libs[name] = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    return _libs[name]


def front_lib():
    lib = _load("libraycast_front.so")
    lib.parse_json.argtypes = [ctypes.c_void_p, ctypes.POINTER(JsonDataT)]
    lib.parse_json.restype = None
    lib.free_shape_list.argtypes = [ctypes.c_void_p]
    lib.free_shape_list.restype = ctypes.c_void_p
    lib.free_light_list.argtypes = [ctypes.c_void_p]
    lib.free_light_list.restype = ctypes.c_void_p
    lib.ppm_WriteOutP3.argtypes = [PPMFormat, ctypes.c_void_p]
    lib.ppm_WriteOutP3.restype = None
    return lib


_torch_tried = False


def _one_hip_runtime():
    """PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so, SONAME
    libamdhip64.so.7, which torch's libraries reference as plain `libamdhip64.so`).  If
    libraycast_hip.so loaded /opt/rocm's runtime first and torch were imported later, the
    loader would map a second HIP runtime into the process (two device contexts; their
    teardown corrupts the heap at exit).  Importing torch first makes libraycast_hip.so's
    `libamdhip64.so.7` / `librccl.so.1` resolve to the runtime already loaded: one per
    process.  Without torch, /opt/rocm's runtime is the only one."""
    global _torch_tried
    if _torch_tried or "torch" in sys.modules:
        return
    _torch_tried = True   # once: a failed import is not retried on every call
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


_HIP_LOCK = threading.Lock()
_hip = None


def hip_lib():
    # RC_HIP_LIB selects a diagnostic build (e.g. libraycast_hip_stamps.so); never the default.
    # Under a lock: threads making their first call at once must not load the library while
    # another is still importing torch (a half-imported torch is already in sys.modules, and
    # the library would then map /opt/rocm's HIP runtime beside torch's: _one_hip_runtime).
    # Once bound, later calls take the cached handle without the lock.
    lib = _hip
    if lib is not None:
        return lib
    with _HIP_LOCK:
        return _hip_lib_locked()


def _hip_lib_locked():
    global _hip
    if _hip is not None:
        return _hip
    _one_hip_runtime()
    lib = _load(os.environ.get("RC_HIP_LIB", "libraycast_hip.so"))
    lib.rc_scene_create.argtypes = [ctypes.POINTER(JsonDataT)]
    lib.rc_scene_create.restype = ctypes.c_void_p
    lib.rc_scene_destroy.argtypes = [ctypes.c_void_p]
    lib.rc_scene_parity_defined.argtypes = [ctypes.c_void_p]
    lib.rc_render.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                              ctypes.POINTER(RcOptions), ctypes.c_void_p, ctypes.POINTER(RcTiming)]
    lib.rc_render_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.POINTER(RcOptions),
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(RcTiming)]
    lib.rc_frame_submit.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(RcOptions), ctypes.c_void_p]
    lib.rc_frames_wait.argtypes = [ctypes.POINTER(RcTiming)]
    lib.rc_pipe_reset.argtypes = []
    lib.rc_last_kernel_ms.restype = ctypes.c_double
    lib.rc_version.restype = ctypes.c_char_p
    lib.rc_default_options.argtypes = [ctypes.POINTER(RcOptions), ctypes.c_int]
    lib.rc_profile_end.argtypes = [ctypes.POINTER(RcPhaseStats)]
    lib.rc_group_unique_id.argtypes = [ctypes.c_char_p]
    lib.rc_group_create_rank.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    lib.rc_group_create_rank.restype = ctypes.c_void_p
    lib.rc_group_create_local.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.rc_group_create_local.restype = ctypes.c_void_p
    lib.rc_group_destroy.argtypes = [ctypes.c_void_p]
    lib.rc_group_size.argtypes = [ctypes.c_void_p]
    lib.rc_group_transport.argtypes = [ctypes.c_void_p]
    lib.rc_render_sharded.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(RcOptions), ctypes.c_void_p,
                                      ctypes.POINTER(RcTiming)]
    lib.rc_group_last_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcShardStats)]
    lib.rc_group_debug_bound.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    lib.rc_default_tuning.argtypes = [ctypes.POINTER(RcTuning)]
    lib.rc_default_tuning.restype = None
    lib.rc_get_tuning.argtypes = [ctypes.POINTER(RcTuning)]
    lib.rc_get_tuning.restype = None
    lib.rc_set_tuning.argtypes = [ctypes.POINTER(RcTuning)]
    lib.rc_lone_frames_check.argtypes = [ctypes.POINTER(ctypes.c_int64),
                                         ctypes.POINTER(ctypes.c_int64)]
    lib.rc_debug_inject_error.argtypes = [ctypes.c_int]
    lib.rc_resolver_stats_get.argtypes = [ctypes.c_int, ctypes.POINTER(RcResolverStats)]
    lib.rc_group_rank_stats.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(RcRankStats)]
    lib.rc_adaptive_stats_get.argtypes = [ctypes.POINTER(RcAdaptiveStats)]
    lib.rc_adaptive_phase_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.rc_render_rates.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(RcOptions), ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.POINTER(RcTiming)]
    lib.rc_render_rates_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                           ctypes.POINTER(RcOptions), ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.POINTER(RcTiming)]
    lib.rc_rate_stats_get.argtypes = [ctypes.POINTER(RcRateStats)]
    lib.rc_rate_phase_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.rc_filter_box.argtypes = [ctypes.c_int, ctypes.POINTER(RcFilter)]
    lib.rc_filter_tent.argtypes = [ctypes.c_int, ctypes.POINTER(RcFilter)]
    lib.rc_filter_check.argtypes = [ctypes.POINTER(RcFilter), ctypes.c_int]
    lib.rc_filter_env.argtypes = [ctypes.POINTER(RcOptions), ctypes.POINTER(RcFilter)]
    lib.rc_render_filtered.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                       ctypes.POINTER(RcOptions), ctypes.POINTER(RcFilter),
                                       ctypes.c_void_p, ctypes.POINTER(RcTiming)]
    lib.rc_render_filtered_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                              ctypes.POINTER(RcOptions), ctypes.POINTER(RcFilter),
                                              ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.POINTER(RcTiming)]
    lib.rc_filter_image_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.POINTER(RcFilter),
                                           ctypes.c_void_p, ctypes.c_void_p]
    lib.rc_filter_phase_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.rc_pattern_builtin.argtypes = [ctypes.c_char_p, ctypes.POINTER(RcPattern)]
    lib.rc_pattern_check.argtypes = [ctypes.POINTER(RcPattern)]
    lib.rc_pattern_env.argtypes = [ctypes.POINTER(RcOptions), ctypes.POINTER(RcPattern),
                                   ctypes.POINTER(ctypes.c_int)]
    lib.rc_render_pattern.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(RcOptions), ctypes.POINTER(RcPattern),
                                      ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(RcTiming)]
    lib.rc_render_pattern_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(RcOptions), ctypes.POINTER(RcPattern),
                                             ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.POINTER(RcTiming)]
    lib.rc_pattern_stats_get.argtypes = [ctypes.POINTER(RcPatternStats)]
    lib.rc_pattern_phase_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.rc_sample_seq_builtin.argtypes = [ctypes.c_char_p, ctypes.POINTER(RcSampleSeq)]
    lib.rc_sample_seq_check.argtypes = [ctypes.POINTER(RcSampleSeq)]
    lib.rc_accum_pass_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                         ctypes.POINTER(RcOptions), ctypes.POINTER(RcSampleSeq),
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.POINTER(RcTiming)]
    lib.rc_accum_resolve_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_void_p]
    lib.rc_render_accum.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(RcOptions), ctypes.POINTER(RcSampleSeq),
                                    ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                    ctypes.POINTER(RcTiming)]
    lib.rc_accum_stats_get.argtypes = [ctypes.POINTER(RcAccumStats)]
    lib.rc_accum_phase_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.rc_window_check.argtypes = [ctypes.POINTER(RcWindow), ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int]
    lib.rc_window_env.argtypes = [ctypes.POINTER(RcOptions), ctypes.c_int, ctypes.c_int,
                                  ctypes.POINTER(RcWindow)]
    lib.rc_render_window.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcWindow), ctypes.c_int,
                                     ctypes.c_int, ctypes.POINTER(RcOptions), ctypes.c_void_p,
                                     ctypes.POINTER(RcTiming)]
    lib.rc_render_window_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcWindow),
                                            ctypes.c_int, ctypes.c_int, ctypes.POINTER(RcOptions),
                                            ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.POINTER(RcTiming)]
    lib.rc_accum_pass_window_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcWindow),
                                                ctypes.c_int, ctypes.c_int,
                                                ctypes.POINTER(RcOptions),
                                                ctypes.POINTER(RcSampleSeq), ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.POINTER(RcTiming)]
    lib.rc_accum_scroll_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcWindow), ctypes.c_int,
                                           ctypes.c_int, ctypes.POINTER(RcOptions),
                                           ctypes.POINTER(RcSampleSeq), ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.POINTER(RcTiming)]
    lib.rc_render_gbuffer.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcWindow), ctypes.c_int,
                                      ctypes.c_int, ctypes.POINTER(RcOptions),
                                      ctypes.POINTER(RcGbuffer), ctypes.POINTER(RcTiming)]
    lib.rc_render_gbuffer_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcWindow),
                                             ctypes.c_int, ctypes.c_int, ctypes.POINTER(RcOptions),
                                             ctypes.POINTER(RcGbuffer), ctypes.c_void_p,
                                             ctypes.POINTER(RcTiming)]
    lib.rc_pick.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(RcOptions),
                            ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib.rc_pick_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                   ctypes.POINTER(RcOptions), ctypes.c_int, ctypes.c_int64,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.rc_id_edge_rates_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.c_void_p]
    lib.rc_gbuffer_phase_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.rc_view_check.argtypes = [ctypes.POINTER(RcView)]
    lib.rc_render_view.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcView),
                                   ctypes.POINTER(RcWindow), ctypes.c_int, ctypes.c_int,
                                   ctypes.POINTER(RcOptions), ctypes.c_void_p,
                                   ctypes.POINTER(RcTiming)]
    lib.rc_render_view_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcView),
                                          ctypes.POINTER(RcWindow), ctypes.c_int, ctypes.c_int,
                                          ctypes.POINTER(RcOptions), ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.POINTER(RcTiming)]
    lib.rc_trace_rays.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcOptions), ctypes.c_int64,
                                  ctypes.c_void_p, ctypes.POINTER(RcRayOut)]
    lib.rc_trace_rays_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcOptions),
                                         ctypes.c_int64, ctypes.c_void_p,
                                         ctypes.POINTER(RcRayOut), ctypes.c_void_p]
    lib.rc_view_phase_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.rc_camera_check.argtypes = [ctypes.POINTER(RcCamera)]
    lib.rc_render_camera.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcCamera),
                                     ctypes.POINTER(RcWindow), ctypes.c_int, ctypes.c_int,
                                     ctypes.POINTER(RcOptions), ctypes.c_void_p,
                                     ctypes.POINTER(RcTiming)]
    lib.rc_render_camera_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcCamera),
                                            ctypes.POINTER(RcWindow), ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(RcOptions), ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.POINTER(RcTiming)]
    lib.rc_trace_rays_from.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcOptions), ctypes.c_int64,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(RcRayOut)]
    lib.rc_trace_rays_from_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcOptions),
                                              ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.POINTER(RcRayOut), ctypes.c_void_p]
    lib.rc_accum_pass_camera_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcCamera),
                                                ctypes.c_int, ctypes.POINTER(RcWindow),
                                                ctypes.c_int, ctypes.c_int,
                                                ctypes.POINTER(RcOptions),
                                                ctypes.POINTER(RcSampleSeq), ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.POINTER(RcTiming)]
    lib.rc_render_camera_accum.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcCamera),
                                           ctypes.c_int, ctypes.POINTER(RcWindow), ctypes.c_int,
                                           ctypes.c_int, ctypes.POINTER(RcOptions),
                                           ctypes.POINTER(RcSampleSeq), ctypes.c_void_p,
                                           ctypes.POINTER(RcTiming)]
    lib.rc_ao_dirs_check.argtypes = [ctypes.POINTER(RcAoDirs)]
    for name in ("rc_occluded_rays", "rc_occluded_rays_device"):
        getattr(lib, name).argtypes = [ctypes.c_void_p, ctypes.POINTER(RcOptions), ctypes.c_int64,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.POINTER(RcTiming)]
    lib.rc_ao_pass_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcCamera),
                                      ctypes.POINTER(RcWindow), ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(RcOptions), ctypes.POINTER(RcAoDirs),
                                      ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.POINTER(RcTiming)]
    lib.rc_ao_resolve_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_void_p]
    lib.rc_render_ao.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcCamera),
                                 ctypes.POINTER(RcWindow), ctypes.c_int, ctypes.c_int,
                                 ctypes.POINTER(RcOptions), ctypes.POINTER(RcAoDirs), ctypes.c_int,
                                 ctypes.c_void_p, ctypes.POINTER(RcTiming)]
    lib.rc_ao_stats_get.argtypes = [ctypes.POINTER(RcAoStats)]
    lib.rc_ao_phase_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.rc_render_camera_gbuffer.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcCamera),
                                             ctypes.POINTER(RcWindow), ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(RcOptions), ctypes.POINTER(RcGbuffer),
                                             ctypes.POINTER(RcTiming)]
    lib.rc_render_camera_gbuffer_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcCamera),
                                                    ctypes.POINTER(RcWindow), ctypes.c_int,
                                                    ctypes.c_int, ctypes.POINTER(RcOptions),
                                                    ctypes.POINTER(RcGbuffer), ctypes.c_void_p,
                                                    ctypes.POINTER(RcTiming)]
    for name in ("rc_ao_filter_box", "rc_ao_filter_tent"):
        getattr(lib, name).argtypes = [ctypes.c_int, ctypes.POINTER(RcAoFilter)]
    lib.rc_ao_filter_check.argtypes = [ctypes.POINTER(RcAoFilter)]
    lib.rc_ao_filter_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcGbuffer), ctypes.c_int,
                                        ctypes.c_int, ctypes.POINTER(RcAoFilter), ctypes.c_void_p,
                                        ctypes.c_void_p]
    lib.rc_ao_compose_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcOptions),
                                         ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.POINTER(ctypes.c_float), ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p]
    lib.rc_render_ambient.argtypes = [ctypes.c_void_p, ctypes.POINTER(RcCamera),
                                      ctypes.POINTER(RcWindow), ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(RcOptions), ctypes.POINTER(RcAoDirs),
                                      ctypes.c_int, ctypes.POINTER(RcAoFilter),
                                      ctypes.POINTER(ctypes.c_float), ctypes.c_void_p,
                                      ctypes.POINTER(RcTiming)]
    _hip = lib
    return lib


_libc = ctypes.CDLL(None)
_libc.fopen.restype = ctypes.c_void_p
_libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
_libc.fclose.argtypes = [ctypes.c_void_p]
_libc.open_memstream.restype = ctypes.c_void_p
_libc.open_memstream.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
_libc.free.argtypes = [ctypes.c_void_p]


_PACK_LOCK = threading.Lock()


class Scene:
    """A parsed scene: the reference's json_data_t lists plus the packed device scene."""

    def __init__(self, js):
        self.js = js
        self._packed = None

    @classmethod
    def from_file(cls, path):
        """parse_json (C/parse.c:13) through libraycast_front.so.  Like the reference, a
        malformed file makes the parser print to stderr and exit(1)."""
        lib = front_lib()
        f = _libc.fopen(os.fsencode(path), b"r")
        if not f:
            raise FileNotFoundError(path)
        js = JsonDataT()
        try:
            lib.parse_json(f, ctypes.byref(js))
        finally:
            _libc.fclose(f)
        return cls(js)

    @property
    def num_shapes(self):
        return self.js.num_shapes

    @property
    def num_lights(self):
        return self.js.num_lights

    def shapes(self):
        out, p = [], self.js.shapes_list
        while p:
            out.append(p.contents)
            p = ctypes.cast(p.contents.next, ctypes.POINTER(ShapeT))
        return out

    def lights(self):
        out, p = [], self.js.lights_list
        while p:
            out.append(p.contents)
            p = ctypes.cast(p.contents.next, ctypes.POINTER(LightT))
        return out

    def packed(self):
        """rc_scene handle (packed image + phantom record) for the HIP library."""
        with _PACK_LOCK:   # render threads sharing a Scene create its handle once
            if self._packed is None:
                h = hip_lib().rc_scene_create(ctypes.byref(self.js))
                if not h:
                    raise RuntimeError("rc_scene_create failed")
                self._packed = h
            return self._packed

    def parity_defined(self):
        return bool(hip_lib().rc_scene_parity_defined(self.packed()))

    def close(self):
        if self._packed is not None:
            hip_lib().rc_scene_destroy(self._packed)
            self._packed = None
        lib = front_lib()
        if self.js.shapes_list:
            lib.free_shape_list(ctypes.cast(self.js.shapes_list, ctypes.c_void_p))
            self.js.shapes_list = None
        if self.js.lights_list:
            lib.free_light_list(ctypes.cast(self.js.lights_list, ctypes.c_void_p))
            self.js.lights_list = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def get_tuning(default=False):
    """The process-wide schedule tuning (rc_get_tuning / rc_default_tuning) as a dict."""
    t = RcTuning()
    (hip_lib().rc_default_tuning if default else hip_lib().rc_get_tuning)(ctypes.byref(t))
    return {n: getattr(t, n) for n in TUNING_FIELDS + TUNING_TAIL}


def set_tuning(**fields):
    """Change tuning fields (the rest keep their current values); rc_set_tuning validates."""
    cur = get_tuning()
    unknown = set(fields) - set(cur)
    if unknown:
        raise KeyError(f"unknown tuning fields {sorted(unknown)}")
    cur.update(fields)
    t = RcTuning(**cur)
    if hip_lib().rc_set_tuning(ctypes.byref(t)) != 0:
        raise ValueError(f"rc_set_tuning rejected {fields}")


class tuned:
    """Context manager: `with tuned(side=0): ...` renders with the given tuning, then restores."""

    def __init__(self, **fields):
        self.fields = fields

    def __enter__(self):
        self.saved = get_tuning()
        set_tuning(**self.fields)
        return self

    def __exit__(self, *exc):
        set_tuning(**self.saved)
        return False


def ssaa_adaptive(s, t):
    """RC_SSAA_ADAPTIVE(s, t): rc_options.ssaa with the factor s and the contrast threshold t."""
    return int(s) | (int(t) << 8)


def ssaa_factor(v):
    """RC_SSAA_FACTOR(v)."""
    return int(v) & 0xff


def ssaa_threshold(v):
    """RC_SSAA_THRESHOLD(v)."""
    return (int(v) >> 8) & 0xff


def options(depth=6, mode="parity", gpus=1, device=0, ssaa=1, adaptive=0):
    """rc_options; adaptive = t > 0 encodes RC_SSAA_ADAPTIVE(ssaa, t) (the library validates)."""
    opt = RcOptions()
    opt.max_recursion = depth + 1
    opt.mode = MODES[mode] if isinstance(mode, str) else int(mode)
    opt.num_gpus = gpus
    opt.device = device
    opt.ssaa = ssaa_adaptive(ssaa, adaptive) if adaptive else ssaa
    return opt


def default_options(use_env=False):
    """rc_default_options as a dict (with use_env: the RAYCAST_* environment applied); "ssaa" is
    the factor and "adaptive" the threshold (0: off) of the encoded field."""
    opt = RcOptions()
    hip_lib().rc_default_options(ctypes.byref(opt), 1 if use_env else 0)
    d = {k: getattr(opt, k) for k, _ in RcOptions._fields_}
    d["ssaa"], d["adaptive"] = ssaa_factor(opt.ssaa), ssaa_threshold(opt.ssaa)
    return d


def box_downsample(img, s):
    """The supersampling contract (include/raycast_hip.h, rc_options.ssaa) in numpy: the
    [H, W, 3] uint8 box filter of an [s*H, s*W, 3] uint8 image, per channel
    (sum of the s x s block + s*s/2) // (s*s)."""
    img = np.asarray(img)
    s = int(s)
    if s < 1 or img.dtype != np.uint8 or img.ndim != 3 or img.shape[0] % s or img.shape[1] % s:
        raise ValueError(f"box_downsample: a uint8 [s*H, s*W, C] image and s >= 1, got "
                         f"{img.dtype} {img.shape} and s = {s}")
    h, w, c = img.shape[0] // s, img.shape[1] // s, img.shape[2]
    total = img.reshape(h, s, w, s, c).sum(axis=(1, 3), dtype=np.uint32)
    return ((total + (s * s) // 2) // (s * s)).astype(np.uint8)


def _window_range(a):
    """max - min over the 3 x 3 window, clipped to the image, per channel: [H, W, C] int."""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3:
        raise ValueError(f"a uint8 [H, W, C] image, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    lo = np.pad(a, ((1, 1), (1, 1), (0, 0)), constant_values=255)
    hi = np.pad(a, ((1, 1), (1, 1), (0, 0)), constant_values=0)
    mn, mx = a.copy(), a.copy()
    for dy in range(3):
        for dx in range(3):
            mn = np.minimum(mn, lo[dy:dy + h, dx:dx + w])
            mx = np.maximum(mx, hi[dy:dy + h, dx:dx + w])
    return mx.astype(np.int32) - mn.astype(np.int32)


def edge_mask(a, t):
    """The adaptive contract's edge test (include/raycast_hip.h, RC_SSAA_ADAPTIVE) in numpy:
    [H, W] bool, true where the largest per-channel max - min of the uint8 image `a` over the
    3 x 3 window centred on the pixel, clipped to the image, is >= t."""
    return _window_range(a).max(axis=2) >= int(t)


def adaptive_compose(a, f, t):
    """The adaptive contract: `f` (the ssaa = s image) where edge_mask(a, t), `a` (the one-ray
    image) elsewhere."""
    a, f = np.asarray(a), np.asarray(f)
    if a.shape != f.shape or f.dtype != np.uint8:
        raise ValueError(f"two uint8 images of one shape, got {a.shape} and {f.dtype} {f.shape}")
    return np.where(edge_mask(a, t)[:, :, None], f, a)


def _pixmap(out, width, height, fresh=np.empty):
    """The caller's [H, W, 3] uint8 C-contiguous pixmap, or a fresh one when `out` is None."""
    if out is None:
        out = fresh((height, width, 3), dtype=np.uint8)
    assert out.shape == (height, width, 3) and out.dtype == np.uint8 and out.flags.c_contiguous
    return out


def _timing_back(timing, t):
    """Copy the RcTiming record `t` into the caller's dict (None: the caller wants none)."""
    if timing is not None:
        timing.update({k: getattr(t, k) for k, _ in RcTiming._fields_})


def _call(name, *args):
    """The library's export `name` with `args`; a non-zero return raises."""
    if getattr(hip_lib(), name)(*args) != 0:
        raise RuntimeError(f"{name} failed (see stderr)")


@contextlib.contextmanager
def _timed(timing):
    """A call's RcTiming record and the argument of a *_device entry (the record by reference,
    or None when the caller wants no timing: the call then returns with its frame enqueued);
    after the call the record goes into the caller's dict."""
    t = RcTiming()
    yield t, ctypes.byref(t) if timing is not None else None
    _timing_back(timing, t)


def _stream(stream_ptr):
    """A stream argument: the caller's hipStream_t, or null for the context's own."""
    return ctypes.c_void_p(stream_ptr or 0)


def _host_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _stats(name, cls, message, *lead):
    """The fields of the stats struct `cls` that the getter `name` fills, as a dict."""
    st = cls()
    if getattr(hip_lib(), name)(*lead, ctypes.byref(st)) != 0:
        raise RuntimeError(message)
    return {k: getattr(st, k) for k, _ in cls._fields_}


def _phase_ms(name, keys, message):
    """The kernel spans that the getter `name` reads, in ms, under `keys`."""
    ms = (ctypes.c_double * len(keys))()
    if getattr(hip_lib(), name)(ms) != 0:
        raise RuntimeError(message)
    return dict(zip(keys, ms))


def render(scene, width, height, depth=6, mode="parity", gpus=1, device=0, timing=None, out=None,
           ssaa=1, adaptive=0):
    """Render to a host array [H, W, 3] uint8 through rc_render (the raycast() path); `out`
    (optional) is the caller's C-contiguous pixmap, like the reference's malloc'd one.  ssaa =
    2, 4 or 8: the box filter of the ssaa*W x ssaa*H image (box_downsample), made on the device.
    adaptive = t in 1..255 (fast and cuda mode, with ssaa): only the pixels of the one-ray image
    whose 3 x 3 contrast reaches t are supersampled (adaptive_compose)."""
    out = _pixmap(out, width, height)
    opt = options(depth, mode, gpus, device, ssaa, adaptive)
    with _timed(timing) as (t, _):
        if hip_lib().rc_render(scene.packed(), width, height, ctypes.byref(opt), _host_ptr(out),
                               ctypes.byref(t)) != 0:
            raise RuntimeError("rc_render failed (no GPU, or HIP error: see stderr)")
    return out


def render_device(scene, width, height, d_out_ptr, stream_ptr=None, depth=6, mode="parity",
                  row0=0, row_step=1, nrows=None, timing=None, ssaa=1, adaptive=0):
    """Render rows row0, row0+row_step, ... into device memory at d_out_ptr (nrows*W*3 B); with
    ssaa > 1 the rows are those of the box-filtered W x H image.  adaptive > 0: whole images
    only."""
    nrows = height if nrows is None else nrows
    opt = options(depth, mode, ssaa=ssaa, adaptive=adaptive)
    with _timed(timing) as (_, t):
        _call("rc_render_device", scene.packed(), width, height, row0, row_step, nrows,
              ctypes.byref(opt), ctypes.c_void_p(d_out_ptr), _stream(stream_ptr), t)


def frame_submit(scene, width, height, d_out_ptr, depth=6, mode="parity", ssaa=1, adaptive=0):
    """Enqueue one whole image into device memory at d_out_ptr (W*H*3 B) with frames in
    flight (rc_frame_submit); returns at once.  Pair with frames_wait().  ssaa > 1 (and
    adaptive): fast and cuda mode only (parity frames in flight do not supersample)."""
    opt = options(depth, mode, ssaa=ssaa, adaptive=adaptive)
    _call("rc_frame_submit", scene.packed(), width, height, ctypes.byref(opt),
          ctypes.c_void_p(d_out_ptr))


def frames_wait(timing=None):
    """Block until every submitted frame is complete (rc_frames_wait)."""
    t = RcTiming()
    if hip_lib().rc_frames_wait(ctypes.byref(t)) != 0:
        raise RuntimeError(f"rc_frames_wait failed: {t.frames_failed} of {t.frames_checked} "
                           "frames' carry hand-offs failed (see stderr)")
    _timing_back(timing, t)


def adaptive_stats():
    """The last adaptive frame enqueued on the current device (rc_adaptive_stats_get, which
    waits for it): {"refined_pixels": pixels with contrast >= t, "rays": W*H + s*s*that}."""
    return _stats("rc_adaptive_stats_get", RcAdaptiveStats,
                  "rc_adaptive_stats_get: no adaptive frame on this device")


def adaptive_phase_ms():
    """Kernel spans of the last timed adaptive frame (rc_adaptive_phase_ms), in ms:
    {"render", "mark", "refine"}."""
    return _phase_ms("rc_adaptive_phase_ms", ("render", "mark", "refine"),
                     "rc_adaptive_phase_ms: no timed adaptive frame on this device")


def rates_compose(base, images, rates):
    """The rate-map contract (include/raycast_hip.h, rc_render_rates) in numpy: `base` where the
    rate is 0 and images[s] where it is s.  base and every image are [H, W, 3] uint8, rates is
    [H, W] uint8 with values in RATE_VALUES; images needs an entry for every non-zero rate that
    occurs."""
    base, rates = np.asarray(base), np.asarray(rates)
    if base.dtype != np.uint8 or base.ndim != 3 or base.shape[2] != 3:
        raise ValueError(f"base: a uint8 [H, W, 3] image, got {base.dtype} {base.shape}")
    if rates.dtype != np.uint8 or rates.shape != base.shape[:2]:
        raise ValueError(f"rates: uint8 {base.shape[:2]}, got {rates.dtype} {rates.shape}")
    out = base.copy()
    for r in np.unique(rates).tolist():
        if r not in RATE_VALUES:
            raise ValueError(f"rate {r} is not one of {RATE_VALUES}")
        if r == 0:
            continue
        if r not in images:
            raise ValueError(f"rate {r} occurs in the map and images has no entry for it")
        img = np.asarray(images[r])
        if img.dtype != np.uint8 or img.shape != base.shape:
            raise ValueError(f"images[{r}]: uint8 {base.shape}, got {img.dtype} {img.shape}")
        sel = rates == r
        out[sel] = img[sel]
    return out


def render_rates(scene, width, height, rates, depth=6, mode="fast", out=None, timing=None):
    """Variable-rate supersampling through rc_render_rates: `rates` is the [H, W] uint8 map with
    values in RATE_VALUES, `out` the caller's C-contiguous [H, W, 3] uint8 pixmap, in and out (the
    default is zeros): a pixel of rate 0 keeps its bytes, one of rate s gets the ssaa = s image's
    pixel (rates_compose).  Fast and cuda mode."""
    rates = np.asarray(rates)
    if rates.dtype != np.uint8 or rates.shape != (height, width):
        raise ValueError(f"rates: uint8 {(height, width)}, got {rates.dtype} {rates.shape}")
    rates = np.ascontiguousarray(rates)
    out = _pixmap(out, width, height, np.zeros)
    opt = options(depth, mode)
    with _timed(timing) as (t, _):
        _call("rc_render_rates", scene.packed(), width, height, ctypes.byref(opt), _host_ptr(rates),
              _host_ptr(out), ctypes.byref(t))
    return out


def render_rates_device(scene, width, height, d_rates_ptr, d_out_ptr, stream_ptr=None, depth=6,
                        mode="fast", timing=None):
    """rc_render_rates_device: the map (W*H bytes) and the image (W*H*3 bytes) are device memory;
    enqueued on the stream and asynchronous unless `timing` is given.  A map byte outside
    RATE_VALUES leaves its pixel alone and is counted in rate_stats()["invalid"]."""
    opt = options(depth, mode)
    with _timed(timing) as (_, t):
        _call("rc_render_rates_device", scene.packed(), width, height, ctypes.byref(opt),
              ctypes.c_void_p(d_rates_ptr), ctypes.c_void_p(d_out_ptr), _stream(stream_ptr), t)


def rate_stats():
    """The last rate-map frame enqueued on the current device (rc_rate_stats_get, which waits for
    it): {"pixels": {1: n, 2: n, 4: n, 8: n}, "invalid": map bytes outside RATE_VALUES, "rays"}."""
    st = RcRateStats()
    if hip_lib().rc_rate_stats_get(ctypes.byref(st)) != 0:
        raise RuntimeError("rc_rate_stats_get: no rate-map frame on this device")
    return {"pixels": {s: int(st.pixels[i]) for i, s in enumerate(RATE_VALUES[1:])},
            "invalid": int(st.invalid), "rays": int(st.rays)}


def rate_phase_ms():
    """Kernel spans of the last rate-map frame (rc_rate_phase_ms), in ms: {"render": the rate-1
    pass with the binning, "refine": the three lists}."""
    return _phase_ms("rc_rate_phase_ms", ("render", "refine"),
                     "rc_rate_phase_ms: no rate-map frame on this device")


def filter_box(s):
    """The box filter's taps at factor s (2, 4 or 8): [1]*s, the plain ssaa = s image."""
    s = int(s)
    if s not in (2, 4, 8):
        raise ValueError(f"filter_box: s = {s} is not 2, 4 or 8")
    return [1] * s


def filter_tent(s):
    """The tent's taps at factor s (2, 4 or 8): [1, 3, .., 2s-1, 2s-1, .., 3, 1], halo s/2, sum
    2*s*s: the tent of radius one output pixel at the subsample centres, times 2."""
    s = int(s)
    if s not in (2, 4, 8):
        raise ValueError(f"filter_tent: s = {s} is not 2, 4 or 8")
    up = list(range(1, 2 * s, 2))
    return up + up[::-1]


def filter_check(taps, s):
    """The rules of a tap vector at factor s (include/raycast_hip.h, rc_filter), stated here so
    that they hold without the library; returns the halo h, raises ValueError naming the rule."""
    s = int(s)
    if s not in (2, 4, 8):
        raise ValueError(f"filter: s = {s} is not 2, 4 or 8")
    taps = [int(k) for k in taps]
    n = len(taps)
    if n > FILTER_MAX_TAPS:
        raise ValueError(f"filter: {n} taps, at most {FILTER_MAX_TAPS}")
    if n < s or (n - s) % 2:
        raise ValueError(f"filter: {n} taps at s = {s}: the count is s + 2h with a halo h >= 0")
    h = (n - s) // 2
    if h > s:
        raise ValueError(f"filter: {n} taps at s = {s}: halo {h} > s (at most {3 * s} taps)")
    if any(k < -32768 or k > 32767 for k in taps):
        raise ValueError("filter: the taps are int16")
    if sum(taps) <= 0:
        raise ValueError(f"filter: the taps sum to {sum(taps)}, the sum must be positive")
    if sum(abs(k) for k in taps) > 2048:
        raise ValueError(f"filter: the taps' absolute values sum to "
                         f"{sum(abs(k) for k in taps)}, at most 2048 (the int32 bound)")
    return h


def filter_accumulate(img, s, taps):
    """The filter contract's accumulators acc[y][x][c] (before rounding and clamping): int64
    [H, W, C] of a uint8 [s*H, s*W, C] image."""
    img = np.asarray(img)
    s = int(s)
    h = filter_check(taps, s)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[0] % s or img.shape[1] % s \
            or img.shape[0] == 0 or img.shape[1] == 0:
        raise ValueError(f"filter_downsample: a uint8 [s*H, s*W, C] image, got {img.dtype} "
                         f"{img.shape} and s = {s}")
    oh, ow = img.shape[0] // s, img.shape[1] // s
    k = np.asarray(taps, dtype=np.int64)
    b = np.pad(img.astype(np.int64), ((h, h), (h, h), (0, 0)), mode="edge")
    rows = sum(k[i] * b[:, i:i + s * ow:s] for i in range(len(k)))       # [s*H + 2h, W, C]
    return sum(k[j] * rows[j:j + s * oh:s] for j in range(len(k)))       # [H, W, C]


def filter_downsample(img, s, taps):
    """The filter contract (include/raycast_hip.h, rc_filter) in numpy: the [H, W, C] uint8 image
    of an [s*H, s*W, C] uint8 image through the integer taps k, applied along x and along y over
    the edge-replicated image: clamp((acc + S*S/2) // (S*S), 0, 255) with S = sum k."""
    acc = filter_accumulate(img, s, taps)
    s2 = int(sum(int(k) for k in taps)) ** 2
    return np.clip((acc + s2 // 2) // s2, 0, 255).astype(np.uint8)


def _rc_filter(taps, s):
    filter_check(taps, s)
    f = RcFilter()
    f.ntaps = len(taps)
    for i, k in enumerate(taps):
        f.taps[i] = int(k)
    return f


def render_filtered(scene, width, height, taps, ssaa, depth=6, mode="parity", device=0,
                    timing=None, out=None):
    """rc_render_filtered: the ssaa*W x ssaa*H image of the mode through the tap vector `taps`
    (filter_downsample), into a host array [H, W, 3] uint8.  ssaa is 2, 4 or 8."""
    f = _rc_filter(taps, ssaa)
    out = _pixmap(out, width, height)
    opt = options(depth, mode, 1, device, ssaa)
    with _timed(timing) as (t, _):
        _call("rc_render_filtered", scene.packed(), width, height, ctypes.byref(opt),
              ctypes.byref(f), _host_ptr(out), ctypes.byref(t))
    return out


def render_filtered_device(scene, width, height, taps, ssaa, d_out_ptr, stream_ptr=None, depth=6,
                           mode="parity", timing=None):
    """rc_render_filtered_device: the image (W*H*3 bytes) is device memory; enqueued on the
    stream and asynchronous unless `timing` is given."""
    f = _rc_filter(taps, ssaa)
    opt = options(depth, mode, ssaa=ssaa)
    with _timed(timing) as (_, t):
        _call("rc_render_filtered_device", scene.packed(), width, height, ctypes.byref(opt),
              ctypes.byref(f), ctypes.c_void_p(d_out_ptr), _stream(stream_ptr), t)


def filter_image_device(d_src_ptr, width, height, s, taps, d_dst_ptr, stream_ptr=None):
    """rc_filter_image_device: the filter pass alone, d_dst (W x H x 3 bytes) <- d_src (s*W x s*H
    x 3 bytes), device memory, on the stream; asynchronous."""
    f = _rc_filter(taps, s)
    _call("rc_filter_image_device", ctypes.c_void_p(d_src_ptr), width, height, int(s),
          ctypes.byref(f), ctypes.c_void_p(d_dst_ptr), _stream(stream_ptr))


def filter_phase_ms():
    """Kernel spans of the last timed two-pass supersampled frame (rc_filter_phase_ms), in ms:
    {"render": the s*W x s*H image, "filter": the filter pass}."""
    return _phase_ms("rc_filter_phase_ms", ("render", "filter"),
                     "rc_filter_phase_ms: no timed two-pass frame on this device")


def filter_from_env(ssaa=1, adaptive=0):
    """raycast()'s reading of RAYCAST_FILTER (rc_filter_env) for a frame with the factor `ssaa`
    and the adaptive threshold `adaptive`: the tent's taps when the frame goes through the
    filtered path, None when it goes through rc_render (the warnings go to stderr)."""
    f = RcFilter()
    opt = options(ssaa=ssaa, adaptive=adaptive)
    if hip_lib().rc_filter_env(ctypes.byref(opt), ctypes.byref(f)) != 1:
        return None
    return [int(f.taps[i]) for i in range(f.ntaps)]


def pattern_check(g, points):
    """The rules of a sample pattern (include/raycast_hip.h, rc_pattern), stated here so that they
    hold without the library; returns the sample count n, raises ValueError naming the rule."""
    g = int(g)
    if g not in (2, 4, 8):
        raise ValueError(f"pattern: grid {g} is not 2, 4 or 8")
    pts = [(int(x), int(y)) for x, y in points]
    n = len(pts)
    if n not in (2, 4, 8, 16):
        raise ValueError(f"pattern: {n} samples, not 2, 4, 8 or 16")
    if n > g * g:
        raise ValueError(f"pattern: {n} samples on a {g} x {g} lattice of {g * g} points")
    for k, (x, y) in enumerate(pts):
        if not (0 <= x < g and 0 <= y < g):
            raise ValueError(f"pattern: sample {k} at ({x}, {y}) is off the {g} x {g} lattice")
        if (x, y) in pts[:k]:
            raise ValueError(f"pattern: sample {k} repeats ({x}, {y})")
    return n


def pattern(p):
    """A checked pattern (g, [(x, y), ...]) from a built-in name (PATTERNS) or a (g, points)
    pair."""
    if isinstance(p, str):
        if p not in PATTERNS:
            raise ValueError(f"pattern: '{p}' is not one of {sorted(PATTERNS)}")
        p = PATTERNS[p]
    g, points = p
    pts = [(int(x), int(y)) for x, y in points]
    pattern_check(g, pts)
    return int(g), pts


def pattern_downsample(big, g, points):
    """The pattern contract (include/raycast_hip.h, rc_pattern) in numpy: the [H, W, C] uint8 image
    of a [g*H, g*W, C] uint8 image, per channel (sum over the n points (x, y) of
    big[g*Y + y, g*X + x] + n/2) // n."""
    big = np.asarray(big)
    g = int(g)
    points = [(int(x), int(y)) for x, y in points]
    n = pattern_check(g, points)
    if big.dtype != np.uint8 or big.ndim != 3 or big.shape[0] % g or big.shape[1] % g:
        raise ValueError(f"pattern_downsample: a uint8 [g*H, g*W, C] image, got {big.dtype} "
                         f"{big.shape} and g = {g}")
    total = sum(big[int(y)::g, int(x)::g].astype(np.uint32) for x, y in points)
    return ((total + n // 2) // n).astype(np.uint8)


def _lattice(struct, checked):
    """The checked (g, points) in an RcPattern or an RcSampleSeq (the same four fields)."""
    g, pts = checked
    lat = struct()
    lat.grid, lat.nsamples = g, len(pts)
    for k, (x, y) in enumerate(pts):
        lat.x[k], lat.y[k] = x, y
    return lat


def _rc_pattern(p):
    return _lattice(RcPattern, pattern(p))


def render_pattern(scene, width, height, pat, threshold=0, depth=6, mode="fast", device=0,
                   timing=None, out=None):
    """rc_render_pattern: every pixel (threshold 0) or the pixels of the one-ray image whose
    3 x 3 contrast reaches `threshold` (adaptive_compose) get the rounded mean of the pattern's
    samples of the g*W x g*H image (pattern_downsample).  `pat` is a built-in name or a
    (g, [(x, y), ...]) pair.  Fast and cuda mode."""
    p = _rc_pattern(pat)
    out = _pixmap(out, width, height)
    opt = options(depth, mode, 1, device)
    with _timed(timing) as (t, _):
        _call("rc_render_pattern", scene.packed(), width, height, ctypes.byref(opt),
              ctypes.byref(p), int(threshold), _host_ptr(out), ctypes.byref(t))
    return out


def render_pattern_device(scene, width, height, pat, d_out_ptr, threshold=0, stream_ptr=None,
                          depth=6, mode="fast", timing=None):
    """rc_render_pattern_device: the image (W*H*3 bytes) is device memory; enqueued on the stream
    and asynchronous unless `timing` is given."""
    p = _rc_pattern(pat)
    opt = options(depth, mode)
    with _timed(timing) as (_, t):
        _call("rc_render_pattern_device", scene.packed(), width, height, ctypes.byref(opt),
              ctypes.byref(p), int(threshold), ctypes.c_void_p(d_out_ptr), _stream(stream_ptr), t)


def pattern_stats():
    """The last pattern frame enqueued on the current device (rc_pattern_stats_get, which waits
    for it): {"refined_pixels", "rays"}; threshold 0: W*H and n*W*H, else the listed pixels and
    W*H + n*listed."""
    return _stats("rc_pattern_stats_get", RcPatternStats,
                  "rc_pattern_stats_get: no pattern frame on this device")


def pattern_phase_ms():
    """Kernel spans of the last pattern frame (rc_pattern_phase_ms), in ms: {"render", "mark",
    "refine"}; threshold 0: "render" is the pattern kernel and the others are 0."""
    return _phase_ms("rc_pattern_phase_ms", ("render", "mark", "refine"),
                     "rc_pattern_phase_ms: no pattern frame on this device")


def pattern_from_env(mode="fast", ssaa=1, adaptive=0):
    """raycast()'s reading of RAYCAST_PATTERN (rc_pattern_env) for a frame of that mode, factor
    and adaptive threshold: (g, [(x, y), ...], t) when the frame goes through the pattern path,
    None when it goes through rc_render (the warnings go to stderr)."""
    p, t = RcPattern(), ctypes.c_int(0)
    opt = options(mode=mode, ssaa=ssaa, adaptive=adaptive)
    if hip_lib().rc_pattern_env(ctypes.byref(opt), ctypes.byref(p), ctypes.byref(t)) != 1:
        return None
    return p.grid, [(int(p.x[k]), int(p.y[k])) for k in range(p.nsamples)], t.value


def sample_seq_check(g, points):
    """The rules of a sample sequence (include/raycast_hip.h, rc_sample_seq), stated here so that
    they hold without the library; returns the length, raises ValueError naming the rule."""
    g = int(g)
    if g not in (2, 4, 8):
        raise ValueError(f"sample sequence: grid {g} is not 2, 4 or 8")
    pts = [(int(x), int(y)) for x, y in points]
    n, most = len(pts), min(ACCUM_MAX_SAMPLES, g * g)
    if not 1 <= n <= most:
        raise ValueError(f"sample sequence: {n} samples, not 1..{most}")
    for k, (x, y) in enumerate(pts):
        if not (0 <= x < g and 0 <= y < g):
            raise ValueError(f"sample sequence: sample {k} at ({x}, {y}) is off the {g} x {g} "
                             "lattice")
        if (x, y) in pts[:k]:
            raise ValueError(f"sample sequence: sample {k} repeats ({x}, {y})")
    return n


def sample_seq(p):
    """A checked sequence (g, [(x, y), ...]) from a built-in name (SAMPLE_SEQS) or a (g, points)
    pair."""
    if isinstance(p, str):
        if p not in SAMPLE_SEQS:
            raise ValueError(f"sample sequence: '{p}' is not one of {sorted(SAMPLE_SEQS)}")
        p = SAMPLE_SEQS[p]
    g, points = p
    pts = [(int(x), int(y)) for x, y in points]
    sample_seq_check(g, pts)
    return int(g), pts


def _accum_state(acc):
    acc = np.asarray(acc)
    if acc.dtype != np.uint16 or acc.ndim != 3 or acc.shape[2] != 4:
        raise ValueError(f"an accumulator is [H, W, 4] uint16 (three sums and n), got {acc.dtype} "
                         f"{acc.shape}")
    return acc


def accum_resolve(acc):
    """The accumulation contract's resolve (include/raycast_hip.h, rc_accum_px) in numpy: the
    [H, W, 3] uint8 image (sum + n/2) // n of an [H, W, 4] uint16 accumulator; (0, 0, 0) where
    n = 0."""
    acc = _accum_state(acc).astype(np.uint32)
    n = acc[:, :, 3:4]
    res = (acc[:, :, :3] + n // 2) // np.maximum(n, 1)
    return np.where(n > 0, res, 0).astype(np.uint8)


def accum_step(acc, out, big, g, points, t=0, reset=False):
    """One pass of the accumulation contract in numpy: the samples `points` (1..16 lattice points,
    the pass's slice of its sequence) of the [g*H, g*W, 3] uint8 image `big` are added to the
    pixels of the active set, every pixel (t = 0, or reset, which also zeroes the accumulator
    first) or edge_mask(out, t); an active pixel whose n would pass 256 is saturated and keeps
    everything.  Returns (acc', out', active, saturated); the arguments are not written."""
    big, g, t = np.asarray(big), int(g), int(t)
    points = [(int(x), int(y)) for x, y in points]
    count = len(points)
    if not 1 <= count <= ACCUM_MAX_COUNT:
        raise ValueError(f"accum_step: {count} samples, a pass takes 1..{ACCUM_MAX_COUNT}")
    if g not in (2, 4, 8) or any(not (0 <= x < g and 0 <= y < g) for x, y in points):
        raise ValueError(f"accum_step: points off the {g} x {g} lattice (g is 2, 4 or 8)")
    if not 0 <= t <= 255 or (reset and t):
        raise ValueError(f"accum_step: threshold {t} (0..255, and 0 with reset)")
    if big.dtype != np.uint8 or big.ndim != 3 or big.shape[0] % g or big.shape[1] % g:
        raise ValueError(f"accum_step: a uint8 [g*H, g*W, C] image, got {big.dtype} {big.shape}")
    acc, out = _accum_state(acc), np.asarray(out)
    h, w = big.shape[0] // g, big.shape[1] // g
    if acc.shape[:2] != (h, w) or out.shape != (h, w, 3) or out.dtype != np.uint8:
        raise ValueError(f"accum_step: acc {acc.shape} and out {out.dtype} {out.shape} do not fit "
                         f"a {w} x {h} image")
    state = np.zeros((h, w, 4), dtype=np.uint32) if reset else acc.astype(np.uint32)
    mask = edge_mask(out, t) if t > 0 else np.ones((h, w), dtype=bool)
    saturated = mask & (state[:, :, 3] + count > ACCUM_MAX_N)
    take = mask & ~saturated
    add = sum(big[y::g, x::g].astype(np.uint32) for x, y in points)
    state[:, :, :3] += add * take[:, :, None]
    state[:, :, 3] += (count * take).astype(np.uint32)
    new_acc = np.where(take[:, :, None], state, acc).astype(np.uint16)
    new_out = np.where(take[:, :, None], accum_resolve(new_acc), out)
    return new_acc, new_out, int(mask.sum()), int(saturated.sum())


def accum_run(big, g, points, dense, t=0):
    """rc_render_accum's contract in numpy: samples [0, dense) of the sequence for every pixel
    (a reset pass in chunks of at most 16), then one single-sample pass with threshold t for each
    of the others.  Returns the [H, W, 3] uint8 image."""
    big, g = np.asarray(big), int(g)
    points = [(int(x), int(y)) for x, y in points]
    n = sample_seq_check(g, points)
    if not 1 <= int(dense) <= n:
        raise ValueError(f"accum_run: dense {dense} is not 1..{n}")
    h, w = big.shape[0] // g, big.shape[1] // g
    acc = np.zeros((h, w, 4), dtype=np.uint16)
    out = np.zeros((h, w, 3), dtype=np.uint8)
    for k in range(0, dense, ACCUM_MAX_COUNT):
        acc, out, _, _ = accum_step(acc, out, big, g, points[k:min(dense, k + ACCUM_MAX_COUNT)], 0,
                                    reset=k == 0)
    for k in range(dense, n):
        acc, out, _, _ = accum_step(acc, out, big, g, points[k:k + 1], t)
    return out


def _rc_sample_seq(p):
    return _lattice(RcSampleSeq, sample_seq(p))


def accum_pass_device(scene, width, height, seq, first, count, d_acc_ptr, d_out_ptr, threshold=0,
                      reset=False, stream_ptr=None, depth=6, mode="fast", timing=None):
    """rc_accum_pass_device: samples [first, first + count) of `seq` (a built-in name or a
    (g, [(x, y), ...]) pair) are added to the accumulator (W*H*8 bytes of device memory, an
    [H, W, 4] uint16 array) and the means stored in the image (W*H*3 bytes), for every pixel
    (threshold 0) or the pixels of the image as it stands whose 3 x 3 contrast reaches
    `threshold` (accum_step).  Enqueued on the stream and asynchronous unless `timing` is given."""
    s = _rc_sample_seq(seq)
    opt = options(depth, mode)
    with _timed(timing) as (_, t):
        _call("rc_accum_pass_device", scene.packed(), width, height, ctypes.byref(opt),
              ctypes.byref(s), int(first), int(count), int(threshold), 1 if reset else 0,
              ctypes.c_void_p(d_acc_ptr), ctypes.c_void_p(d_out_ptr), _stream(stream_ptr), t)


def accum_resolve_device(d_acc_ptr, width, height, d_out_ptr, stream_ptr=None):
    """rc_accum_resolve_device: the image of an accumulator (accum_resolve), nothing shot."""
    _call("rc_accum_resolve_device", ctypes.c_void_p(d_acc_ptr), width, height,
          ctypes.c_void_p(d_out_ptr), _stream(stream_ptr))


def render_accum(scene, width, height, seq, dense=None, threshold=0, depth=6, mode="fast",
                 device=0, timing=None, out=None):
    """rc_render_accum (accum_run): samples [0, dense) of `seq` for every pixel, then one
    single-sample pass with `threshold` for each of the others.  dense = None: the whole sequence.
    Fast and cuda mode."""
    s = _rc_sample_seq(seq)
    out = _pixmap(out, width, height)
    opt = options(depth, mode, 1, device)
    with _timed(timing) as (t, _):
        _call("rc_render_accum", scene.packed(), width, height, ctypes.byref(opt), ctypes.byref(s),
              s.nsamples if dense is None else int(dense), int(threshold), _host_ptr(out),
              ctypes.byref(t))
    return out


def accum_stats():
    """The last accumulation call enqueued on the current device (rc_accum_stats_get, which waits
    for it): {"passes", "active_pixels", "saturated", "rays"}; the pixel counts are the last
    pass's, the rays the whole call's."""
    return _stats("rc_accum_stats_get", RcAccumStats,
                  "rc_accum_stats_get: no accumulation call on this device")


def accum_phase_ms():
    """Kernel spans of the last pass of the last accumulation call (rc_accum_phase_ms), in ms:
    {"mark", "shoot"}; "mark" is 0 for a pass that takes every pixel.  After accum_scroll_device
    "mark" is the move of the kept rectangle and "shoot" all the sample chunks."""
    return _phase_ms("rc_accum_phase_ms", ("mark", "shoot"),
                     "rc_accum_phase_ms: no accumulation call on this device")


def _window(window, width, height, s=1):
    """The checked (full_w, full_h, x0, y0) of a width x height window at factor s (the rules of
    rc_window_check that do not depend on the kernels' grids, stated here so that they hold
    without the library); raises ValueError naming the rule."""
    fw, fh, x0, y0 = (int(v) for v in window)
    w, h, s = int(width), int(height), int(s)
    if s not in (1, 2, 4, 8):
        raise ValueError(f"window: factor {s} is not 1, 2, 4 or 8")
    if fw < 1 or fh < 1 or w < 1 or h < 1:
        raise ValueError(f"window: a {w} x {h} window of a {fw} x {fh} image: sizes below 1")
    if x0 < 0 or y0 < 0:
        raise ValueError(f"window: origin ({x0}, {y0}) is negative")
    if x0 + w > fw or y0 + h > fh:
        raise ValueError(f"window: {w} x {h} at ({x0}, {y0}) reaches outside {fw} x {fh}")
    if s * fw > 2 ** 31 - 1 or s * fh > 2 ** 31 - 1:
        raise ValueError(f"window: {s} times {fw} x {fh} passes 2^31 - 1")
    return fw, fh, x0, y0


def _rc_window(window):
    win = RcWindow()
    win.full_w, win.full_h, win.x0, win.y0 = (int(v) for v in window)
    return win


def window_check(window, width, height, s=1):
    """rc_window_check: True when the library renders that window at factor s (its message goes
    to stderr otherwise)."""
    win = _rc_window(window)
    return hip_lib().rc_window_check(ctypes.byref(win), int(width), int(height), int(s)) == 0


def window_crop(img, s, window, width, height):
    """The window contract (include/raycast_hip.h, rc_window) in numpy: the rows s*y0 ..
    s*(y0 + H) and columns s*x0 .. s*(x0 + W) of an [s*full_h, s*full_w, C] image, so with s = 1
    out[y][x] = img[y0 + y][x0 + x], and with s = g the [g*H, g*W, C] image whose samples an
    accumulation pass through the window takes."""
    img = np.asarray(img)
    fw, fh, x0, y0 = _window(window, width, height, s)
    s = int(s)
    if img.ndim != 3 or img.shape[0] != s * fh or img.shape[1] != s * fw:
        raise ValueError(f"window_crop: an [{s * fh}, {s * fw}, C] image, got {img.shape}")
    return img[s * y0:s * (y0 + int(height)), s * x0:s * (x0 + int(width))]


def window_tiles(full_w, full_h, tw, th):
    """The windows that cover a full_w x full_h image in tiles of tw x th, row by row, the last
    column and row clipped: [((full_w, full_h, x0, y0), W, H), ...]."""
    full_w, full_h, tw, th = int(full_w), int(full_h), int(tw), int(th)
    if full_w < 1 or full_h < 1 or tw < 1 or th < 1:
        raise ValueError(f"window_tiles: {full_w} x {full_h} in tiles of {tw} x {th}")
    return [((full_w, full_h, x0, y0), min(tw, full_w - x0), min(th, full_h - y0))
            for y0 in range(0, full_h, th) for x0 in range(0, full_w, tw)]


def window_for_zoom(width, height, zoom, cx, cy):
    """The W x H window of the zoom*W x zoom*H image (an integer zoom >= 1) centred on pixel
    (cx, cy) of the unzoomed W x H frame, clamped to the frame: the window's pixel (W // 2, H // 2)
    is the virtual pixel (zoom*cx + zoom // 2, zoom*cy + zoom // 2) unless the clamp moved it."""
    w, h, z, cx, cy = int(width), int(height), int(zoom), int(cx), int(cy)
    if w < 1 or h < 1 or z < 1 or not (0 <= cx < w and 0 <= cy < h):
        raise ValueError(f"window_for_zoom: zoom {z} on pixel ({cx}, {cy}) of a {w} x {h} frame")
    x0 = min(max(z * cx + z // 2 - w // 2, 0), z * w - w)
    y0 = min(max(z * cy + z // 2 - h // 2, 0), z * h - h)
    return z * w, z * h, x0, y0


def render_window(scene, window, width, height, ssaa=1, depth=6, mode="fast", device=0,
                  timing=None, out=None):
    """rc_render_window: the W x H window at window = (full_w, full_h, x0, y0) of the full_w x
    full_h image of that mode with that ssaa (window_crop of it, s = 1).  Fast and cuda mode."""
    win = _rc_window(window)
    out = _pixmap(out, width, height)
    opt = options(depth, mode, 1, device, ssaa)
    with _timed(timing) as (t, _):
        _call("rc_render_window", scene.packed(), ctypes.byref(win), width, height,
              ctypes.byref(opt), _host_ptr(out), ctypes.byref(t))
    return out


def render_window_device(scene, window, width, height, d_out_ptr, ssaa=1, stream_ptr=None,
                         depth=6, mode="fast", timing=None):
    """rc_render_window_device: the window's image (W*H*3 bytes) is device memory; enqueued on the
    stream and asynchronous unless `timing` is given."""
    win = _rc_window(window)
    opt = options(depth, mode, ssaa=ssaa)
    with _timed(timing) as (_, t):
        _call("rc_render_window_device", scene.packed(), ctypes.byref(win), width, height,
              ctypes.byref(opt), ctypes.c_void_p(d_out_ptr), _stream(stream_ptr), t)


def accum_pass_window_device(scene, window, width, height, seq, first, count, d_acc_ptr,
                             d_out_ptr, threshold=0, reset=False, stream_ptr=None, depth=6,
                             mode="fast", timing=None):
    """rc_accum_pass_window_device: accum_pass_device with the samples of the window at window =
    (full_w, full_h, x0, y0) of the virtual image (accum_step on window_crop of its g*full_w x
    g*full_h image, s = g); the accumulator and the image are the window's own W x H."""
    win = _rc_window(window)
    s = _rc_sample_seq(seq)
    opt = options(depth, mode)
    with _timed(timing) as (_, t):
        _call("rc_accum_pass_window_device", scene.packed(), ctypes.byref(win), width, height,
              ctypes.byref(opt), ctypes.byref(s), int(first), int(count), int(threshold),
              1 if reset else 0, ctypes.c_void_p(d_acc_ptr), ctypes.c_void_p(d_out_ptr),
              _stream(stream_ptr), t)


def window_pan(window, dx, dy):
    """The window (full_w, full_h, x0, y0) moved by (dx, dy) whole pixels of the virtual image:
    rc_accum_scroll_device's new window for that pan."""
    fw, fh, x0, y0 = (int(v) for v in window)
    return fw, fh, x0 + int(dx), y0 + int(dy)


def scroll_kept(width, height, dx, dy):
    """The kept rectangle of a scroll by (dx, dy) in destination coordinates, (kx, ky, kw, kh);
    kw = kh = 0 when nothing is kept.  The exposed pixels are the other W*H - kw*kh."""
    w, h, dx, dy = int(width), int(height), int(dx), int(dy)
    if abs(dx) >= w or abs(dy) >= h:
        return 0, 0, 0, 0
    return max(0, -dx), max(0, -dy), w - abs(dx), h - abs(dy)


def accum_scroll(acc, out, big, g, points, dx, dy):
    """rc_accum_scroll_device's contract in numpy: the state (acc, out) moved by (-dx, -dy) where
    source and destination overlap, and a reset pass plus t = 0 passes over `points` (1..64, in
    chunks of 16: accum_step) everywhere else, on `big`, the NEW window's [g*H, g*W, 3] samples
    (window_crop).  Returns (acc', out', exposed pixels); the arguments are not written."""
    acc, out = _accum_state(acc), np.asarray(out)
    h, w = acc.shape[:2]
    if out.shape != (h, w, 3) or out.dtype != np.uint8:
        raise ValueError(f"accum_scroll: acc {acc.shape} and out {out.dtype} {out.shape} do not "
                         "fit one image")
    points = [(int(x), int(y)) for x, y in points]
    if not 1 <= len(points) <= ACCUM_MAX_SAMPLES:
        raise ValueError(f"accum_scroll: {len(points)} samples, not 1..{ACCUM_MAX_SAMPLES}")
    new_acc, new_out = np.zeros_like(acc), np.zeros_like(out)
    for k in range(0, len(points), ACCUM_MAX_COUNT):
        new_acc, new_out, _, _ = accum_step(new_acc, new_out, big, g,
                                            points[k:k + ACCUM_MAX_COUNT], 0, reset=k == 0)
    kx, ky, kw, kh = scroll_kept(w, h, dx, dy)
    if kw:
        sx, sy = kx + int(dx), ky + int(dy)
        new_acc[ky:ky + kh, kx:kx + kw] = acc[sy:sy + kh, sx:sx + kw]
        new_out[ky:ky + kh, kx:kx + kw] = out[sy:sy + kh, sx:sx + kw]
    return new_acc, new_out, w * h - kw * kh


def accum_scroll_device(scene, window, width, height, seq, count, dx, dy, d_acc_src_ptr,
                        d_out_src_ptr, d_acc_dst_ptr, d_out_dst_ptr, stream_ptr=None, depth=6,
                        mode="fast", timing=None):
    """rc_accum_scroll_device (accum_scroll): `window` is the NEW window, (dx, dy) its origin minus
    the old one.  The destination state gets the source's records and bytes where the two windows
    overlap and seq[0..count) freshly accumulated where the pan exposed new pixels; the two states
    are separate device buffers of the same W x H.  Enqueued on the stream and asynchronous unless
    `timing` is given."""
    win = _rc_window(window)
    s = _rc_sample_seq(seq)
    opt = options(depth, mode)
    with _timed(timing) as (_, t):
        _call("rc_accum_scroll_device", scene.packed(), ctypes.byref(win), width, height,
              ctypes.byref(opt), ctypes.byref(s), int(count), int(dx), int(dy),
              ctypes.c_void_p(d_acc_src_ptr), ctypes.c_void_p(d_out_src_ptr),
              ctypes.c_void_p(d_acc_dst_ptr), ctypes.c_void_p(d_out_dst_ptr),
              _stream(stream_ptr), t)


def _plane_names(planes):
    """The requested planes as a tuple of GBUFFER_PLANES' names, in that order, at least one."""
    names = (planes,) if isinstance(planes, str) else tuple(planes)
    for p in names:
        if p not in GBUFFER_PLANES:
            raise ValueError(f"gbuffer: plane {p!r} is not one of {tuple(GBUFFER_PLANES)}")
    if not names:
        raise ValueError("gbuffer: no plane asked for")
    return tuple(p for p in GBUFFER_PLANES if p in names)


def id_edge_rates(ids, s, base=1):
    """The geometric edge criterion (include/raycast_hip.h, rc_id_edge_rates_device) in numpy: the
    [H, W] uint8 rate map that is s where a pixel of the 3 x 3 neighbourhood, clipped to the image,
    has another id than the pixel itself, and base elsewhere; s in 2, 4, 8 and base in 0, 1."""
    ids = np.asarray(ids)
    if ids.dtype != np.int32 or ids.ndim != 2 or ids.size == 0:
        raise ValueError(f"id_edge_rates: a non-empty int32 [H, W] plane, got {ids.dtype} {ids.shape}")
    if int(s) not in (2, 4, 8) or int(base) not in (0, 1):
        raise ValueError(f"id_edge_rates: s {s} is not 2, 4 or 8 or base {base} is not 0 or 1")
    h, w = ids.shape
    pad = np.pad(ids, 1, mode="edge")      # a clipped neighbour is one of the pixel's own 3 x 3
    edge = np.zeros((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            edge |= pad[dy:dy + h, dx:dx + w] != ids
    return np.where(edge, np.uint8(s), np.uint8(base)).astype(np.uint8)


def render_gbuffer(scene, width, height, planes=("id", "t"), window=None, mode="fast", device=0,
                   timing=None):
    """rc_render_gbuffer: the primary hit of every pixel of the width x height window at window =
    (full_w, full_h, x0, y0) (None: the whole image) as a dict of numpy arrays, one per requested
    plane: "id" [H, W] int32 (the shape's index in the scene, -1: no hit), "t" [H, W] float32,
    "P" and "N" [H, W, 3] float32 (zeros on a miss; fast and parity mode only)."""
    names = _plane_names(planes)
    out = {p: np.empty((height, width) + ((3,) if GBUFFER_PLANES[p][1] == 3 else ()),
                       dtype=GBUFFER_PLANES[p][0]) for p in names}
    g = RcGbuffer(**{p: a.ctypes.data for p, a in out.items()})
    win = None if window is None else ctypes.byref(_rc_window(window))
    opt = options(0, mode, 1, device)
    with _timed(timing) as (t, _):
        _call("rc_render_gbuffer", scene.packed(), win, width, height, ctypes.byref(opt),
              ctypes.byref(g), ctypes.byref(t))
    return out


def render_gbuffer_device(scene, width, height, window=None, d_id_ptr=None, d_t_ptr=None,
                          d_p_ptr=None, d_n_ptr=None, stream_ptr=None, mode="fast", timing=None):
    """rc_render_gbuffer_device: the planes are device memory (W*H int32, W*H float32, W*H*3
    float32 twice), None for a plane that is not wanted; enqueued on the stream and asynchronous
    unless `timing` is given."""
    g = RcGbuffer(d_id_ptr or None, d_t_ptr or None, d_p_ptr or None, d_n_ptr or None)
    win = None if window is None else ctypes.byref(_rc_window(window))
    opt = options(0, mode)
    with _timed(timing) as (_, t):
        _call("rc_render_gbuffer_device", scene.packed(), win, width, height, ctypes.byref(opt),
              ctypes.byref(g), _stream(stream_ptr), t)


def render_camera_gbuffer(scene, eye, m, width, height, planes=("id", "t"), window=None,
                          mode="fast", device=0, timing=None):
    """rc_render_camera_gbuffer: render_gbuffer through the camera (eye, m): the primary hit of
    render_camera's rays at ssaa = 1, the general scan from the eye, as a dict of numpy arrays, one
    per requested plane.  Fast mode only."""
    names = _plane_names(planes)
    out = {p: np.empty((height, width) + ((3,) if GBUFFER_PLANES[p][1] == 3 else ()),
                       dtype=GBUFFER_PLANES[p][0]) for p in names}
    g = RcGbuffer(**{p: a.ctypes.data for p, a in out.items()})
    cam = _rc_camera(eye, m)
    win = None if window is None else ctypes.byref(_rc_window(window))
    opt = options(0, mode, 1, device)
    with _timed(timing) as (t, _):
        _call("rc_render_camera_gbuffer", scene.packed(), ctypes.byref(cam), win, width, height,
              ctypes.byref(opt), ctypes.byref(g), ctypes.byref(t))
    return out


def render_camera_gbuffer_device(scene, eye, m, width, height, window=None, d_id_ptr=None,
                                 d_t_ptr=None, d_p_ptr=None, d_n_ptr=None, stream_ptr=None,
                                 mode="fast", timing=None):
    """rc_render_camera_gbuffer_device: the planes are device memory (W*H int32, W*H float32,
    W*H*3 float32 twice), None for a plane that is not wanted; enqueued on the stream and
    asynchronous unless `timing` is given."""
    g = RcGbuffer(d_id_ptr or None, d_t_ptr or None, d_p_ptr or None, d_n_ptr or None)
    cam = _rc_camera(eye, m)
    win = None if window is None else ctypes.byref(_rc_window(window))
    opt = options(0, mode)
    with _timed(timing) as (_, t):
        _call("rc_render_camera_gbuffer_device", scene.packed(), ctypes.byref(cam), win, width,
              height, ctypes.byref(opt), ctypes.byref(g), _stream(stream_ptr), t)


def _pick_points(xy):
    xy = np.asarray(xy)
    if xy.ndim != 2 or xy.shape[1] != 2 or xy.dtype.kind not in "iu":
        raise ValueError(f"pick: xy is an integer [n, 2] array of (x, y) pairs, got {xy.dtype} "
                         f"{xy.shape}")
    if not 1 <= len(xy) <= PICK_MAX_POINTS:
        raise ValueError(f"pick: {len(xy)} points, not 1 .. {PICK_MAX_POINTS}")
    if xy.size and (xy.min() < -2 ** 31 or xy.max() > 2 ** 31 - 1):
        raise ValueError("pick: a coordinate outside int32")
    return np.ascontiguousarray(xy, dtype=np.int32)


def pick(scene, full_w, full_h, xy, frame=False, mode="fast", device=0):
    """rc_pick: what is under the pixels xy ([n, 2] integers, (x, y) pairs) of the full_w x full_h
    image, as a structured array of HIT_DTYPE ("id", "t", "P", "N"; frame: P and N too, zeros
    without).  A point outside the image is refused."""
    pts = _pick_points(xy)
    hits = np.zeros(len(pts), dtype=HIT_DTYPE)
    opt = options(0, mode, 1, device)
    _call("rc_pick", scene.packed(), int(full_w), int(full_h), ctypes.byref(opt), int(bool(frame)),
          len(pts), _host_ptr(pts), _host_ptr(hits))
    return hits


def pick_device(scene, full_w, full_h, n, d_xy_ptr, d_hits_ptr, frame=False, stream_ptr=None,
                mode="fast"):
    """rc_pick_device: n (x, y) int32 pairs and n 32-byte records (HIT_DTYPE, 16-byte aligned) in
    device memory, enqueued on the stream; a point outside the image gets id = -2 and zeros."""
    opt = options(0, mode)
    _call("rc_pick_device", scene.packed(), int(full_w), int(full_h), ctypes.byref(opt),
          int(bool(frame)), int(n), ctypes.c_void_p(d_xy_ptr), ctypes.c_void_p(d_hits_ptr),
          _stream(stream_ptr))


def id_edge_rates_device(d_id_ptr, width, height, s, d_rates_ptr, base=1, stream_ptr=None):
    """rc_id_edge_rates_device (id_edge_rates): the map of a device id plane (W*H int32) into
    W*H bytes of device memory, the map render_rates_device takes; one kernel on the stream."""
    _call("rc_id_edge_rates_device", ctypes.c_void_p(d_id_ptr), int(width), int(height), int(s),
          int(base), ctypes.c_void_p(d_rates_ptr), _stream(stream_ptr))


def gbuffer_phase_ms():
    """The kernel span of the last G-buffer or pick frame (rc_gbuffer_phase_ms), in ms."""
    return _phase_ms("rc_gbuffer_phase_ms", ("kernel",),
                     "rc_gbuffer_phase_ms: no G-buffer frame on this device")


def view_identity():
    """The view that changes nothing: rc_render_view with it is rc_render_window, byte for byte."""
    return np.eye(3, dtype=np.float32)


def view_euler(yaw, pitch, roll=0.0):
    """Ry(yaw) . Rx(pitch) . Rz(roll), radians, right-handed rotations about +y, +x and +z, computed
    in double and rounded to float: the camera looks down -z, so a positive yaw turns it to the left
    ("look right 30 degrees" is yaw = -pi / 6), a positive pitch up, and a positive roll rolls it
    counter-clockwise.  A convenience: the contract takes the nine floats as given, the
    trigonometry is not part of it."""
    cy, sy = np.cos(np.float64(yaw)), np.sin(np.float64(yaw))
    cx, sx = np.cos(np.float64(pitch)), np.sin(np.float64(pitch))
    cz, sz = np.cos(np.float64(roll)), np.sin(np.float64(roll))
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], np.float64)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], np.float64)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], np.float64)
    return ((ry @ rx @ rz) + 0.0).astype(np.float32)     # + 0.0: no -0 entries


def _view_matrix(m):
    m = np.asarray(m)
    if m.size != 9:
        raise ValueError(f"view: a 3 x 3 matrix (or nine floats, row-major), got shape {m.shape}")
    return np.ascontiguousarray(m, dtype=np.float32).reshape(3, 3)


def _rc_view(m):
    return RcView((ctypes.c_float * 9)(*_view_matrix(m).ravel().tolist()))


def view_check(m):
    """rc_view_check: True when the library takes that matrix (every entry finite; its message
    goes to stderr otherwise)."""
    return hip_lib().rc_view_check(ctypes.byref(_rc_view(m))) == 0


def view_dirs(camera_w, camera_h, full, xy, m, cuda=False):
    """The view contract (include/raycast_hip.h, rc_view) in numpy, operation for operation: the
    [n, 3] float32 directions of the virtual pixels xy ([n, 2] integers, (X, Y) pairs) of the full
    = (full_w, full_h) image of a camera_w x camera_h view plane under the matrix m.  With ssaa = s
    pass the subsamples' coordinates and full = (s * full_w, s * full_h).  p = (px, py, -1) is the
    reference's unnormalised primary vector, q = m p in float with every operation rounded once,
    and the direction is the mode's normalize of q: the C port's (a double sum of squares, a zero
    length leaves q as it is) or with cuda the CUDA port's (a float sum, no guard)."""
    f32, f64 = np.float32, np.float64
    m = _view_matrix(m)
    xy = np.asarray(xy)
    if xy.ndim != 2 or xy.shape[1] != 2 or xy.dtype.kind not in "iu":
        raise ValueError(f"view_dirs: xy is an integer [n, 2] array of (X, Y) pairs, got {xy.dtype} "
                         f"{xy.shape}")
    fw, fh = (int(v) for v in full)
    cw, ch = f32(camera_w), f32(camera_h)
    pw, ph = cw / f32(fw), ch / f32(fh)
    px = ((0.0 - f64(cw) / 2.0) + f64(pw) * (xy[:, 0].astype(f64) + 0.5)).astype(f32)
    py = ((0.0 + f64(ch) / 2.0) - f64(ph) * (xy[:, 1].astype(f64) + 0.5)).astype(f32)
    pz = np.full(len(px), -1.0, f32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        q = np.stack([(m[i, 0] * px + m[i, 1] * py) + m[i, 2] * pz for i in range(3)], 1)
        assert q.dtype == f32
        if cuda:
            s = q[:, 0] * q[:, 0]
            s = s + q[:, 1] * q[:, 1]
            s = s + q[:, 2] * q[:, 2]
            ln = np.sqrt(s.astype(f64)).astype(f32)
            return (q / ln[:, None]).astype(f32)
        d = q.astype(f64)
        s = d[:, 0] * d[:, 0]
        s = s + d[:, 1] * d[:, 1]
        s = s + d[:, 2] * d[:, 2]
        ln = np.sqrt(s).astype(f32)
        zero = ln == 0.0
        out = (q / np.where(zero, f32(1.0), ln)[:, None]).astype(f32)
        out[zero] = q[zero]
        return out


def view_grid(width, height, x0=0, y0=0):
    """The (X, Y) pairs of a width x height block of pixels at (x0, y0), row-major: view_dirs' xy
    for a whole image or a window."""
    ys, xs = np.mgrid[y0:y0 + height, x0:x0 + width]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int64)


def render_view(scene, m, width, height, window=None, ssaa=1, depth=6, mode="fast", device=0,
                timing=None, out=None):
    """rc_render_view: the width x height image (or, with window = (full_w, full_h, x0, y0), that
    window of the virtual image) of the camera turned by the view matrix m: pixel colours are the
    bounce loop along view_dirs' directions, box-filtered at ssaa.  Fast and cuda mode."""
    view = _rc_view(m)
    win = None if window is None else ctypes.byref(_rc_window(window))
    out = _pixmap(out, width, height)
    opt = options(depth, mode, 1, device, ssaa)
    with _timed(timing) as (t, _):
        _call("rc_render_view", scene.packed(), ctypes.byref(view), win, width, height,
              ctypes.byref(opt), _host_ptr(out), ctypes.byref(t))
    return out


def render_view_device(scene, m, width, height, d_out_ptr, window=None, ssaa=1, stream_ptr=None,
                       depth=6, mode="fast", timing=None):
    """rc_render_view_device: the image (W*H*3 bytes) is device memory; enqueued on the stream and
    asynchronous unless `timing` is given."""
    view = _rc_view(m)
    win = None if window is None else ctypes.byref(_rc_window(window))
    opt = options(depth, mode, ssaa=ssaa)
    with _timed(timing) as (_, t):
        _call("rc_render_view_device", scene.packed(), ctypes.byref(view), win, width, height,
              ctypes.byref(opt), ctypes.c_void_p(d_out_ptr), _stream(stream_ptr), t)


def _ray_dirs(dirs):
    dirs = np.asarray(dirs)
    if dirs.ndim != 2 or dirs.shape[1] != 3:
        raise ValueError(f"trace_rays: dirs is an [n, 3] array of directions, got {dirs.shape}")
    if not 1 <= len(dirs) <= RAYS_MAX:
        raise ValueError(f"trace_rays: {len(dirs)} rays, not 1 .. {RAYS_MAX}")
    return np.ascontiguousarray(dirs, dtype=np.float32)


def trace_rays(scene, dirs, outputs=("rgb8",), frame=False, depth=6, mode="fast", device=0):
    """rc_trace_rays: the rays from the origin along dirs ([n, 3] float32, used as given: not
    normalised), as a dict of numpy arrays, one per requested output: "rgb" [n, 3] float32 (the
    colour before quantisation), "rgb8" [n, 3] uint8 (its bytes) and "hits" [n] HIT_DTYPE (the
    primary hit; frame: P and N too, fast mode only).  Any projection is its directions; picking
    in a turned view is trace_rays(view_dirs(cursor pixel), ("hits",))."""
    d = _ray_dirs(dirs)
    names = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    for p in names:
        if p not in RAY_OUTPUTS:
            raise ValueError(f"trace_rays: output {p!r} is not one of {tuple(RAY_OUTPUTS)}")
    out = {p: np.zeros((len(d),) + RAY_OUTPUTS[p][1], dtype=RAY_OUTPUTS[p][0])
           for p in RAY_OUTPUTS if p in names}
    ro = RcRayOut(frame=int(bool(frame)), **{p: a.ctypes.data for p, a in out.items()})
    opt = options(depth, mode, 1, device)
    _call("rc_trace_rays", scene.packed(), ctypes.byref(opt), len(d), _host_ptr(d),
          ctypes.byref(ro))
    return out


def trace_rays_device(scene, n, d_dirs_ptr, d_rgb8_ptr=None, d_rgb_ptr=None, d_hits_ptr=None,
                      frame=False, stream_ptr=None, depth=6, mode="fast"):
    """rc_trace_rays_device: n directions (n x 3 float32) and the outputs (n x 3 bytes, n x 3
    float32, n 32-byte HIT_DTYPE records 16-byte aligned; None: not wanted) in device memory,
    enqueued on the stream."""
    ro = RcRayOut(d_rgb8_ptr or None, d_rgb_ptr or None, d_hits_ptr or None, int(bool(frame)))
    opt = options(depth, mode)
    _call("rc_trace_rays_device", scene.packed(), ctypes.byref(opt), int(n),
          ctypes.c_void_p(d_dirs_ptr), ctypes.byref(ro), _stream(stream_ptr))


def view_phase_ms():
    """The kernel span of the last view, camera or ray frame (rc_view_phase_ms), in ms: the camera
    entries and the rays with origins record the view family's spans."""
    return _phase_ms("rc_view_phase_ms", ("kernel",),
                     "rc_view_phase_ms: no view or ray frame on this device")


def camera(eye, m=None):
    """(eye, m): the three eye floats and the nine matrix floats (3 x 3, row-major) of an rc_camera
    as float32 arrays, used as given; m = None is the identity.  The directions of the camera are
    view_dirs(..., m), unchanged by the eye, and every ray's origin is eye."""
    e = np.asarray(eye)
    if e.size != 3:
        raise ValueError(f"camera: eye is three floats, got shape {e.shape}")
    return (np.ascontiguousarray(e, dtype=np.float32).reshape(3),
            view_identity() if m is None else _view_matrix(m))


def _rc_camera(eye, m):
    e, m = camera(eye, m)
    return RcCamera((ctypes.c_float * 3)(*e.tolist()), RcView((ctypes.c_float * 9)(*m.ravel().tolist())))


def camera_check(eye, m=None):
    """rc_camera_check: True when the library takes that camera (every eye component and matrix
    entry finite; its message goes to stderr otherwise)."""
    return hip_lib().rc_camera_check(ctypes.byref(_rc_camera(eye, m))) == 0


def render_camera(scene, eye, m, width, height, window=None, ssaa=1, depth=6, device=0,
                  mode="fast", timing=None, out=None):
    """rc_render_camera: render_view with the eye moved to `eye`: the width x height image (or that
    window of the virtual image) whose pixel colours are the fast-mode bounce loop from eye along
    view_dirs' directions (m = None: the identity), box-filtered at ssaa.  Fast mode only."""
    cam = _rc_camera(eye, m)
    win = None if window is None else ctypes.byref(_rc_window(window))
    out = _pixmap(out, width, height)
    opt = options(depth, mode, 1, device, ssaa)
    with _timed(timing) as (t, _):
        _call("rc_render_camera", scene.packed(), ctypes.byref(cam), win, width, height,
              ctypes.byref(opt), _host_ptr(out), ctypes.byref(t))
    return out


def render_camera_device(scene, eye, m, width, height, d_out_ptr, window=None, ssaa=1,
                         stream_ptr=None, depth=6, mode="fast", timing=None):
    """rc_render_camera_device: the image (W*H*3 bytes) is device memory; enqueued on the stream
    and asynchronous unless `timing` is given."""
    cam = _rc_camera(eye, m)
    win = None if window is None else ctypes.byref(_rc_window(window))
    opt = options(depth, mode, ssaa=ssaa)
    with _timed(timing) as (_, t):
        _call("rc_render_camera_device", scene.packed(), ctypes.byref(cam), win, width, height,
              ctypes.byref(opt), ctypes.c_void_p(d_out_ptr), _stream(stream_ptr), t)


def accum_add(acc, out, planes, t=0, reset=False):
    """One accumulation pass in numpy for per-sample planes: planes[j] is the [H, W, 3] uint8 image
    sample j of the pass is taken from (for a pass through cameras, the lattice point's slice of
    camera j's g*H x g*W image), count = len(planes) in 1..16.  The contract is accum_step's: the
    active set is every pixel (t = 0, or reset, which also zeroes the accumulator first) or
    edge_mask(out, t); an active pixel whose n would pass 256 is saturated and keeps everything.
    Returns (acc', out', active, saturated); the arguments are not written.
    accum_step(acc, out, big, g, points, ...) is accum_add on the planes big[y::g, x::g]."""
    planes, t = np.asarray(planes), int(t)
    if planes.dtype != np.uint8 or planes.ndim != 4 or planes.shape[3] != 3:
        raise ValueError(f"accum_add: planes are [count, H, W, 3] uint8, got {planes.dtype} "
                         f"{planes.shape}")
    count, h, w = planes.shape[:3]
    if not 1 <= count <= ACCUM_MAX_COUNT:
        raise ValueError(f"accum_add: {count} samples, a pass takes 1..{ACCUM_MAX_COUNT}")
    if not 0 <= t <= 255 or (reset and t):
        raise ValueError(f"accum_add: threshold {t} (0..255, and 0 with reset)")
    acc, out = _accum_state(acc), np.asarray(out)
    if acc.shape[:2] != (h, w) or out.shape != (h, w, 3) or out.dtype != np.uint8:
        raise ValueError(f"accum_add: acc {acc.shape} and out {out.dtype} {out.shape} do not fit "
                         f"a {w} x {h} image")
    state = np.zeros((h, w, 4), dtype=np.uint32) if reset else acc.astype(np.uint32)
    mask = edge_mask(out, t) if t > 0 else np.ones((h, w), dtype=bool)
    saturated = mask & (state[:, :, 3] + count > ACCUM_MAX_N)
    take = mask & ~saturated
    state[:, :, :3] += planes.astype(np.uint32).sum(axis=0) * take[:, :, None]
    state[:, :, 3] += (count * take).astype(np.uint32)
    new_acc = np.where(take[:, :, None], state, acc).astype(np.uint16)
    new_out = np.where(take[:, :, None], accum_resolve(new_acc), out)
    return new_acc, new_out, int(mask.sum()), int(saturated.sum())


def thin_lens(eye, m, focus, lens_points):
    """The cameras of a thin lens around the pinhole camera (eye, m): one (eye, m) pair for each
    lens point (lx, ly), in camera units on the plane z = 0 of the camera's frame.  With M the
    view matrix and f = focus > 0 the distance of the focal plane, the eye is eye + M (lx, ly, 0)
    and the view M [[1, 0, lx/f], [0, 1, ly/f], [0, 0, 1]]: the primary vector's z is -1, so the
    ray's vector is proportional to f M p - M (lx, ly, 0) and the ray through any lens point passes
    through the pinhole ray's point on the plane at depth f.  Computed in float64 and rounded once
    to float32; lens point (0, 0) is the camera as given, bit for bit.  The helper only makes
    cameras: the device contract is exact for whatever cameras it is given."""
    e, m = camera(eye, m)
    f = float(focus)
    if not (f > 0.0 and np.isfinite(f)):
        raise ValueError(f"thin_lens: focus {focus} is not a finite distance above 0")
    pts = np.asarray(lens_points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 2 or not len(pts):
        raise ValueError(f"thin_lens: lens points are [n, 2], got shape {pts.shape}")
    e64, m64 = e.astype(np.float64), m.astype(np.float64)
    cams = []
    for lx, ly in pts:
        if lx == 0.0 and ly == 0.0:
            cams.append((e.copy(), m.copy()))
            continue
        shear = np.array([[1.0, 0.0, lx / f], [0.0, 1.0, ly / f], [0.0, 0.0, 1.0]])
        cams.append(((e64 + m64 @ np.array([lx, ly, 0.0])).astype(np.float32),
                     (m64 @ shear).astype(np.float32)))
    return cams


def _rc_cameras(cams, per, what):
    """The RcCamera array of `cams`: one (eye, m) pair, or a sequence of `per` of them."""
    try:
        single = len(cams) == 2 and np.ndim(cams[0][0]) == 0
    except (TypeError, IndexError):
        raise ValueError(f"{what}: cams is one (eye, m) pair or a list of them") from None
    pairs = [cams] if single else list(cams)
    if len(pairs) not in (1, int(per)):
        raise ValueError(f"{what}: {len(pairs)} cameras, it takes 1 or {int(per)}")
    arr = (RcCamera * len(pairs))()
    for k, pair in enumerate(pairs):
        if len(pair) != 2:
            raise ValueError(f"{what}: camera {k} is not an (eye, m) pair")
        arr[k] = _rc_camera(pair[0], pair[1])
    return arr


def accum_pass_camera_device(scene, cams, window, width, height, seq, first, count, d_acc_ptr,
                             d_out_ptr, threshold=0, reset=False, stream_ptr=None, depth=6,
                             mode="fast", timing=None):
    """rc_accum_pass_camera_device: accum_pass_window_device with the samples taken through
    cameras: `cams` is one (eye, m) pair for the whole pass or a list of `count` of them, sample
    first + j through camera j (accum_add on the lattice points' slices of the cameras' g*full_w x
    g*full_h images).  window = None: the whole width x height image.  Fast mode only."""
    arr = _rc_cameras(cams, count, "accum_pass_camera_device")
    win = None if window is None else ctypes.byref(_rc_window(window))
    s = _rc_sample_seq(seq)
    opt = options(depth, mode)
    with _timed(timing) as (_, t):
        _call("rc_accum_pass_camera_device", scene.packed(), arr, len(arr), win, width, height,
              ctypes.byref(opt), ctypes.byref(s), int(first), int(count), int(threshold),
              1 if reset else 0, ctypes.c_void_p(d_acc_ptr), ctypes.c_void_p(d_out_ptr),
              _stream(stream_ptr), t)


def render_camera_accum(scene, cams, width, height, seq, window=None, depth=6, device=0,
                        mode="fast", timing=None, out=None):
    """rc_render_camera_accum: the whole of `seq` for every pixel through `cams`, one (eye, m) pair
    or a list of one for each sample of the sequence; the mean image.  With hier<g> and one camera
    that is render_camera's image at ssaa = g.  Fast mode only."""
    s = _rc_sample_seq(seq)
    arr = _rc_cameras(cams, s.nsamples, "render_camera_accum")
    win = None if window is None else ctypes.byref(_rc_window(window))
    out = _pixmap(out, width, height)
    opt = options(depth, mode, 1, device)
    with _timed(timing) as (t, _):
        _call("rc_render_camera_accum", scene.packed(), arr, len(arr), win, width, height,
              ctypes.byref(opt), ctypes.byref(s), _host_ptr(out), ctypes.byref(t))
    return out


def trace_rays_from(scene, origins, dirs, outputs=("rgb8",), frame=False, depth=6, mode="fast",
                    device=0):
    """rc_trace_rays_from: trace_rays with ray k leaving origins[k] ([n, 3] float32, used as given
    and not checked: a non-finite origin is a miss, as in the oracle): the rays an occlusion or a
    gather pass shoots from the hit points of a G-buffer.  Fast mode only."""
    d = _ray_dirs(dirs)
    o = np.asarray(origins)
    if o.shape != d.shape:
        raise ValueError(f"trace_rays_from: origins is an [n, 3] array like dirs {d.shape}, got "
                         f"{o.shape}")
    o = np.ascontiguousarray(o, dtype=np.float32)
    names = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    for p in names:
        if p not in RAY_OUTPUTS:
            raise ValueError(f"trace_rays_from: output {p!r} is not one of {tuple(RAY_OUTPUTS)}")
    out = {p: np.zeros((len(d),) + RAY_OUTPUTS[p][1], dtype=RAY_OUTPUTS[p][0])
           for p in RAY_OUTPUTS if p in names}
    ro = RcRayOut(frame=int(bool(frame)), **{p: a.ctypes.data for p, a in out.items()})
    opt = options(depth, mode, 1, device)
    _call("rc_trace_rays_from", scene.packed(), ctypes.byref(opt), len(d), _host_ptr(o),
          _host_ptr(d), ctypes.byref(ro))
    return out


def trace_rays_from_device(scene, n, d_origins_ptr, d_dirs_ptr, d_rgb8_ptr=None, d_rgb_ptr=None,
                           d_hits_ptr=None, frame=False, stream_ptr=None, depth=6, mode="fast"):
    """rc_trace_rays_from_device: n origins and n directions (n x 3 float32 each) and the outputs
    (as trace_rays_device's; None: not wanted) in device memory, enqueued on the stream."""
    ro = RcRayOut(d_rgb8_ptr or None, d_rgb_ptr or None, d_hits_ptr or None, int(bool(frame)))
    opt = options(depth, mode)
    _call("rc_trace_rays_from_device", scene.packed(), ctypes.byref(opt), int(n),
          ctypes.c_void_p(d_origins_ptr), ctypes.c_void_p(d_dirs_ptr), ctypes.byref(ro),
          _stream(stream_ptr))


def ao_dirs(n, tmax=np.inf, rot=None):
    """A direction set (u [n, 3] float32, tmax) for the occlusion pass: the spiral points of the
    unit sphere, z_i = 1 - 2 (i + 1/2) / n, r_i = sqrt(1 - z_i^2), phi_i = (i + 1/2) pi (3 -
    sqrt 5), u_i = (r_i cos phi_i, r_i sin phi_i, z_i), computed in float64, multiplied by the
    3 x 3 `rot` when one is given (so that successive passes use different sets) and rounded once
    to float32.  The pass flips each direction into the hit normal's hemisphere.  The function only
    makes inputs: the device contract is exact for whatever set it is given."""
    n = int(n)
    if not 1 <= n <= AO_MAX_DIRS:
        raise ValueError(f"ao_dirs: n {n} is not 1..{AO_MAX_DIRS}")
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    u = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    if rot is not None:
        m = np.asarray(rot, dtype=np.float64)
        if m.shape != (3, 3):
            raise ValueError(f"ao_dirs: rot is a 3 x 3 matrix, got shape {m.shape}")
        u = u @ m.T
    return u.astype(np.float32), float(tmax)


def _rc_ao_dirs(dirs, what):
    """The RcAoDirs of a set (u, tmax): u is [n, 3], used as given (the library checks it)."""
    try:
        u, tmax = dirs
        u = np.ascontiguousarray(u, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: a direction set is a (u [n, 3], tmax) pair") from None
    if u.ndim != 2 or u.shape[1] != 3 or not 1 <= len(u) <= AO_MAX_DIRS:
        raise ValueError(f"{what}: u is [n, 3] with n in 1..{AO_MAX_DIRS}, got shape {u.shape}")
    d = RcAoDirs(n=len(u), tmax=float(tmax))
    ctypes.memmove(d.u, u.ctypes.data, u.nbytes)
    return d


def ao_dirs_check(dirs):
    """rc_ao_dirs_check: True when the library takes the set (u, tmax): tmax in (0, +inf], every
    direction finite and not zero (its message goes to stderr otherwise)."""
    return hip_lib().rc_ao_dirs_check(ctypes.byref(_rc_ao_dirs(dirs, "ao_dirs_check"))) == 0


def ao_flip(N, u):
    """The pass's directions at a hit: [..., n, 3] float32, u_j * -1.0f where the float dot
    (N0 u0 + N1 u1) + N2 u2 is below zero and u_j as given elsewhere (a zero or NaN dot does not
    flip).  N is [..., 3], u is [n, 3]."""
    N = np.asarray(N, dtype=np.float32)[..., None, :]
    u = np.asarray(u, dtype=np.float32)
    with np.errstate(all="ignore"):
        d = N[..., 0] * u[:, 0]
        d = d + N[..., 1] * u[:, 1]
        d = d + N[..., 2] * u[:, 2]
        return np.where((d < 0)[..., None], u * np.float32(-1.0), u).astype(np.float32)


def _ao_state(acc):
    acc = np.asarray(acc)
    if acc.dtype != AO_DTYPE or acc.ndim != 2:
        raise ValueError(f"an occlusion state is [H, W] of AO_DTYPE, got {acc.dtype} {acc.shape}")
    return acc


def ao_step(acc, open_add, n, reset=False):
    """One occlusion pass in numpy: (acc', saturated).  acc is [H, W] of AO_DTYPE, open_add [H, W]
    the pass's open rays per pixel (n at a primary miss), n its directions.  A pixel whose rays + n
    would pass 65535 is saturated and keeps its record; `reset` takes every record as zero."""
    acc, n = _ao_state(acc), int(n)
    add = np.asarray(open_add)
    if not 1 <= n <= AO_MAX_DIRS or add.shape != acc.shape or (add < 0).any() or (add > n).any():
        raise ValueError(f"ao_step: n {n} (1..{AO_MAX_DIRS}) and open_add {add.shape} in 0..n for "
                         f"a state of {acc.shape}")
    rays = np.zeros(acc.shape, np.uint32) if reset else acc["rays"].astype(np.uint32)
    opn = np.zeros(acc.shape, np.uint32) if reset else acc["open"].astype(np.uint32)
    sat = rays + n > AO_MAX_RAYS
    new = np.zeros(acc.shape, AO_DTYPE)
    new["open"] = np.where(sat, opn, opn + add.astype(np.uint32))
    new["rays"] = np.where(sat, rays, rays + n)
    return new, int(sat.sum())


def ao_byte(acc):
    """rc_ao_byte of every record: (510 open + rays) // (2 rays), 255 where rays is 0."""
    acc = _ao_state(acc)
    opn, rays = acc["open"].astype(np.int64), acc["rays"].astype(np.int64)
    return np.where(rays > 0, (510 * opn + rays) // np.maximum(2 * rays, 1), 255).astype(np.uint8)


def _ray_words(a, n, dtype, what, name):
    """A per-ray word array of an occlusion batch ([n] of dtype), or None."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.shape != (n,):
        raise ValueError(f"{what}: {name} is [n] like the rays ({n}), got shape {a.shape}")
    return a


def occluded_rays(scene, origins, dirs, skip=None, tmax=None, depth=6, mode="fast", device=0,
                  timing=None):
    """rc_occluded_rays: is ray k, leaving origins[k] along dirs[k] (both [n, 3] float32, used as
    given), blocked by a shape other than skip[k] (int32, None: -1 everywhere) at 0 < t < tmax[k]
    (float32 in units of |dirs[k]|, None: +inf everywhere)?  [n] uint8, 1 blocked.  With tmax inf
    that is the reference's shadow test.  Fast mode only."""
    d = _ray_dirs(dirs)
    o = np.asarray(origins)
    if o.shape != d.shape:
        raise ValueError(f"occluded_rays: origins is an [n, 3] array like dirs {d.shape}, got "
                         f"{o.shape}")
    o = np.ascontiguousarray(o, dtype=np.float32)
    s = _ray_words(skip, len(d), np.int32, "occluded_rays", "skip")
    tm = _ray_words(tmax, len(d), np.float32, "occluded_rays", "tmax")
    out = np.zeros(len(d), dtype=np.uint8)
    opt = options(depth, mode, 1, device)
    with _timed(timing) as (t, _):
        _call("rc_occluded_rays", scene.packed(), ctypes.byref(opt), len(d), _host_ptr(o),
              _host_ptr(d), None if s is None else _host_ptr(s),
              None if tm is None else _host_ptr(tm), _host_ptr(out), None, ctypes.byref(t))
    return out


def occluded_rays_device(scene, n, d_origins_ptr, d_dirs_ptr, d_out_ptr, d_skip_ptr=None,
                         d_tmax_ptr=None, stream_ptr=None, depth=6, mode="fast", timing=None):
    """rc_occluded_rays_device: the n rays, the optional per-ray words and the n bytes in device
    memory, enqueued on the stream and asynchronous unless `timing` is given."""
    opt = options(depth, mode)
    with _timed(timing) as (_, t):
        _call("rc_occluded_rays_device", scene.packed(), ctypes.byref(opt), int(n),
              ctypes.c_void_p(d_origins_ptr), ctypes.c_void_p(d_dirs_ptr),
              ctypes.c_void_p(d_skip_ptr or 0), ctypes.c_void_p(d_tmax_ptr or 0),
              ctypes.c_void_p(d_out_ptr), _stream(stream_ptr), t)


def ao_pass_device(scene, eye, m, width, height, dirs, d_ao_ptr, d_out_ptr=None, window=None,
                   reset=False, stream_ptr=None, depth=6, mode="fast", timing=None):
    """rc_ao_pass_device: one ambient-occlusion pass of the camera (eye, m) with the set dirs =
    (u, tmax) into the state at d_ao_ptr (width * height AO_DTYPE records, device memory): from
    every primary hit the flipped directions (ao_flip) with the hit shape skipped, counted by
    ao_step; d_out_ptr (or None): the width * height bytes of ao_byte.  Fast mode only."""
    cam = _rc_camera(eye, m)
    d = _rc_ao_dirs(dirs, "ao_pass_device")
    win = None if window is None else ctypes.byref(_rc_window(window))
    opt = options(depth, mode)
    with _timed(timing) as (_, t):
        _call("rc_ao_pass_device", scene.packed(), ctypes.byref(cam), win, width, height,
              ctypes.byref(opt), ctypes.byref(d), 1 if reset else 0, ctypes.c_void_p(d_ao_ptr),
              ctypes.c_void_p(d_out_ptr or 0), _stream(stream_ptr), t)


def ao_resolve_device(d_ao_ptr, width, height, d_out_ptr, stream_ptr=None):
    """rc_ao_resolve_device: the bytes of a state (ao_byte), nothing shot."""
    _call("rc_ao_resolve_device", ctypes.c_void_p(d_ao_ptr), width, height,
          ctypes.c_void_p(d_out_ptr), _stream(stream_ptr))


def render_ao(scene, eye, m, width, height, sets, window=None, depth=6, device=0, mode="fast",
              timing=None, out=None):
    """rc_render_ao: the [H, W] uint8 occlusion plane of the camera (eye, m) after a reset pass
    with sets[0] and one pass for each further set; `sets` is one (u, tmax) pair or a list of
    them.  255 is open sky, 0 fully enclosed.  Fast mode only."""
    single = isinstance(sets, tuple) and len(sets) == 2 and np.ndim(sets[1]) == 0
    pairs = [sets] if single else list(sets)
    if not 1 <= len(pairs) <= AO_MAX_SETS:
        raise ValueError(f"render_ao: {len(pairs)} sets, it takes 1..{AO_MAX_SETS}")
    arr = (RcAoDirs * len(pairs))(*[_rc_ao_dirs(p, "render_ao") for p in pairs])
    cam = _rc_camera(eye, m)
    win = None if window is None else ctypes.byref(_rc_window(window))
    if out is None:
        out = np.empty((height, width), dtype=np.uint8)
    assert out.shape == (height, width) and out.dtype == np.uint8 and out.flags.c_contiguous
    opt = options(depth, mode, 1, device)
    with _timed(timing) as (t, _):
        _call("rc_render_ao", scene.packed(), ctypes.byref(cam), win, width, height,
              ctypes.byref(opt), arr, len(arr), _host_ptr(out), ctypes.byref(t))
    return out


def ao_stats():
    """The last occlusion pass on the current device: hit_pixels (unsaturated pixels whose primary
    ray hit), rays (occlusion rays shot), blocked (of those) and saturated (pixels left as they
    were)."""
    return _stats("rc_ao_stats_get", RcAoStats,
                  "no ambient-occlusion pass has run on the current device")


def ao_phase_ms():
    """The span of the last occlusion call's kernels in ms: {"ao": ...}."""
    return _phase_ms("rc_ao_phase_ms", ("ao",),
                     "no ambient-occlusion call has been recorded on the current device")


def ao_filter_params(radius, taps="tent", nmin=0.9, dplane=0.05):
    """An RcAoFilter: `taps` is "tent" (taps[d] = radius + 1 - d, rc_ao_filter_tent), "box" (taps 1,
    rc_ao_filter_box) or a sequence of radius + 1 integers taps[|d|]; nmin and dplane are the two
    thresholds of ao_filter's rule.  The library checks the values (ao_filter_check)."""
    radius = int(radius)
    if not 0 <= radius <= AO_FILTER_MAX_RADIUS:
        raise ValueError(f"ao_filter_params: radius {radius} is not 0..{AO_FILTER_MAX_RADIUS}")
    f = RcAoFilter()
    if isinstance(taps, str):
        if taps not in ("tent", "box"):
            raise ValueError(f"ao_filter_params: taps {taps!r} is not 'tent', 'box' or a sequence")
        make = "rc_ao_filter_tent" if taps == "tent" else "rc_ao_filter_box"
        _call(make, radius, ctypes.byref(f))
    else:
        k = [int(v) for v in taps]
        if len(k) != radius + 1 or any(not 0 <= v <= 65535 for v in k):
            raise ValueError(f"ao_filter_params: taps is radius + 1 = {radius + 1} values in "
                             f"0..65535, got {k}")
        f.radius = radius
        for d, v in enumerate(k):
            f.taps[d] = v
    f.nmin, f.dplane = float(nmin), float(dplane)
    return f


def ao_filter_check(params):
    """rc_ao_filter_check: True when the library takes the filter (its message goes to stderr
    otherwise)."""
    return hip_lib().rc_ao_filter_check(ctypes.byref(params)) == 0


def ao_filter(acc, ids, P, N, params):
    """rc_ao_filter_device's rule in numpy: the [H, W] uint8 plane of the state acc ([H, W] of
    AO_DTYPE) pooled over the (2 radius + 1)^2 window under the guide ids [H, W] int32, P and N
    [H, W, 3] float32.  Pixel q is pooled into p when q == p, or id_q == id_p and, in float32 in
    this order, nd = (Np0 Nq0 + Np1 Nq1) + Np2 Nq2 >= nmin and |pd| <= dplane with e = P_q - P_p,
    pd = (Np0 e0 + Np1 e1) + Np2 e2; its weight is taps[|dx|] taps[|dy|]; the byte is
    (510 O + R) // (2 R) of the weighted sums of open and rays (255 where R is 0), and ao_byte of
    the pixel's own record where id_p < 0.  Vectorised over the offsets, int64 sums."""
    acc = _ao_state(acc)
    h, w = acc.shape
    ids = np.asarray(ids)
    P, N = np.asarray(P), np.asarray(N)
    if ids.shape != (h, w) or ids.dtype != np.int32 or P.shape != (h, w, 3) or \
            N.shape != (h, w, 3) or P.dtype != np.float32 or N.dtype != np.float32:
        raise ValueError(f"ao_filter: ids int32 {(h, w)}, P and N float32 {(h, w, 3)} like the "
                         f"state, got {ids.dtype} {ids.shape}, {P.dtype} {P.shape}, {N.dtype} "
                         f"{N.shape}")
    r = int(params.radius)
    taps = [int(params.taps[d]) for d in range(r + 1)]
    nmin, dplane = np.float32(params.nmin), np.float32(params.dplane)
    opn, rays = acc["open"].astype(np.int64), acc["rays"].astype(np.int64)
    O, R = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            ya, yb = max(0, -dy), min(h, h - dy)          # rows of p whose q is inside
            if ya >= yb:
                continue
            for dx in range(-r, r + 1):
                xa, xb = max(0, -dx), min(w, w - dx)
                if xa >= xb:
                    continue
                ps = (slice(ya, yb), slice(xa, xb))
                qs = (slice(ya + dy, yb + dy), slice(xa + dx, xb + dx))
                if dx == 0 and dy == 0:
                    ok = np.ones((yb - ya, xb - xa), bool)
                else:
                    Np, Nq, e = N[ps], N[qs], P[qs] - P[ps]
                    nd = (Np[..., 0] * Nq[..., 0] + Np[..., 1] * Nq[..., 1]) + Np[..., 2] * Nq[..., 2]
                    pd = (Np[..., 0] * e[..., 0] + Np[..., 1] * e[..., 1]) + Np[..., 2] * e[..., 2]
                    ok = (ids[qs] == ids[ps]) & (nd >= nmin) & (np.abs(pd) <= dplane)
                wgt = taps[abs(dx)] * taps[abs(dy)]
                O[ps] += np.where(ok, wgt * opn[qs], 0)
                R[ps] += np.where(ok, wgt * rays[qs], 0)
    pooled = np.where(R > 0, (510 * O + R) // np.maximum(2 * R, 1), 255)
    return np.where(ids < 0, ao_byte(acc), pooled).astype(np.uint8)


def ao_filter_device(d_ao_ptr, d_id_ptr, d_P_ptr, d_N_ptr, width, height, params, d_out_ptr,
                     stream_ptr=None):
    """rc_ao_filter_device: ao_filter of the state at d_ao_ptr under the guide planes at d_id_ptr,
    d_P_ptr and d_N_ptr (all width x height, device memory) into the width * height bytes at
    d_out_ptr; no scene, enqueued on the stream."""
    g = RcGbuffer(d_id_ptr or None, None, d_P_ptr or None, d_N_ptr or None)
    _call("rc_ao_filter_device", ctypes.c_void_p(d_ao_ptr), ctypes.byref(g), width, height,
          ctypes.byref(params), ctypes.c_void_p(d_out_ptr), _stream(stream_ptr))


def ao_compose(rgb, ids, ao, table):
    """rc_ao_compose_device's integer step in numpy: out[c] = min(255, rgb[c] + (table[id][c] * ao +
    127) // 255) where 0 <= id < len(table), rgb elsewhere.  rgb [H, W, 3] uint8, ids [H, W] int32,
    ao [H, W] uint8, table [n_shapes, 3] uint8 (quant(ambient[c] * diffuse_color_k[c]))."""
    rgb, ids, ao = np.asarray(rgb), np.asarray(ids), np.asarray(ao)
    table = np.asarray(table)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or ids.shape != rgb.shape[:2] or \
            ao.shape != ids.shape or ao.dtype != np.uint8 or table.dtype != np.uint8 or \
            table.ndim != 2 or table.shape[1] != 3:
        raise ValueError(f"ao_compose: rgb [H, W, 3] uint8, ids [H, W], ao [H, W] uint8 and table "
                         f"[n, 3] uint8, got {rgb.shape}, {ids.shape}, {ao.shape}, {table.shape}")
    ids = ids.astype(np.int64)
    known = (ids >= 0) & (ids < len(table))
    if len(table) == 0:
        return rgb.copy()
    a = table[np.where(known, ids, 0)].astype(np.int64)
    add = (a * ao.astype(np.int64)[..., None] + 127) // 255
    out = np.minimum(255, rgb.astype(np.int64) + add)
    return np.where(known[..., None], out, rgb).astype(np.uint8)


def _ambient(ambient, what):
    a = np.asarray(ambient, dtype=np.float32)
    if a.shape != (3,):
        raise ValueError(f"{what}: ambient is three floats, got shape {a.shape}")
    return (ctypes.c_float * 3)(*a.tolist())


def ao_compose_device(scene, d_id_ptr, d_ao_ptr, ambient, d_rgb_in_ptr, d_rgb_out_ptr, width,
                      height, stream_ptr=None, mode="fast"):
    """rc_ao_compose_device: ao_compose with the table of `scene` and `ambient` (three floats,
    finite, not negative) on device planes; d_rgb_out_ptr may equal d_rgb_in_ptr."""
    opt = options(0, mode)
    _call("rc_ao_compose_device", scene.packed(), ctypes.byref(opt), ctypes.c_void_p(d_id_ptr),
          ctypes.c_void_p(d_ao_ptr), _ambient(ambient, "ao_compose_device"),
          ctypes.c_void_p(d_rgb_in_ptr), ctypes.c_void_p(d_rgb_out_ptr), width, height,
          _stream(stream_ptr))


def render_ambient(scene, eye, m, width, height, sets, params, ambient, window=None, depth=6,
                   device=0, mode="fast", timing=None, out=None):
    """rc_render_ambient: render_camera's [H, W, 3] image at ssaa = 1 plus the ambient term:
    render_ao's passes with `sets`, the camera's G-buffer, ao_filter with `params` and ao_compose
    with `ambient`, all on the device.  Fast mode only."""
    single = isinstance(sets, tuple) and len(sets) == 2 and np.ndim(sets[1]) == 0
    pairs = [sets] if single else list(sets)
    if not 1 <= len(pairs) <= AO_MAX_SETS:
        raise ValueError(f"render_ambient: {len(pairs)} sets, it takes 1..{AO_MAX_SETS}")
    arr = (RcAoDirs * len(pairs))(*[_rc_ao_dirs(p, "render_ambient") for p in pairs])
    cam = _rc_camera(eye, m)
    win = None if window is None else ctypes.byref(_rc_window(window))
    out = _pixmap(out, width, height)
    opt = options(depth, mode, 1, device)
    with _timed(timing) as (t, _):
        _call("rc_render_ambient", scene.packed(), ctypes.byref(cam), win, width, height,
              ctypes.byref(opt), arr, len(arr), ctypes.byref(params),
              _ambient(ambient, "render_ambient"), _host_ptr(out), ctypes.byref(t))
    return out


def window_from_env(width, height, mode="fast", ssaa=1, adaptive=0, gpus=1):
    """raycast()'s reading of RAYCAST_WINDOW (rc_window_env) for a width x height frame of that
    mode, factor, adaptive threshold and GPU count: (full_w, full_h, x0, y0) when the frame goes
    through the window path, None when it does not (the warnings go to stderr)."""
    win = RcWindow()
    opt = options(mode=mode, gpus=gpus, ssaa=ssaa, adaptive=adaptive)
    if hip_lib().rc_window_env(ctypes.byref(opt), int(width), int(height),
                               ctypes.byref(win)) != 1:
        return None
    return win.full_w, win.full_h, win.x0, win.y0


SPIN_SITES = ("team_handoff", "phase_c_carry_in", "ready_queue", "helper_queue")


def resolver_stats(lone=False):
    """Resolver diagnostics (rc_resolver_stats_get): the last rc_frames_wait window (frames in
    flight), or with lone=True the one-frame-at-a-time renders read back since the last such
    call.  A dict; spin waits by site in microseconds."""
    st = RcResolverStats()
    if hip_lib().rc_resolver_stats_get(1 if lone else 0, ctypes.byref(st)) != 0:
        raise RuntimeError("rc_resolver_stats_get failed")
    d = {k: getattr(st, k) for k, _ in RcResolverStats._fields_ if k not in ("pad", "spin_wait_us_max")}
    d["spin_wait_us_max"] = {n: round(st.spin_wait_us_max[i], 1) for i, n in enumerate(SPIN_SITES)}
    return d


def lone_frames_check():
    """Synchronise the device and read back every one-frame-at-a-time parity frame's hand-off
    words since the previous check (rc_lone_frames_check): {"checked": n, "failed": 0}; raises
    if a frame failed."""
    c, f = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = hip_lib().rc_lone_frames_check(ctypes.byref(c), ctypes.byref(f))
    if rc != 0:
        raise RuntimeError(f"rc_lone_frames_check: {f.value} of {c.value} frames failed (see stderr)")
    return {"checked": c.value, "failed": f.value}


def inject_error(nth_frame):
    """Test aid (rc_debug_inject_error): the nth_frame-th parity frame from now (0 = next)
    fails its carry hand-off as a timed-out spin would; -1 cancels."""
    if hip_lib().rc_debug_inject_error(int(nth_frame)) != 0:
        raise ValueError(nth_frame)


def scatter_selftest(ndep, seed=0, skip=0):
    """Test aid (rc_debug_scatter_selftest, no GPU): rc_render's in-frame scatter against a
    host writer thread; returns the number of wrong pixmap bytes or the failure status."""
    lib = hip_lib()
    lib.rc_debug_scatter_selftest.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
    return lib.rc_debug_scatter_selftest(int(ndep), int(seed), int(skip))


def debug_carry_ins():
    """Test aid (rc_debug_carry_ins): what the resolver published in the device's last
    one-frame-at-a-time parity frame (render on one GPU, render_device), read back from the
    frame's workspace: (pix int64[n] the DEP pixels y * W + x in scan order, carry float32[n, 3]
    each entry's carry-in, hit uint8[n] its hit bit, first_bad: the first entry whose tags are not
    the frame's epoch, or -1).  Raises if there is no such frame or its hand-off failed."""
    lib = hip_lib()
    lib.rc_debug_carry_ins.argtypes = [ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)] + \
        [ctypes.c_void_p] * 3 + [ctypes.POINTER(ctypes.c_int64)]
    n, bad = ctypes.c_int64(0), ctypes.c_int64(-1)
    rc = lib.rc_debug_carry_ins(0, ctypes.byref(n), None, None, None, None)
    if rc != 0:
        raise RuntimeError(f"rc_debug_carry_ins: {rc} (no completed parity frame in the workspace, or "
                           f"its hand-off failed)")
    pix = np.zeros(n.value, np.int64)
    carry = np.zeros((n.value, 3), np.float32)
    hit = np.zeros(n.value, np.uint8)
    if n.value:
        rc = lib.rc_debug_carry_ins(n.value, ctypes.byref(n), pix.ctypes.data, carry.ctypes.data,
                                    hit.ctypes.data, ctypes.byref(bad))
        if rc != 0 or n.value != len(pix):
            raise RuntimeError(f"rc_debug_carry_ins: {rc}")
    return pix, carry, hit, int(bad.value)


def write_p3(img, path):
    """ppm_WriteOutP3 (C/ppm.c:168-184, the product's byte-identical writer) of an [H, W, 3]
    uint8 image into `path`."""
    lib = front_lib()
    h, w, _ = img.shape
    img = np.ascontiguousarray(img)
    p = PPMFormat(w, h, w * h * 3, 255, 0, None, img.ctypes.data)
    f = _libc.fopen(os.fsencode(path), b"wb")
    if not f:
        raise OSError(path)
    try:
        lib.ppm_WriteOutP3(p, ctypes.c_void_p(f))
    finally:
        _libc.fclose(f)


def p3_bytes(img):
    """The P3 file the reference would write for img (C/ppm.c:168-184), produced by the
    product writer into memory (open_memstream)."""
    lib = front_lib()
    h, w, _ = img.shape
    img = np.ascontiguousarray(img)
    p = PPMFormat(w, h, w * h * 3, 255, 0, None, img.ctypes.data)
    buf, size = ctypes.c_void_p(), ctypes.c_size_t()
    f = _libc.open_memstream(ctypes.byref(buf), ctypes.byref(size))
    if not f:
        raise MemoryError("open_memstream")
    lib.ppm_WriteOutP3(p, ctypes.c_void_p(f))
    _libc.fclose(f)
    try:
        return ctypes.string_at(buf, size.value)
    finally:
        _libc.free(buf)


def p3_md5(img):
    """md5 of the P3 file the reference would write for img (C/ppm.c:168-184)."""
    import hashlib
    return hashlib.md5(p3_bytes(img)).hexdigest()


def pipe_reset():
    """Wait for every frame, then release the frame pipeline (rc_pipe_reset); the next
    frame_submit rebuilds it from the current RC_PIPE_* environment."""
    if hip_lib().rc_pipe_reset() != 0:
        raise RuntimeError("rc_pipe_reset failed: a resolver hand-off timed out (see stderr)")


def last_kernel_ms():
    return hip_lib().rc_last_kernel_ms()


def profile_begin():
    """Start a per-phase kernel timing window on the current device (rc_profile_begin)."""
    if hip_lib().rc_profile_begin() != 0:
        raise RuntimeError("rc_profile_begin failed")


def profile_end():
    """Close the window: per-phase kernel times (ms) averaged over the renders inside it."""
    return _stats("rc_profile_end", RcPhaseStats, "rc_profile_end failed")


def encode_p3(img):
    """The reference P3 byte stream (C/ppm.c:168-184) of an [H, W, 3] uint8 image."""
    h, w, _ = img.shape
    table = [f"{v}\n".encode() for v in range(256)]
    body = b"".join(table[v] for v in img.reshape(-1).tolist())
    return f"P3\n{w} {h} \n255\n".encode() + body


def version():
    return hip_lib().rc_version().decode()


# ------------------------------------------------------------- multi-GPU row shards --
XFER = {"auto": 0, "rccl": 1, "copy": 2}
GROUP_ID_BYTES = 128


class Group:
    """Row-sharded rendering over several GPUs (rc_group / rc_render_sharded):
    row y -> rank y % G, RCCL gathers to rank 0; parity adds the DEP-entry gather, the
    carry resolver on the root and the carry-in scatter.  `Group.local([0, 1, 2])` drives all
    ranks from this process; `Group.rank(world, rank, uid, device)` is one rank of a
    one-process-per-GPU job (uid from `Group.unique_id()` on rank 0, shared by the caller)."""

    def __init__(self, handle):
        if not handle:
            raise RuntimeError("rc_group creation failed (see stderr)")
        self._h = handle

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(GROUP_ID_BYTES)
        if hip_lib().rc_group_unique_id(buf) != 0:
            raise RuntimeError("rc_group_unique_id failed")
        return buf.raw

    @classmethod
    def local(cls, devices, transport="auto"):
        arr = (ctypes.c_int * len(devices))(*devices)
        return cls(hip_lib().rc_group_create_local(len(devices), arr, XFER[transport]))

    @classmethod
    def rank(cls, world, rank, uid, device):
        assert len(uid) == GROUP_ID_BYTES
        return cls(hip_lib().rc_group_create_rank(world, rank, uid, device))

    @property
    def size(self):
        return hip_lib().rc_group_size(self._h)

    @property
    def transport(self):
        return {1: "rccl", 2: "copy"}[hip_lib().rc_group_transport(self._h)]

    def render(self, scene, width, height, d_image_ptr=None, depth=6, mode="parity",
               timing=None):
        """Collective render; the root's image lands at d_image_ptr (W*H*3 B on rank 0's
        device)."""
        opt = options(depth, mode)
        with _timed(timing) as (t, _):
            _call("rc_render_sharded", self._h, scene.packed(), width, height, ctypes.byref(opt),
                  ctypes.c_void_p(d_image_ptr or 0), ctypes.byref(t))

    def stats(self):
        return _stats("rc_group_last_stats", RcShardStats, "rc_group_last_stats failed", self._h)

    def rank_stats(self, rank):
        """One rank's own timeline of the last render (rc_group_rank_stats), or None when this
        process does not drive that rank."""
        st = RcRankStats()
        if hip_lib().rc_group_rank_stats(self._h, int(rank), ctypes.byref(st)) != 0:
            return None
        return {k: getattr(st, k) for k, _ in RcRankStats._fields_}

    def debug_bound(self, per_rank):
        """Test aid (rc_group_debug_bound): the fixed-size entry exchange's per-rank bound."""
        if hip_lib().rc_group_debug_bound(self._h, int(per_rank)) != 0:
            raise ValueError(per_rank)

    def close(self):
        if self._h:
            hip_lib().rc_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def row_shard(height, rank, world):
    """Rows of rank `rank` under the row-cyclic partition (row y -> rank y % world):
    (row0, row_step, nrows).  Contiguous blocks are 1.7-2.1x imbalanced on the reference
    scenes at 8 ranks; cyclic rows are within ~2%."""
    return rank, world, (height - rank + world - 1) // world


def deinterleave(gathered, height):
    """Undo the row-cyclic partition: image row y = gathered[y % world][y // world] (the
    host-side statement of k_deinterleave, for the CPU protocol tests)."""
    world, rows_max, w, c = gathered.shape
    full = gathered.permute(1, 0, 2, 3).reshape(rows_max * world, w, c)
    return full[:height]
