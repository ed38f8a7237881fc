"""The sampling family's refusals and environment warnings, pinned byte for byte (no GPU).

Everything these entry points refuse is refused from the arguments alone, before the first HIP
call, with one message on stderr and -1; the RAYCAST_FILTER / RAYCAST_PATTERN / RAYCAST_WINDOW
readers warn and decide in the same way.  One table of calls (REFUSALS, ENV) feeds both tests
and tests/golden/make_refusals_golden.py, which recorded tests/golden/refusals.json.  A call
that breaks two rules pins the order of the clauses: the first message is the one printed.
"""
import ctypes
import json
import os
import tempfile

import numpy as np
import pytest

from helpers import GOLDEN, rc, scene_path

GOLDEN_FILE = os.path.join(GOLDEN, "refusals.json")
FAKE = 4096      # a non-null, 8-byte aligned "device pointer" that a refused call never follows
ODD = 4100       # the same, not 8-byte aligned
_PIX = np.zeros((8, 8, 3), dtype=np.uint8)
HOST = _PIX.ctypes.data
_scene = None


def scene():
    global _scene
    if _scene is None:
        _scene = rc.Scene.from_file(scene_path("simple"))
    return _scene.packed()


def O(mode="fast", **kw):
    return rc.options(6, mode, **kw)


def _lattice(cls, g, pts, n=None):
    p = cls()
    p.grid, p.nsamples = g, len(pts) if n is None else n
    for k, (x, y) in enumerate(pts):
        p.x[k], p.y[k] = x, y
    return p


def PAT(g, pts, n=None):
    return _lattice(rc.RcPattern, g, pts, n)


def SEQ(g, pts, n=None):
    return _lattice(rc.RcSampleSeq, g, pts, n)


def FILT(taps, n=None):
    f = rc.RcFilter()
    f.ntaps = len(taps) if n is None else n
    for i, k in enumerate(taps):
        f.taps[i] = k
    return f


def WIN(fw, fh, x0, y0):
    w = rc.RcWindow()
    w.full_w, w.full_h, w.x0, w.y0 = fw, fh, x0, y0
    return w


def ref(x):
    return None if x is None else ctypes.byref(x)


RGSS4 = rc.PATTERNS["rgss4"]
GOODP = PAT(*RGSS4)
GOODS = SEQ(*RGSS4)
TENT4 = FILT(rc.filter_tent(4))
BOX2 = FILT([1, 1])
GOODW = WIN(64, 48, 8, 4)
S = "scene"      # stands for the packed scene handle in an argument list

# the options that every feature with a grid of its own refuses, in clause order; `two`: calls
# that break two rules at once
BAD_OPTS = {"ssaa3": O(ssaa=3), "ssaa-1": O(ssaa=-1), "thr_no_factor": O(ssaa=1, adaptive=16),
            "ssaa2": O(ssaa=2), "ssaa4_adaptive": O(ssaa=4, adaptive=16), "parity": O("parity"),
            "gpus2": O(gpus=2), "cuda_gpus2": O("cuda", gpus=2),
            "two_ssaa2_parity": O("parity", ssaa=2), "two_parity_gpus2": O("parity", gpus=2),
            "two_ssaa3_parity": O("parity", ssaa=3)}

REFUSALS = []    # (id, export, argument list)


def case(tag, export, *args):
    REFUSALS.append((f"{export}[{tag}]", export, args))


def pair(tag, name, lead, tail_host=(), tail_dev=()):
    """The host-pixmap entry and its *_device twin with the same leading arguments."""
    case(tag, name, *lead, *tail_host, HOST, None)
    case(tag, name + "_device", *lead, *tail_dev, FAKE, None, None)


# ---------------------------------------------------------------- the four checks --
BAD_FILTERS = {"factor3": (TENT4, 3), "taps25": (FILT([1] * 24, 25), 4),
               "taps3_s4": (FILT([1] * 3), 4),
               "odd_halo": (FILT([1] * 5), 4), "wide_halo": (FILT([1] * 8), 2),
               "sum0": (FILT([1, -1, 1, -1]), 4), "sum_neg": (FILT([-1] * 4), 4),
               "mag": (FILT([1000, 1000, -500, 100]), 4),
               "two_factor_taps": (FILT([1] * 24, 25), 3),
               "two_sum_mag": (FILT([-2000, 100, 100, 100]), 4)}
case("null", "rc_filter_check", None, 4)
for tag, (f, s) in BAD_FILTERS.items():
    case(tag, "rc_filter_check", ref(f), s)

BAD_LATTICES = {"grid3": (3, [(0, 0), (1, 1)], None), "grid0": (0, [(0, 0), (1, 1)], None),
                "off_x": (2, [(0, 0), (2, 1)], None),
                "off_y": (4, [(0, 0), (1, 4), (2, 2), (3, 3)], None),
                "duplicate": (4, [(1, 0), (3, 1), (1, 0), (2, 3)], None),
                "two_off_dup": (2, [(0, 0), (0, 0), (2, 0), (1, 1)], None),
                "two_grid_off": (3, [(0, 0), (5, 5)], None)}
BAD_PATTERNS = dict(BAD_LATTICES, n3=(4, [(0, 0), (1, 1), (2, 2)], None), n0=(4, [], None),
                    n32=(8, [], 32), n8_g2=(2, [(0, 0), (1, 0), (0, 1), (1, 1)], 8),
                    n16_g2=(2, [], 16), two_grid_n=(5, [(0, 0), (1, 1), (2, 2)], None))
BAD_SEQS = dict(BAD_LATTICES, n0=(4, [], None), n_neg=(4, [], -1), n5_g2=(2, [], 5),
                n17_g4=(4, [], 17), n65_g8=(8, [], 65), two_grid_n=(5, [], 0))
case("null", "rc_pattern_check", None)
for tag, (g, pts, n) in BAD_PATTERNS.items():
    case(tag, "rc_pattern_check", ref(PAT(g, pts, n)))
case("null", "rc_sample_seq_check", None)
for tag, (g, pts, n) in BAD_SEQS.items():
    case(tag, "rc_sample_seq_check", ref(SEQ(g, pts, n)))

BAD_WINDOWS = {"factor3": (GOODW, 16, 16, 3), "factor-1": (GOODW, 16, 16, -1),
               "full_w0": (WIN(0, 48, 0, 0), 16, 16, 1), "full_h-1": (WIN(64, -1, 0, 0), 16, 16, 1),
               "w0": (GOODW, 0, 16, 1), "h-1": (GOODW, 16, -1, 2),
               "x0_neg": (WIN(64, 48, -1, 0), 16, 16, 1), "y0_neg": (WIN(64, 48, 0, -8), 16, 16, 4),
               "outside_x": (WIN(64, 48, 49, 0), 16, 16, 1),
               "outside_y": (WIN(64, 48, 0, 40), 16, 16, 1),
               "x0_past": (WIN(64, 48, 65, 0), 1, 1, 1), "wider": (WIN(64, 48, 0, 0), 65, 16, 0),
               "past_int": (WIN(1 << 30, 48, 0, 0), 16, 16, 4),
               "past_int_h": (WIN(64, 1 << 28, 0, 0), 16, 16, 8),
               "grid_rows": (WIN(64, 1 << 22, 0, 0), 16, 1 << 22, 1),
               "grid_rows_s8": (WIN(64, 1 << 20, 0, 0), 16, 1 << 18, 8),
               "two_factor_size": (WIN(0, 48, 0, 0), 16, 16, 3),
               "two_size_origin": (WIN(64, 48, -1, 0), 0, 16, 1),
               "two_origin_outside": (WIN(64, 48, -1, 40), 16, 16, 1),
               "two_outside_int": (WIN(1 << 30, 48, 0, 40), 16, 16, 4)}
case("null", "rc_window_check", None, 16, 16, 1)
for tag, (w, W, H, s) in BAD_WINDOWS.items():
    case(tag, "rc_window_check", ref(w), W, H, s)

# ------------------------------------------------------------------- rate maps --
_MAP = np.ones((8, 8), dtype=np.uint8)
_MAP3 = _MAP.copy()
_MAP3[2, 5] = 3
_MAP9 = _MAP.copy()
_MAP9[7, 7], _MAP9[7, 0] = 200, 9


def rates(tag, opt, w=8, h=8, m=_MAP):
    pair(tag, "rc_render_rates", (S, w, h, ref(opt)), (m.ctypes.data,), (FAKE,))


for tag, opt in BAD_OPTS.items():
    rates(tag, opt)
for tag, (w, h) in {"w0": (0, 8), "h0": (8, 0), "w_neg": (-1, 8), "pixels_2^32": (1 << 16, 1 << 16),
                    "side_8w": (1 << 28, 1), "tile_rows": (1, 1 << 24)}.items():
    rates(tag, O(), w, h)
rates("two_w0_ssaa2", O(ssaa=2), 0, 8)
rates("two_gpus2_size", O(gpus=2), 1 << 16, 1 << 16)
rates("cuda_size", O("cuda"), 1 << 16, 1 << 16)
case("map_3", "rc_render_rates", S, 8, 8, ref(O()), _MAP3.ctypes.data, HOST, None)
case("map_9_200", "rc_render_rates", S, 8, 8, ref(O()), _MAP9.ctypes.data, HOST, None)
case("two_parity_map", "rc_render_rates", S, 8, 8, ref(O("parity")), _MAP3.ctypes.data, HOST, None)
for tag, args in {"null_scene": (None, 8, 8, ref(O()), FAKE), "null_opt": (S, 8, 8, None, FAKE),
                  "null_map": (S, 8, 8, ref(O()), None),
                  "two_null_w0": (None, 0, 8, ref(O()), FAKE)}.items():
    case(tag, "rc_render_rates", *args, HOST, None)
    case(tag, "rc_render_rates_device", *args, FAKE, None, None)
case("null_out", "rc_render_rates", S, 8, 8, ref(O()), _MAP.ctypes.data, None, None)
case("null_out", "rc_render_rates_device", S, 8, 8, ref(O()), FAKE, None, None, None)

# ---------------------------------------------------------------- sample patterns --
def pattern(tag, opt, p=GOODP, t=0, w=8, h=8):
    pair(tag, "rc_render_pattern", (S, w, h, ref(opt), ref(p), t))


for tag, opt in BAD_OPTS.items():
    pattern(tag, opt)
pattern("parity_thr", O("parity"), GOODP, 32)
for tag, (g, pts, n) in BAD_PATTERNS.items():
    pattern(tag, O(), PAT(g, pts, n))
for tag, t in {"thr-1": -1, "thr256": 256, "thr65536": 1 << 16}.items():
    pattern(tag, O(), GOODP, t)
for tag, (w, h) in {"w_past": ((1 << 26) + 1, 1), "h_past": (1, (1 << 26) + 1), "w0": (0, 8),
                    "h0": (8, 0), "w_neg": (-1, 8)}.items():
    pattern(tag, O(), GOODP, 0, w, h)
pattern("w_past_g8", O("cuda"), PAT(*rc.PATTERNS["queens8"]), 0, (1 << 25) + 1, 1)
pattern("h_past_g2", O(), PAT(*rc.PATTERNS["diag2"]), 0, 1, (1 << 27) + 1)
pattern("thr_pixels_2^32", O(), GOODP, 16, 1 << 16, 1 << 16)
pattern("thr_pixels_2^32_b", O("cuda"), GOODP, 1, 1 << 26, 64)
pattern("tile_rows", O(), GOODP, 0, 1, 1 << 26)
pattern("tile_rows_thr", O(), GOODP, 16, 1, 1 << 26)
pattern("tile_rows_n16", O(), PAT(4, [(x, y) for y in range(4) for x in range(4)]), 0, 1, 1 << 20)
pattern("two_gpus2_pattern", O(gpus=2), PAT(3, [(0, 0), (1, 1)]))
pattern("two_pattern_thr", O(), PAT(3, [(0, 0), (1, 1)]), 256)
pattern("two_thr_size", O(), GOODP, 256, 0, 8)
pattern("two_size_index", O(), GOODP, 16, (1 << 26) + 1, 1 << 16)
pattern("null_pattern", O(), None)
pattern("null_opt", None)
pattern("two_null_parity", O("parity"), None)
pair("null_scene", "rc_render_pattern", (None, 8, 8, ref(O()), ref(GOODP), 0))
case("null_out", "rc_render_pattern", S, 8, 8, ref(O()), ref(GOODP), 0, None, None)
case("null_out", "rc_render_pattern_device", S, 8, 8, ref(O()), ref(GOODP), 0, None, None, None)

# ------------------------------------------------------------------ accumulation --
def accum(tag, opt, seq=GOODS, first=0, count=1, t=0, reset=0, w=8, h=8, acc=FAKE, out=FAKE,
          win=GOODW, sc=S):
    """rc_accum_pass_device, and rc_accum_pass_window_device through `win`."""
    tail = (ref(opt), ref(seq), first, count, t, reset, acc, out, None, None)
    case(tag, "rc_accum_pass_device", sc, w, h, *tail)
    case(tag, "rc_accum_pass_window_device", sc, ref(win), w, h, *tail)


def render_accum(tag, opt, seq=GOODS, dense=4, t=0, w=8, h=8, sc=S, out=HOST):
    case(tag, "rc_render_accum", sc, w, h, ref(opt), ref(seq), dense, t, out, None)


for tag, opt in BAD_OPTS.items():
    accum(tag, opt)
    render_accum(tag, opt)
for tag, (g, pts, n) in BAD_SEQS.items():
    accum(tag, O(), SEQ(g, pts, n))
    render_accum(tag, O(), SEQ(g, pts, n))
for tag, t in {"thr-1": -1, "thr256": 256}.items():
    accum(tag, O(), t=t)
    render_accum(tag, O(), t=t)
for tag, (w, h, t) in {"w_past": ((1 << 26) + 1, 1, 0), "h_past": (1, (1 << 26) + 1, 0),
                       "w0": (0, 8, 0), "h_neg": (8, -1, 16),
                       "thr_pixels_2^32": (1 << 16, 1 << 16, 16),
                       "tile_rows": (1, 1 << 26, 0)}.items():
    accum(tag, O(), t=t, w=w, h=h, win=WIN(1 << 27, 1 << 27, 0, 0))
    render_accum(tag, O("cuda"), t=t, w=w, h=h)
accum("two_gpus2_seq", O(gpus=2), SEQ(3, [(0, 0)]))
accum("two_seq_thr", O(), SEQ(3, [(0, 0)]), t=256)
accum("two_thr_size", O(), t=-1, w=0)
accum("two_odd_parity", O("parity"), acc=ODD)
accum("two_refused_window", O("parity"), win=WIN(64, 48, 60, 0))
accum("two_window_count", O(), count=0, win=WIN(64, 48, 60, 0))
accum("two_count_reset", O(), count=17, t=16, reset=1)
accum("odd_acc", O(), acc=ODD)
for tag, (first, count) in {"count0": (0, 0), "count17": (0, 17), "first_neg": (-1, 1),
                            "past_end": (3, 2), "first_end": (4, 1)}.items():
    accum(tag, O(), first=first, count=count)
accum("count17_hier8", O(), SEQ(*rc.SAMPLE_SEQS["hier8"]), count=17)
accum("reset_thr", O(), t=16, reset=1)
for tag, w in {"outside": WIN(64, 48, 60, 0), "past_int_g4": WIN(1 << 30, 48, 0, 0),
               "origin": WIN(64, 48, 0, -1)}.items():
    case("window_" + tag, "rc_accum_pass_window_device", S, ref(w), 8, 8, ref(O()), ref(GOODS),
         0, 1, 0, 0, FAKE, FAKE, None, None)
case("null_window", "rc_accum_pass_window_device", S, None, 8, 8, ref(O()), ref(GOODS), 0, 1, 0,
     0, FAKE, FAKE, None, None)
case("two_null_window_scene", "rc_accum_pass_window_device", None, None, 8, 8, ref(O()),
     ref(GOODS), 0, 1, 0, 0, FAKE, FAKE, None, None)
accum("null_scene", O(), sc=None)
accum("null_opt", None)
accum("null_seq", O(), None)
accum("null_acc", O(), acc=None)
accum("null_out", O(), out=None)
accum("two_null_odd", O(), None, acc=ODD)
render_accum("dense0", O(), dense=0)
render_accum("dense5", O(), dense=5)
render_accum("dense_neg", O("cuda"), dense=-1)
render_accum("two_thr_dense", O(), dense=0, t=256)
render_accum("null_scene", O(), sc=None)
render_accum("null_opt", None)
render_accum("null_seq", O(), None)
render_accum("null_out", O(), out=None)
for tag, (acc, w, h, out) in {"null_acc": (None, 8, 8, FAKE), "null_out": (FAKE, 8, 8, None),
                              "odd_acc": (ODD, 8, 8, FAKE), "w0": (FAKE, 0, 8, FAKE),
                              "h_neg": (FAKE, 8, -1, FAKE),
                              "one_grid": (FAKE, 0x7fffffff, 0x7fffffff, FAKE),
                              "two_null_odd": (ODD, 8, 8, None),
                              "two_odd_w0": (ODD, 0, 8, FAKE)}.items():
    case(tag, "rc_accum_resolve_device", acc, w, h, out, None)

# ----------------------------------------------------------------------- windows --
def window(tag, opt, win=GOODW, w=16, h=16):
    pair(tag, "rc_render_window", (S, ref(win), w, h, ref(opt)))


for tag, opt in {"ssaa3": O(ssaa=3), "ssaa-1": O(ssaa=-1), "thr_no_factor": O(ssaa=1, adaptive=16),
                 "ssaa4_adaptive": O(ssaa=4, adaptive=16), "parity": O("parity"),
                 "parity_ssaa2": O("parity", ssaa=2), "gpus2": O(gpus=2),
                 "cuda_gpus2": O("cuda", gpus=2),
                 "two_adaptive_parity": O("parity", ssaa=4, adaptive=16),
                 "two_parity_gpus2": O("parity", gpus=2)}.items():
    window(tag, opt)
for tag, (win, w, h, s) in BAD_WINDOWS.items():
    if s in (0, 1, 2, 4, 8):
        window(tag, O(ssaa=s), win, w, h)
window("two_gpus2_window", O(gpus=2), WIN(64, 48, 60, 0))
window("null_window", O(), None)
window("null_opt", None)
pair("null_scene", "rc_render_window", (None, ref(GOODW), 16, 16, ref(O())))
case("null_out", "rc_render_window", S, ref(GOODW), 16, 16, ref(O()), None, None)
case("null_out", "rc_render_window_device", S, ref(GOODW), 16, 16, ref(O()), None, None, None)

# ----------------------------------------------------------------------- filters --
def filtered(tag, opt, f=TENT4, w=8, h=8):
    pair(tag, "rc_render_filtered", (S, w, h, ref(opt), ref(f)))


for tag, opt in {"ssaa3": O("parity", ssaa=3), "ssaa-1": O(ssaa=-1),
                 "thr_no_factor": O(ssaa=1, adaptive=16),
                 "ssaa4_adaptive": O(ssaa=4, adaptive=16), "ssaa1": O("parity", ssaa=1),
                 "ssaa0": O(ssaa=0),
                 "gpus2": O("parity", ssaa=4, gpus=2),
                 "two_adaptive_gpus2": O(ssaa=4, adaptive=16, gpus=2),
                 "two_ssaa1_gpus2": O("cuda", ssaa=1, gpus=2)}.items():
    filtered(tag, opt)
for tag, (f, s) in BAD_FILTERS.items():
    if s in (2, 4, 8):
        filtered(tag, O("parity", ssaa=s), f)
    case(tag, "rc_filter_image_device", FAKE, 8, 8, s, ref(f), 1 << 20, None)
filtered("filter_of_other_factor", O(ssaa=2), TENT4)
for tag, (s, f, w, h) in {"w0": (4, TENT4, 0, 8), "h_neg": (4, TENT4, 8, -1),
                          "w_past": (4, TENT4, (1 << 26) + 1, 1),
                          "h_past_s2": (2, BOX2, 1, (1 << 27) + 1)}.items():
    filtered(tag, O("parity", ssaa=s), f, w, h)
    case(tag, "rc_filter_image_device", FAKE, w, h, s, ref(f), 1 << 20, None)
filtered("two_gpus2_filter", O(ssaa=4, gpus=2), FILT([1] * 3))
filtered("two_filter_size", O(ssaa=4), FILT([1] * 3), 0, 8)
filtered("null_filter", O(ssaa=4), None)
filtered("null_opt", None)
filtered("two_null_ssaa3", O(ssaa=3), None)
pair("null_scene", "rc_render_filtered", (None, 8, 8, ref(O(ssaa=4)), ref(TENT4)))
case("null_out", "rc_render_filtered", S, 8, 8, ref(O(ssaa=4)), ref(TENT4), None, None)
case("null_out", "rc_render_filtered_device", S, 8, 8, ref(O(ssaa=4)), ref(TENT4), None, None, None)
_SRC = 1 << 20     # an 8 x 8 image at factor 4 is 3072 bytes from _SRC, its output 192 bytes
for tag, dst in {"overlap_same": _SRC, "overlap_inside": _SRC + 3000,
                 "overlap_before": _SRC - 100}.items():
    case(tag, "rc_filter_image_device", _SRC, 8, 8, 4, ref(TENT4), dst, None)
case("two_filter_size", "rc_filter_image_device", FAKE, 0, 8, 4, ref(FILT([1] * 3)), 1 << 20, None)
case("two_size_overlap", "rc_filter_image_device", _SRC, 0, 8, 4, ref(TENT4), _SRC, None)
case("null_src", "rc_filter_image_device", None, 8, 8, 4, ref(TENT4), FAKE, None)
case("null_dst", "rc_filter_image_device", FAKE, 8, 8, 4, ref(TENT4), None, None)
case("null_filter", "rc_filter_image_device", FAKE, 8, 8, 4, None, 1 << 20, None)

assert len({c[0] for c in REFUSALS}) == len(REFUSALS), "duplicate case ids"

# ------------------------------------------------------------- the environment --
ENV_NAMES = ("RAYCAST_FILTER", "RAYCAST_PATTERN", "RAYCAST_WINDOW")
ENV = []    # (id, environment, wrapper, keyword arguments)


def env_case(tag, env, fn, **kw):
    ENV.append((f"{fn}[{tag}]", env, fn, kw))


for tag, v, kw in (("unset", None, dict(ssaa=4)), ("tent", "tent", dict(ssaa=4)),
                   ("tent_s2", "tent", dict(ssaa=2)), ("box", "box", dict(ssaa=8)),
                   ("gauss", "gauss", dict(ssaa=4)), ("empty", "", dict(ssaa=4)),
                   ("tent_ssaa1", "tent", dict(ssaa=1)), ("box_ssaa0", "box", dict(ssaa=0)),
                   ("tent_adaptive", "tent", dict(ssaa=4, adaptive=16)),
                   ("two_gauss_ssaa1", "gauss", dict(ssaa=1)),
                   ("two_gauss_adaptive", "Tent", dict(ssaa=2, adaptive=1))):
    env_case(tag, {} if v is None else {"RAYCAST_FILTER": v}, "filter_from_env", **kw)
for tag, v, kw in (("unset", None, {}), ("rgss4", "rgss4", {}),
                   ("queens8_cuda", "queens8", dict(mode="cuda")),
                   ("rgss4_32", "rgss4:32", dict(ssaa=0)), ("diag2_0", "diag2:0", {}),
                   ("name", "rgss", {}), ("name_empty", "", {}), ("name_colon", ":16", {}),
                   ("thr_empty", "rgss4:", {}), ("thr256", "checker8:256", {}),
                   ("thr_neg", "rgss4:-1", {}),
                   ("thr_tail", "rgss4:16x", {}), ("parity", "rgss4:32", dict(mode="parity")),
                   ("ssaa2", "rgss4", dict(ssaa=2)),
                   ("ssaa4_adaptive", "rgss4", dict(ssaa=4, adaptive=16)),
                   ("two_name_parity", "rgss", dict(mode="parity")),
                   ("two_thr_parity", "rgss4:256", dict(mode="parity")),
                   ("two_parity_ssaa", "rgss4", dict(mode="parity", ssaa=8))):
    env_case(tag, {} if v is None else {"RAYCAST_PATTERN": v}, "pattern_from_env", **kw)
for tag, env, kw in (("unset", {}, {}), ("taken", {"RAYCAST_WINDOW": "64x48+8+4"}, {}),
                     ("taken_ssaa4_cuda", {"RAYCAST_WINDOW": "64x48+48+32"},
                      dict(mode="cuda", ssaa=4)),
                     ("taken_box", {"RAYCAST_WINDOW": "64x48+0+0", "RAYCAST_FILTER": "box"},
                      dict(ssaa=2)),
                     ("taken_pattern_empty", {"RAYCAST_WINDOW": "64x48+0+0", "RAYCAST_PATTERN": ""},
                      {}),
                     ("format_short", {"RAYCAST_WINDOW": "64x48"}, {}),
                     ("format_sep", {"RAYCAST_WINDOW": "64x48x8+4"}, {}),
                     ("format_tail", {"RAYCAST_WINDOW": "64x48+8+4 "}, {}),
                     ("format_sign", {"RAYCAST_WINDOW": "64x48+-8+4"}, {}),
                     ("format_int", {"RAYCAST_WINDOW": "2147483648x48+8+4"}, {}),
                     ("format_empty", {"RAYCAST_WINDOW": ""}, {}),
                     ("parity", {"RAYCAST_WINDOW": "64x48+8+4"}, dict(mode="parity")),
                     ("adaptive", {"RAYCAST_WINDOW": "64x48+8+4"}, dict(ssaa=4, adaptive=16)),
                     ("pattern", {"RAYCAST_WINDOW": "64x48+8+4", "RAYCAST_PATTERN": "rgss4"}, {}),
                     ("tent", {"RAYCAST_WINDOW": "64x48+8+4", "RAYCAST_FILTER": "tent"},
                      dict(ssaa=2)),
                     ("gpus2", {"RAYCAST_WINDOW": "64x48+8+4"}, dict(gpus=2)),
                     ("outside", {"RAYCAST_WINDOW": "64x48+60+4"}, {}),
                     ("zero_image", {"RAYCAST_WINDOW": "0x48+0+0"}, {}),
                     ("past_int", {"RAYCAST_WINDOW": "1073741824x48+0+0"}, dict(ssaa=4)),
                     ("two_format_parity", {"RAYCAST_WINDOW": "64x48"}, dict(mode="parity")),
                     ("two_parity_adaptive", {"RAYCAST_WINDOW": "64x48+8+4"},
                      dict(mode="parity", ssaa=4, adaptive=16)),
                     ("two_adaptive_pattern",
                      {"RAYCAST_WINDOW": "64x48+8+4", "RAYCAST_PATTERN": "x"},
                      dict(ssaa=4, adaptive=16)),
                     ("two_pattern_tent",
                      {"RAYCAST_WINDOW": "64x48+8+4", "RAYCAST_PATTERN": "rgss4",
                                           "RAYCAST_FILTER": "tent"}, {}),
                     ("two_tent_gpus2", {"RAYCAST_WINDOW": "64x48+8+4", "RAYCAST_FILTER": "tent"},
                      dict(gpus=2)),
                     ("two_gpus2_outside", {"RAYCAST_WINDOW": "64x48+60+4"}, dict(gpus=2))):
    env_case(tag, env, "window_from_env", width=16, height=16, **kw)

assert len({c[0] for c in ENV}) == len(ENV), "duplicate case ids"


# ------------------------------------------------------------------ running them --
def captured(fn):
    """fn()'s result and what the process wrote to file descriptor 2 meanwhile (the library's
    fprintf(stderr) is unbuffered)."""
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            result = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return result, tmp.read().decode()


def run_refusal(export, args):
    args = [scene() if a is S else a for a in args]
    code, err = captured(lambda: getattr(rc.hip_lib(), export)(*args))
    return {"rc": code, "stderr": err}


def run_env(env, fn, kw, setenv, delenv):
    """setenv(name, value) and delenv(name) change the process environment (monkeypatch's in the
    test, os.environ's in the recorder)."""
    for name in ENV_NAMES:
        delenv(name)
    for name, value in env.items():
        setenv(name, value)
    taken, err = captured(lambda: getattr(rc, fn)(**kw))
    for name in env:
        delenv(name)
    return {"taken": json.loads(json.dumps(taken)), "stderr": err}


def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("cid,export,args", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusal(cid, export, args):
    got = run_refusal(export, args)
    assert got["rc"] == -1
    assert got == golden()["refusals"][cid]


@pytest.mark.parametrize("cid,env,fn,kw", ENV, ids=[c[0] for c in ENV])
def test_env(cid, env, fn, kw, monkeypatch):
    got = run_env(env, fn, kw, monkeypatch.setenv,
                  lambda name: monkeypatch.delenv(name, raising=False))
    assert got == golden()["env"][cid]


def test_golden_has_no_stale_case():
    g = golden()
    assert sorted(g["refusals"]) == sorted(c[0] for c in REFUSALS)
    assert sorted(g["env"]) == sorted(c[0] for c in ENV)
    assert _PIX.sum() == 0     # no refused call wrote the pixmap
