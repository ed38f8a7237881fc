"""Scrolling an accumulated view without a GPU (rc_accum_scroll_device): the numpy contract
against states built from scratch on the oracle's image, every refusal of the entry point pinned
byte for byte, and the layout: the ctypes argument list against the header and the exposed set's
index mapping (rc_sample_kernels.hip, scroll_rects and exposed_pixel) restated in Python.

The pan (-60, 30) of the 40 x 24 window cannot come from a window inside the 97 x 61 image (the
origin moves by at most 57 columns), and the old window is no argument of the call: nothing is
kept, so what the source was built through does not matter.  That case's new window is the pan
of (5, 3) clamped into the image, (0, 33); every other case's is the pan itself."""
import ctypes
import os
import re
import tempfile

import numpy as np
import pytest

from helpers import ROOT, oracle_render, oracle_render_cuda, rc, scene_path

FULL = (97, 61)
W, H = 40, 24
ORIGIN = (5, 3)
DEPTH = 6
PANS = [(12, 6), (-5, 0), (0, -3), (-4, 5), (0, 0), (40, 0), (-60, 30)]
CASES = [("simple", "fast"), ("reflection", "fast"), ("quadric", "fast"), ("quadric", "cuda")]


def exposed_count(w, h, dx, dy):
    return w * h - max(0, w - abs(dx)) * max(0, h - abs(dy))


def new_window(dx, dy):
    """The window after the pan, clamped into the image (a clamp only for (-60, 30))."""
    x0 = min(max(ORIGIN[0] + dx, 0), FULL[0] - W)
    y0 = min(max(ORIGIN[1] + dy, 0), FULL[1] - H)
    return (*FULL, x0, y0)


def from_scratch(big, g, pts, window, w, h, upto):
    """A reset pass [0, 1) and a pass [1, upto) through `window`, on the oracle's image."""
    crop = rc.window_crop(big, g, window, w, h)
    acc, out = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8)
    acc, out, _, _ = rc.accum_step(acc, out, crop, g, pts[:1], 0, reset=True)
    if upto > 1:
        acc, out, _, _ = rc.accum_step(acc, out, crop, g, pts[1:upto], 0)
    return acc, out


# ------------------------------------------------------------ 1. the model against the oracle --
@pytest.mark.parametrize("scene,mode", CASES, ids=[f"{s}-{m}" for s, m in CASES])
def test_model_equals_from_scratch(scene, mode):
    sc = rc.Scene.from_file(scene_path(scene))
    g, pts = rc.SAMPLE_SEQS["hier4"]
    if mode == "cuda":
        big = oracle_render_cuda(sc, g * FULL[0], g * FULL[1], DEPTH)
    else:
        big, stats = oracle_render(sc, g * FULL[0], g * FULL[1], DEPTH, mode)
        assert stats["parity_defined"] == 1
    big.setflags(write=False)
    acc_a, out_a = from_scratch(big, g, pts, (*FULL, *ORIGIN), W, H, 5)
    assert (acc_a[:, :, 3] == 5).all()
    acc_a.setflags(write=False)
    out_a.setflags(write=False)
    for dx, dy in PANS:
        win = new_window(dx, dy)
        if (dx, dy) != (-60, 30):
            assert win == rc.window_pan((*FULL, *ORIGIN), dx, dy)
        want_acc, want_out = from_scratch(big, g, pts, win, W, H, 5)
        acc, out, exposed = rc.accum_scroll(acc_a, out_a, rc.window_crop(big, g, win, W, H), g,
                                            pts[:5], dx, dy)
        tag = f"{scene} {mode} pan ({dx}, {dy})"
        np.testing.assert_array_equal(acc, want_acc, err_msg=tag)
        np.testing.assert_array_equal(out, want_out, err_msg=tag)
        assert exposed == exposed_count(W, H, dx, dy), tag
        if (dx, dy) == (12, 6) and scene == "quadric":
            # a condition on the input, not a tolerance: the exposed L looks at more than one colour
            kx, ky, kw, kh = rc.scroll_kept(W, H, dx, dy)
            mask = np.ones((H, W), bool)
            mask[ky:ky + kh, kx:kx + kw] = False
            assert mask.sum() == exposed
            assert len(np.unique(want_out[mask], axis=0)) >= 2
    # the kept part of a state with another history is moved as it is: n = 0 and n = 9 records
    odd = np.array(acc_a)
    odd[::2, :, 3] = 0
    odd[1::2, :, 3] = 9
    win = new_window(12, 6)
    acc, out, _ = rc.accum_scroll(odd, out_a, rc.window_crop(big, g, win, W, H), g, pts[:3], 12, 6)
    np.testing.assert_array_equal(acc[:H - 6, :W - 12], odd[6:, 12:])
    assert (acc[H - 6:, :, 3] == 3).all() and (acc[:, W - 12:, 3] == 3).all()


def test_model_takes_64_samples_in_chunks():
    """count = 64 of hier8: the exposed pixels are the box filter of the 8 x 8 subsamples."""
    rng = np.random.default_rng(18)
    g, pts = rc.SAMPLE_SEQS["hier8"]
    w, h = 5, 4
    big = rng.integers(0, 256, size=(g * h, g * w, 3), dtype=np.uint8)
    acc0 = rng.integers(0, 200, size=(h, w, 4)).astype(np.uint16)
    out0 = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    acc, out, exposed = rc.accum_scroll(acc0, out0, big, g, pts, 2, -1)
    assert exposed == exposed_count(w, h, 2, -1) == 20 - 9
    np.testing.assert_array_equal(acc[1:, :3], acc0[:3, 2:])
    np.testing.assert_array_equal(out[1:, :3], out0[:3, 2:])
    box = rc.box_downsample(big, g)
    np.testing.assert_array_equal(out[0], box[0])
    np.testing.assert_array_equal(out[:, 3:], box[:, 3:])
    assert (acc[0, :, 3] == 64).all() and (acc[:, 3:, 3] == 64).all()
    with pytest.raises(ValueError):
        rc.accum_scroll(acc0, out0, big, g, [], 1, 0)
    with pytest.raises(ValueError):
        rc.accum_scroll(acc0, out0[:, :4], big, g, pts[:2], 1, 0)


# ---------------------------------------------------------------------------- 2. refusals --
ACC_A, ACC_B = 1 << 20, 2 << 20      # "device pointers" a refused call never follows; an 8 x 8
OUT_A, OUT_B = 3 << 20, 4 << 20      # state is 512 bytes of records and 192 bytes of image
ODD = 4100
_scene = None
WHO = "rc_accum_scroll_device"


def packed_scene():
    global _scene
    if _scene is None:
        _scene = rc.Scene.from_file(scene_path("simple"))
    return _scene.packed()


def captured(fn):
    """fn()'s result and what the process wrote to file descriptor 2 meanwhile."""
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


def seq_of(g, pts):
    s = rc.RcSampleSeq()
    s.grid, s.nsamples = g, len(pts)
    for k, (x, y) in enumerate(pts):
        s.x[k], s.y[k] = x, y
    return s


def win_of(fw, fh, x0, y0):
    w = rc.RcWindow()
    w.full_w, w.full_h, w.x0, w.y0 = fw, fh, x0, y0
    return w


def scroll_args(**kw):
    a = dict(scene="scene", win=win_of(64, 48, 8, 4), w=8, h=8, opt=rc.options(6, "fast"),
             seq=seq_of(*rc.PATTERNS["rgss4"]), count=2, dx=3, dy=-2, acc_src=ACC_A, out_src=OUT_A,
             acc_dst=ACC_B, out_dst=OUT_B)
    a.update(kw)
    ref = lambda x: None if x is None else ctypes.byref(x)   # noqa: E731
    return (packed_scene() if a["scene"] == "scene" else a["scene"], ref(a["win"]), a["w"], a["h"],
            ref(a["opt"]), ref(a["seq"]), a["count"], a["dx"], a["dy"], a["acc_src"], a["out_src"],
            a["acc_dst"], a["out_dst"], None, None)


NULL = f"Error: {WHO}: a null pointer\n"
ALIGN = f"Error: {WHO}: an accumulator is not 8-byte aligned\n"
PARITY = (f"Error: {WHO}: accumulated samples are for fast and cuda mode: every pixel of a parity "
          "image depends on the scan-order carry of the whole image, so it cannot be shot sparsely; "
          "use plain ssaa\n")
ACC_OVERLAP = (f"Error: {WHO}: the source and the destination accumulators overlap: a kept record "
               "moves from one state to the other, keep two states and swap them\n")
OUT_OVERLAP = (f"Error: {WHO}: the source and the destination images overlap: a kept pixel moves "
               "from one state to the other, keep two states and swap them\n")
REFUSALS = {
    "null_scene": (dict(scene=None), NULL),
    "null_window": (dict(win=None), NULL),
    "null_opt": (dict(opt=None), NULL),
    "null_seq": (dict(seq=None), NULL),
    "null_acc_src": (dict(acc_src=None), NULL),
    "null_out_src": (dict(out_src=None), NULL),
    "null_acc_dst": (dict(acc_dst=None), NULL),
    "null_out_dst": (dict(out_dst=None), NULL),
    "odd_acc_src": (dict(acc_src=ODD), ALIGN),
    "odd_acc_dst": (dict(acc_dst=ODD), ALIGN),
    "count0": (dict(count=0),
               f"Error: {WHO}: count 0 is not 1..4 (the sequence's length)\n"),
    "count5": (dict(count=5),
               f"Error: {WHO}: count 5 is not 1..4 (the sequence's length)\n"),
    "parity": (dict(opt=rc.options(6, "parity")), PARITY),
    "ssaa2": (dict(opt=rc.options(6, "fast", ssaa=2)),
              f"Error: {WHO}: ssaa 2 in the options: the sample sequence carries the grid, leave "
              "ssaa at 0 or 1\n"),
    "gpus2": (dict(opt=rc.options(6, "fast", gpus=2)),
              f"Error: {WHO}: num_gpus 2: the row shards take no accumulator\n"),
    "bad_seq": (dict(seq=seq_of(3, [(0, 0), (1, 1)])),
                "Error: rc_sample_seq_check: grid 3 is not 2, 4 or 8\n"),
    "window_outside": (dict(win=win_of(64, 48, 60, 0)),
                       "Error: rc_window_check: a 8 x 8 window at (60, 0) reaches outside the "
                       "64 x 48 image\n"),
    "pixels_2^32": (dict(w=1 << 16, h=1 << 16, win=win_of(1 << 20, 1 << 20, 0, 0)),
                    f"Error: {WHO}: 65536 x 65536 is too large to scroll (32-bit pixel indices)\n"),
    "acc_same": (dict(acc_dst=ACC_A), ACC_OVERLAP),
    "acc_partial": (dict(acc_dst=ACC_A + 504), ACC_OVERLAP),
    "acc_partial_before": (dict(acc_dst=ACC_A - 8), ACC_OVERLAP),
    "out_same": (dict(out_dst=OUT_A), OUT_OVERLAP),
    "out_partial": (dict(out_dst=OUT_A - 100), OUT_OVERLAP),
    # two rules broken at once: the clause order of the header's list
    "two_null_odd": (dict(seq=None, acc_src=ODD), NULL),
    "two_odd_parity": (dict(acc_dst=ODD, opt=rc.options(6, "parity")), ALIGN),
    "two_parity_window": (dict(opt=rc.options(6, "parity"), win=win_of(64, 48, 60, 0)), PARITY),
    "two_window_count": (dict(win=win_of(64, 48, 60, 0), count=0),
                         "Error: rc_window_check: a 8 x 8 window at (60, 0) reaches outside the "
                         "64 x 48 image\n"),
    "two_count_overlap": (dict(count=5, acc_dst=ACC_A),
                          f"Error: {WHO}: count 5 is not 1..4 (the sequence's length)\n"),
    "two_overlaps": (dict(acc_dst=ACC_A, out_dst=OUT_A), ACC_OVERLAP),
}


@pytest.mark.parametrize("tag", sorted(REFUSALS))
def test_refusal(tag):
    kw, message = REFUSALS[tag]
    args = scroll_args(**kw)
    code, err = captured(lambda: rc.hip_lib().rc_accum_scroll_device(*args))
    assert code == -1
    assert err == message


# ------------------------------------------------------------------------------ 3. layout --
def test_window_pan():
    assert rc.window_pan((97, 61, 5, 3), 12, 6) == (97, 61, 17, 9)
    assert rc.window_pan((97, 61, 5, 3), -5, -3) == (97, 61, 0, 0)
    assert rc.window_pan((97, 61, 5, 3), 0, 0) == (97, 61, 5, 3)
    assert rc.window_pan(np.array([97, 61, 5, 3]), np.int64(-2), 1) == (97, 61, 3, 4)
    assert all(type(v) is int for v in rc.window_pan(np.array([97, 61, 5, 3]), np.int64(-2), 1))


C_TO_CTYPES = {
    "const rc_scene *": ctypes.c_void_p, "const rc_window *": ctypes.POINTER(rc.RcWindow),
    "int": ctypes.c_int, "const rc_options *": ctypes.POINTER(rc.RcOptions),
    "const rc_sample_seq *": ctypes.POINTER(rc.RcSampleSeq),
    "const rc_accum_px *": ctypes.c_void_p, "rc_accum_px *": ctypes.c_void_p,
    "const uint8_t *": ctypes.c_void_p, "uint8_t *": ctypes.c_void_p, "void *": ctypes.c_void_p,
    "rc_timing *": ctypes.POINTER(rc.RcTiming),
}


def test_ctypes_arguments_match_the_header():
    with open(os.path.join(ROOT, "include", "raycast_hip.h")) as f:
        text = f.read()
    m = re.search(r"\nint rc_accum_scroll_device\(([^)]*)\);", text)
    assert m, "the header declares rc_accum_scroll_device"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    types = [p[:-len(n)].strip() for p, n in zip(params, names)]
    assert names == ["scene", "win", "width", "height", "opt", "seq", "count", "dx", "dy",
                     "d_acc_src", "d_out_src", "d_acc_dst", "d_out_dst", "stream", "timing"]
    fn = rc.hip_lib().rc_accum_scroll_device
    assert list(fn.argtypes) == [C_TO_CTYPES[t] for t in types]
    assert fn.restype is ctypes.c_int


def scroll_rects(w, h, dx, dy):
    """rc_sample_kernels.hip scroll_rects(): the kept rectangle and the four exposed rectangles (rows
    above, columns left, columns right, rows below) as (first, width, x, y), and their total."""
    ax, ay = abs(dx), abs(dy)
    kx = ky = kw = kh = 0
    if ax < w and ay < h:
        kw, kh = w - ax, h - ay
        kx, ky = (ax if dx < 0 else 0), (ay if dy < 0 else 0)
    right = kx + kw
    wd = [w, kx, w - right, w]
    ht = [ky, kh, kh, h - ky - kh]
    xs, ys = [0, 0, right, 0], [0, ky, ky, ky + kh]
    rects, total = [], 0
    for k in range(4):
        rects.append((total, max(wd[k], 1), xs[k], ys[k]))
        total += wd[k] * ht[k]
    return (kx, ky, kw, kh), rects, total, sum(1 for k in range(4) if wd[k] * ht[k])


def exposed_pixel(rects, e):
    """rc_sample_kernels.hip exposed_pixel(): the last rectangle whose first entry is at or below e."""
    first, width, x0, y0 = rects[0]
    for k in range(1, 4):
        if e >= rects[k][0]:
            first, width, x0, y0 = rects[k]
    i = e - first
    return x0 + i % width, y0 + i // width


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (33, 17), (64, 48), (3, 70)])
def test_exposed_entries_are_a_bijection_onto_the_complement_of_the_kept_rectangle(w, h):
    pans = {(0, 0), (1, 0), (0, 1), (-1, -1), (w - 1, h - 1), (-(w - 1), 0), (w, 0), (0, -h),
            (3, -2), (-2, 5), (5, 2), (-4, -1), (2 ** 31 - 1, 0), (0, -2 ** 31), (-2 ** 31, 2 ** 31 - 1)}
    for dx, dy in sorted(pans):
        (kx, ky, kw, kh), rects, total, nonempty = scroll_rects(w, h, dx, dy)
        assert (kx, ky, kw, kh) == rc.scroll_kept(w, h, dx, dy)
        assert total == exposed_count(w, h, dx, dy)
        assert nonempty <= (2 if kw else 1)
        ys, xs = np.mgrid[0:h, 0:w]
        kept = (xs + dx >= 0) & (xs + dx < w) & (ys + dy >= 0) & (ys + dy < h)   # the contract
        seen = np.zeros((h, w), np.int64)
        for e in range(total):
            x, y = exposed_pixel(rects, e)
            assert 0 <= x < w and 0 <= y < h, (w, h, dx, dy, e)
            seen[y, x] += 1
        np.testing.assert_array_equal(seen, (~kept).astype(np.int64), err_msg=str((w, h, dx, dy)))
