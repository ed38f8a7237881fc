"""Accumulation through a free camera without a GPU: the pass's contract in numpy
(rc.accum_add) held against rc.accum_step, the thin-lens helper's geometry, the Python-side
argument errors, every refusal of the two entries pinned byte for byte in
tests/golden/camera_accum_refusals.json (recorded by this file run as a script with --record), and
the conditions on the inputs of tests/test_gpu_camera_accum.py, from the oracle's side."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import camera_accum_cases as cac
import ray_cases as rcs
import view_cases as vc
from helpers import GOLDEN, oracle_render, rc, scene_path
from test_refusals import FAKE, GOODS, ODD, O, S, SEQ, WIN, ref, run_refusal

F32, F64 = np.float32, np.float64
GOLDEN_FILE = os.path.join(GOLDEN, "camera_accum_refusals.json")
NEW_EXPORTS = ["rc_accum_pass_camera_device", "rc_render_camera_accum"]


# ------------------------------------------------------------ accum_add and accum_step --
@pytest.fixture(scope="module")
def big():
    """The oracle's 4*33 x 4*17 fast-mode image of the quadric scene: the samples of a 33 x 17
    image on the lattice of 4."""
    img, _ = oracle_render(rc.Scene.from_file(scene_path("quadric")), 4 * 33, 4 * 17, cac.DEPTH,
                           "fast")
    img.setflags(write=False)
    return img


def slices(big, g, pts):
    return np.stack([big[y::g, x::g] for x, y in pts])


def same(a, b, tag):
    assert a[2:] == b[2:], tag
    np.testing.assert_array_equal(a[0], b[0], err_msg=f"acc {tag}")
    np.testing.assert_array_equal(a[1], b[1], err_msg=f"out {tag}")


def test_accum_add_is_accum_step_on_the_lattice_slices(big):
    g, pts = cac.G, cac.HIER4
    acc, out = np.zeros((17, 33, 4), np.uint16), np.full((17, 33, 3), 77, np.uint8)
    first = 0
    for upto in cac.PREFIXES:
        want = rc.accum_step(acc, out, big, g, pts[first:upto], 0, reset=first == 0)
        got = rc.accum_add(acc, out, slices(big, g, pts[first:upto]), 0, reset=first == 0)
        same(got, want, f"hier4[{first}..{upto})")
        assert got[0].dtype == np.uint16 and got[1].dtype == np.uint8
        acc, out, first = want[0], want[1], upto
    # a masked pass after a reset pass
    acc, out, _, _ = rc.accum_step(acc, out, big, g, pts[:1], 0, reset=True)
    want = rc.accum_step(acc, out, big, g, pts[1:4], 16)
    same(rc.accum_add(acc, out, slices(big, g, pts[1:4]), 16), want, "masked")
    assert 0 < want[2] < 33 * 17 and want[3] == 0
    # a saturating pass: n = 250 everywhere but one row, 16 more would pass 256 there
    acc = want[0].copy()
    acc[:, :, 3] = 250
    acc[5, :, 3] = 3
    out = want[1]
    want = rc.accum_step(acc, out, big, g, pts, 0)
    same(rc.accum_add(acc, out, slices(big, g, pts), 0), want, "saturating")
    assert want[3] == 33 * 16 and (want[0][5, :, 3] == 19).all() and (want[0][4, :, 3] == 250).all()


def test_accum_add_argument_errors(big):
    acc, out = np.zeros((17, 33, 4), np.uint16), np.zeros((17, 33, 3), np.uint8)
    ok = slices(big, 4, cac.HIER4[:2])
    for bad in (ok.astype(np.int32), ok[0], ok[:0], np.concatenate([ok] * 9), ok[:, :, :, :2]):
        with pytest.raises(ValueError):
            rc.accum_add(acc, out, bad)
    for kw in ({"t": 256}, {"t": -1}, {"t": 16, "reset": True}):
        with pytest.raises(ValueError):
            rc.accum_add(acc, out, ok, **kw)
    with pytest.raises(ValueError):
        rc.accum_add(acc[:5], out, ok)
    with pytest.raises(ValueError):
        rc.accum_add(acc, out[:, :5], ok)


# ------------------------------------------------------------------------------ thin_lens --
def test_thin_lens_rays_meet_on_the_focal_plane():
    """In float64: the ray of every pixel of a 16 x 12 grid through every one of 8 lens points on
    a disc meets the pinhole ray's point at depth `focus`, to 1e-5 relative (the float32 rounding
    of the matrix and the eye, 2^-24 an entry)."""
    eye, m, focus = (0.5, 0.25, 1.0), rc.view_euler(0.4, -0.5, 0.2), 8.0
    pts = cac.lens_points(8, 0.3)
    cams = rc.thin_lens(eye, m, focus, pts)
    assert len(cams) == 8
    xs, ys = np.meshgrid((np.arange(16) + 0.5) / 16 - 0.5, 0.5 - (np.arange(12) + 0.5) / 12)
    p = np.stack([xs.ravel(), ys.ravel(), -np.ones(xs.size)], axis=1)          # z = -1
    m64, e64 = m.astype(F64), np.asarray(eye, F64)
    target = e64 + focus * (p @ m64.T)             # the pinhole ray at depth focus
    for (le, lm), (lx, ly) in zip(cams, pts):
        assert le.dtype == F32 and lm.dtype == F32 and lm.shape == (3, 3)
        q = p @ lm.astype(F64).T                   # the lens camera's ray vectors, z' = -1 in its frame
        meet = le.astype(F64) + focus * q
        err = np.linalg.norm(meet - target, axis=1) / np.linalg.norm(target - e64, axis=1)
        assert err.max() <= 1e-5, (lx, ly, err.max())
        if lx or ly:                               # a lens point off the axis moves the eye
            assert np.linalg.norm(le.astype(F64) - e64) > 0.0


def test_thin_lens_centre_is_the_camera_bit_for_bit():
    eye, m = np.array([-0.0, 0.25, 1e-40], F32), rc.view_euler(0.4, -0.5, 0.2)
    (e, v), = rc.thin_lens(eye, m, 8.0, [(0.0, 0.0)])
    assert e.view(np.uint32).tolist() == eye.view(np.uint32).tolist()
    assert v.view(np.uint32).tolist() == m.view(np.uint32).tolist()
    e, v = rc.thin_lens((1, 2, 3), None, 2.0, [(0.5, 0.0)])[0]
    assert e.tolist() == [1.5, 2.0, 3.0] and v.tolist() == [[1, 0, 0.25], [0, 1, 0], [0, 0, 1]]
    for bad in ({"focus": 0.0}, {"focus": -1.0}, {"focus": np.inf}, {"lens_points": [1, 2, 3]},
                {"lens_points": []}):
        with pytest.raises(ValueError):
            rc.thin_lens(**{"eye": (0, 0, 0), "m": None, "focus": 8.0,
                            "lens_points": [(0.1, 0.2)], **bad})


# ------------------------------------------------------------------- exports and errors --
def test_exports_and_argument_errors():
    for name in NEW_EXPORTS:
        assert name in rc.HIP_EXPORTS and hasattr(rc.hip_lib(), name), name
    sc = vc.scene("simple")
    cam = ((0.5, 0.25, 1.0), None)
    for cams in ([cam, cam, cam], [], [cam] * 5):                    # count is 4
        with pytest.raises(ValueError):
            rc.accum_pass_camera_device(sc, cams, None, 8, 8, "hier4", 0, 4, FAKE, FAKE)
    for cams in ([cam] * 3, [cam] * 16):                             # hier2 has 4 samples
        with pytest.raises(ValueError):
            rc.render_camera_accum(sc, cams, 8, 8, "hier2")
    with pytest.raises(ValueError):                                  # an eye of two components
        rc.accum_pass_camera_device(sc, ((0, 0), None), None, 8, 8, "hier4", 0, 1, FAKE, FAKE)
    with pytest.raises(ValueError):
        rc.render_camera_accum(sc, [((0, 0, 0, 0), None)] * 4, 8, 8, "hier2")
    with pytest.raises(ValueError):                                  # a view of 16 entries
        rc.accum_pass_camera_device(sc, ((0, 0, 0), np.eye(4)), None, 8, 8, "hier4", 0, 1, FAKE,
                                    FAKE)
    with pytest.raises(ValueError):
        rc.render_camera_accum(sc, ((0, 0, 0), np.zeros(8)), 8, 8, "hier2")
    with pytest.raises(ValueError):
        rc.accum_pass_camera_device(sc, 7, None, 8, 8, "hier4", 0, 1, FAKE, FAKE)
    arr = rc._rc_cameras([cam, ((-0.0, 2.0, 3.0), vc.VIEWS["ypr"])], 2, "test")
    assert len(arr) == 2 and np.signbit(arr[1].eye[0])
    assert list(arr[1].view.m) == vc.VIEWS["ypr"].ravel().tolist()
    assert len(rc._rc_cameras(cam, 16, "test")) == 1


# ------------------------------------------------------------------------------ refusals --
def CAM(eye=(0.5, 0.25, 1.0), m=None):
    return rc._rc_camera(eye, m)


def CAMS(*cams):
    arr = (rc.RcCamera * len(cams))()
    for k, c in enumerate(cams):
        arr[k] = c
    return arr


def _bad_m(k, x):
    m = np.eye(3).ravel()
    m[k] = x
    return CAM(m=m)


HIER4 = SEQ(*rc.SAMPLE_SEQS["hier4"])
ONE = CAMS(CAM())
GOODW = WIN(64, 48, 8, 4)
_PIX = np.full((8, 8, 3), 0x5a, np.uint8)
PIX = _PIX.ctypes.data
CASES = []


def case(tag, export, *args):
    CASES.append((f"{export}[{tag}]", export, args))


def a_pass(tag, opt, cams=ONE, ncams=1, seq=GOODS, first=0, count=1, t=0, reset=0, w=8, h=8,
           acc=FAKE, out=FAKE, win=GOODW, sc=S):
    case(tag, "rc_accum_pass_camera_device", sc, cams, ncams, ref(win), w, h, ref(opt), ref(seq),
         first, count, t, reset, acc, out, None, None)


def host(tag, opt, cams=ONE, ncams=1, seq=GOODS, w=8, h=8, win=GOODW, sc=S, out=PIX):
    case(tag, "rc_render_camera_accum", sc, cams, ncams, ref(win), w, h, ref(opt), ref(seq), out,
         None)


def both(tag, opt, **kw):
    a_pass(tag, opt, **kw)
    host(tag, opt, **kw)


# 1. null pointers (the window may be null)
a_pass("null_scene", O(), sc=None)
a_pass("null_cams", O(), cams=None)
a_pass("null_opt", None)
a_pass("null_seq", O(), seq=None)
a_pass("null_acc", O(), acc=None)
a_pass("null_out", O(), out=None)
a_pass("two_null_odd", O(), seq=None, acc=ODD)
a_pass("two_null_cuda", O("cuda"), cams=None)
host("null_scene", O(), sc=None)
host("null_cams", O(), cams=None)
host("null_opt", None)
host("null_seq", O(), seq=None)
host("null_out", O(), out=None)
# 2. a misaligned accumulator
a_pass("odd_acc", O(), acc=ODD)
a_pass("two_odd_parity", O("parity"), acc=ODD)
# 3. what rc_accum_pass_window_device refuses, cuda mode right after num_gpus
for tag, opt in {"ssaa3": O(ssaa=3), "ssaa-1": O(ssaa=-1), "thr_no_factor": O(ssaa=1, adaptive=16),
                 "ssaa2": O(ssaa=2), "ssaa4_adaptive": O(ssaa=4, adaptive=16),
                 "parity": O("parity"), "gpus2": O(gpus=2), "cuda": O("cuda"),
                 "two_cuda_gpus2": O("cuda", gpus=2), "two_ssaa2_parity": O("parity", ssaa=2),
                 "two_parity_gpus2": O("parity", gpus=2)}.items():
    both(tag, opt)
both("two_cuda_seq", O("cuda"), seq=SEQ(3, [(0, 0)]))
for tag, (g, pts, n) in {"grid3": (3, [(0, 0), (1, 1)], None), "off_x": (2, [(0, 0), (2, 1)], None),
                         "duplicate": (4, [(1, 0), (3, 1), (1, 0), (2, 3)], None),
                         "n0": (4, [], None), "n17_g4": (4, [], 17)}.items():
    both(tag, O(), seq=SEQ(g, pts, n))
for tag, t in {"thr-1": -1, "thr256": 256}.items():
    a_pass(tag, O(), t=t)
for tag, (w, h, t) in {"w_past": ((1 << 26) + 1, 1, 0), "h_past": (1, (1 << 26) + 1, 0),
                       "w0": (0, 8, 0), "h_neg": (8, -1, 16),
                       "thr_pixels_2^32": (1 << 16, 1 << 16, 16),
                       "tile_rows": (1, 1 << 26, 0)}.items():
    a_pass(tag, O(), t=t, w=w, h=h, win=WIN(1 << 27, 1 << 27, 0, 0))
    if t == 0:
        host(tag, O(), w=w, h=h, win=WIN(1 << 27, 1 << 27, 0, 0))
both("no_window_w0", O(), w=0, win=None)
for tag, w in {"outside": WIN(64, 48, 60, 0), "past_int_g4": WIN(1 << 30, 48, 0, 0),
               "origin": WIN(64, 48, 0, -1)}.items():
    both("window_" + tag, O(), win=w)
a_pass("two_seq_thr", O(), seq=SEQ(3, [(0, 0)]), t=256)
a_pass("two_thr_size", O(), t=-1, w=0)
a_pass("two_window_count", O(), count=0, win=WIN(64, 48, 60, 0))
for tag, (first, count) in {"count0": (0, 0), "count17": (0, 17), "first_neg": (-1, 1),
                            "past_end": (3, 2), "first_end": (4, 1)}.items():
    a_pass(tag, O(), first=first, count=count)
a_pass("reset_thr", O(), t=16, reset=1)
a_pass("two_count_reset", O(), count=17, t=16, reset=1)
# 4. the number of cameras
PAIR = CAMS(CAM(), CAM((1.0, 2.0, 3.0)))
for tag, n in {"ncams0": 0, "ncams_neg": -1, "ncams2_count4": 2, "ncams5_count4": 5,
               "ncams16_count4": 16}.items():
    a_pass(tag, O(), cams=PAIR, ncams=n, count=4)
a_pass("two_count17_ncams3", O(), cams=PAIR, ncams=3, count=17)
a_pass("two_reset_thr_ncams3", O(), cams=PAIR, ncams=3, count=4, t=16, reset=1)
for tag, n in {"ncams0": 0, "ncams2_n4": 2, "ncams5_n4": 5}.items():
    host(tag, O(), cams=PAIR, ncams=n)
# 5. the first camera rc_camera_check refuses, by its index
both("eye_nan", O(), cams=CAMS(CAM((0, 0, np.nan))))
both("m_inf", O(), cams=CAMS(_bad_m(5, np.inf)))
a_pass("second_eye_inf", O(), cams=CAMS(CAM(), CAM((-np.inf, 0, 0))), ncams=2, count=2)
a_pass("third_m_nan_fourth_eye_nan", O(),
       cams=CAMS(CAM(), CAM(), _bad_m(2, np.nan), CAM((np.nan, 0, 0))), ncams=4, count=4)
a_pass("two_ncams_eye_nan", O(), cams=CAMS(CAM((np.nan, 0, 0)), CAM()), ncams=2, count=3)
a_pass("two_cuda_eye_nan", O("cuda"), cams=CAMS(CAM((np.nan, 0, 0))))
a_pass("two_outside_eye_nan", O(), cams=CAMS(CAM((np.nan, 0, 0))), win=WIN(64, 48, 60, 0))
_SIXTEEN = [CAM() for _ in range(16)]
_SIXTEEN[13] = _bad_m(8, -np.inf)
host("fourteenth_m_inf", O(), cams=CAMS(*_SIXTEEN), ncams=16, seq=HIER4)

assert len({c[0] for c in CASES}) == len(CASES), "duplicate case ids"


def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("cid,export,args", CASES, ids=[c[0] for c in CASES])
def test_refusal(cid, export, args):
    """-1 and one message, from the arguments alone: these run without a GPU, so no refusal can
    have touched a device, and the pre-filled host pixmap stays as it was."""
    got = run_refusal(export, args)
    assert got["rc"] == -1
    assert got["stderr"].startswith("Error: rc_") and got["stderr"].count("\n") == 1
    assert got == golden()[cid]
    assert (_PIX == 0x5a).all()


def test_golden_has_no_stale_case():
    assert sorted(golden()) == sorted(c[0] for c in CASES)


def test_the_refusals_order():
    """The documented order, on calls that break two rules: the earlier clause speaks."""
    g = golden()
    dev, hst = "rc_accum_pass_camera_device[%s]", "rc_render_camera_accum[%s]"
    assert "a null pointer" in g[dev % "two_null_odd"]["stderr"]
    assert "a null pointer" in g[dev % "two_null_cuda"]["stderr"]
    assert "not 8-byte aligned" in g[dev % "two_odd_parity"]["stderr"]
    assert "num_gpus 2" in g[dev % "two_cuda_gpus2"]["stderr"]
    assert "rays with an origin are for fast mode" in g[dev % "two_cuda_seq"]["stderr"]
    assert "rays with an origin are for fast mode" in g[hst % "two_cuda_seq"]["stderr"]
    assert "rays with an origin are for fast mode" in g[dev % "two_cuda_eye_nan"]["stderr"]
    assert g[dev % "two_window_count"]["stderr"].startswith("Error: rc_window_check: ")
    assert g[dev % "two_outside_eye_nan"]["stderr"].startswith("Error: rc_window_check: ")
    assert "a pass takes 1..16 samples" in g[dev % "two_count17_ncams3"]["stderr"]
    assert "reset with threshold" in g[dev % "two_reset_thr_ncams3"]["stderr"]
    assert "ncams 2 is not 1 or count (3)" in g[dev % "two_ncams_eye_nan"]["stderr"]
    assert "cams[1] fails rc_camera_check: eye[0]" in g[dev % "second_eye_inf"]["stderr"]
    assert "cams[2] fails rc_camera_check: view.m[2]" in g[
        dev % "third_m_nan_fourth_eye_nan"]["stderr"]
    assert "cams[13] fails rc_camera_check: view.m[8]" in g[hst % "fourteenth_m_inf"]["stderr"]


def test_the_window_accumulations_refusals_carry_over():
    """What rc_accum_pass_window_device refuses with a message of the accumulation family's, the
    camera entry refuses with the same words but for the entry's name."""
    with open(os.path.join(GOLDEN, "refusals.json")) as f:
        old = json.load(f)["refusals"]
    own = golden()
    for tag in ("ssaa3", "ssaa-1", "thr_no_factor", "ssaa2", "ssaa4_adaptive", "gpus2", "grid3",
                "off_x", "duplicate", "n0", "n17_g4", "thr-1", "thr256", "w_past", "h_past", "w0",
                "h_neg", "thr_pixels_2^32", "tile_rows", "window_outside", "window_past_int_g4",
                "window_origin", "count0", "count17", "first_neg", "reset_thr", "odd_acc",
                "null_scene"):
        a = old[f"rc_accum_pass_window_device[{tag}]"]["stderr"]
        b = own[f"rc_accum_pass_camera_device[{tag}]"]["stderr"]
        assert a.replace("rc_accum_pass_window_device", "rc_accum_pass_camera_device") == b, tag


# ------------------------------------------- the inputs of the GPU suite are not vacuous --
def test_the_gpu_suites_inputs_are_not_vacuous():
    # cap: every camera used on the GPU sees at least 30 % primary hits in the 64 x 48 frame
    # (ray_cases.CAMERAS guarantees it; tests/test_camera.py checks all of them)
    for name, eye, m in cac.DENSE + [cac.MASKED]:
        assert any(c is (name, eye, m) for c in rcs.CAMERAS) or any(
            c[0] == name and c[1] == eye and c[2] is m for c in rcs.CAMERAS)
        assert (rcs.camera_samples(name, eye, m)[2] >= 0).mean() >= 0.30, (name, eye)
    # cap: the masked pass's active set is neither empty nor everything, 0 < |M| < W * H
    active = cac.masked_pass()[4]
    assert 0 < active < cac.SIZE[0] * cac.SIZE[1], active
    # cap: through every lens camera j > 0 the sample plane differs from camera 0's, at the same
    # lattice point, in at least 1 % of the window's pixels: a kernel that always read cams[0]
    # would miss the expectation
    assert len(cac.LENS) == 16
    for j in range(1, 16):
        a = cac.plane(cac.LENS_SCENE, *cac.LENS[0], cac.HIER4[j])
        b = cac.plane(cac.LENS_SCENE, *cac.LENS[j], cac.HIER4[j])
        assert (a != b).any(axis=2).mean() >= 0.01, j
    # and the five cameras of the pass at first = 3 differ among themselves the same way
    for j in range(1, 5):
        a = cac.plane(cac.LENS_SCENE, *cac.LENS[0], cac.HIER4[3 + j])
        b = cac.plane(cac.LENS_SCENE, *cac.LENS[j], cac.HIER4[3 + j])
        assert (a != b).any(axis=2).mean() >= 0.01, j


if __name__ == "__main__":       # python tests/test_camera_accum.py --record
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_camera_accum.py --record   (writes " + GOLDEN_FILE + ")")
    with open(GOLDEN_FILE, "w") as f:
        json.dump({cid: run_refusal(export, args) for cid, export, args in CASES}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} refusals in {GOLDEN_FILE}", file=sys.stderr)
