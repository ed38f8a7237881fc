"""The G-buffer through a camera, the guided filter and the ambient compose without a GPU
(DESIGN.md §28): the contract's numpy side (rc.ao_filter, rc.ao_compose) on hand cases and against
a pixel-by-pixel restatement, the constructors and rc_ao_filter_check's clauses in order, every
refusal of the entries pinned byte for byte in tests/golden/guided_refusals.json (recorded by this
file run as a script with --record), and the conditions on the inputs of tests/test_gpu_guided.py,
from the oracle's side."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import guided_cases as gc
import ray_cases as rcs
from helpers import GOLDEN, rc
from test_refusals import FAKE, O, S, WIN, ref, run_refusal

F32, I32 = np.float32, np.int32
INF, NAN = np.inf, np.nan
GOLDEN_FILE = os.path.join(GOLDEN, "guided_refusals.json")
NEW_EXPORTS = ["rc_render_camera_gbuffer", "rc_render_camera_gbuffer_device", "rc_ao_filter_box",
               "rc_ao_filter_tent", "rc_ao_filter_check", "rc_ao_filter_device",
               "rc_ao_compose_device", "rc_render_ambient"]


def state(open_, rays):
    acc = np.zeros(np.shape(open_), rc.AO_DTYPE)
    acc["open"], acc["rays"] = open_, rays
    return acc


def flat_guide(h, w, ident=0):
    """One surface: a plane z = -5 seen head on."""
    ids = np.full((h, w), ident, I32)
    P = np.zeros((h, w, 3), F32)
    P[..., 0], P[..., 1], P[..., 2] = np.arange(w)[None, :], np.arange(h)[:, None], -5.0
    N = np.zeros((h, w, 3), F32)
    N[..., 2] = 1.0
    return ids, P, N


# ------------------------------------------------------------- rc.ao_filter: hand cases --
def test_radius_0_is_the_plain_byte():
    rng = np.random.default_rng(1)
    rays = rng.integers(0, 400, (5, 7))
    acc = state((rays * rng.random((5, 7))).astype(int), rays)
    ids, P, N = flat_guide(5, 7)
    for taps in ("box", "tent", [9]):
        got = rc.ao_filter(acc, ids, P, N, rc.ao_filter_params(0, taps))
        np.testing.assert_array_equal(got, rc.ao_byte(acc))


def test_a_lone_pixel_keeps_its_own_byte():
    """A pixel whose id no neighbour shares, and a miss among hits."""
    acc = state(np.full((5, 5), 4), np.full((5, 5), 16))
    acc["open"][2, 2], acc["open"][0, 0] = 13, 9
    ids, P, N = flat_guide(5, 5)
    ids[2, 2], ids[0, 0] = 7, -1
    got = rc.ao_filter(acc, ids, P, N, rc.ao_filter_params(2, "box"))
    plain = rc.ao_byte(acc)
    assert got[2, 2] == plain[2, 2] == (510 * 13 + 16) // 32
    assert got[0, 0] == plain[0, 0]
    # the lone pixel and the miss are pooled into nothing: the others see 4 of 16 everywhere
    others = np.ones((5, 5), bool)
    others[2, 2] = others[0, 0] = False
    assert (got[others] == (510 * 4 + 16) // 32).all()


def test_a_nan_normal_is_rejected_and_keeps_its_centre():
    acc = state(np.full((3, 3), 8), np.full((3, 3), 16))
    acc["open"][1, 1] = 16
    ids, P, N = flat_guide(3, 3)
    N[1, 1] = (NAN, 0.0, 1.0)
    got = rc.ao_filter(acc, ids, P, N, rc.ao_filter_params(1, "box", -INF, INF))
    assert got[1, 1] == 255                      # nothing but itself: every nd is NaN
    assert (got[np.arange(3) != 1][:, np.arange(3) != 1] == 128).all()   # the corners skip it
    # a NaN in P rejects through pd, an inf through inf - inf
    ids, P, N = flat_guide(3, 3)
    P[1, 1, 0] = INF
    got = rc.ao_filter(acc, ids, P, N, rc.ao_filter_params(1, "box", -INF, INF))
    assert got[1, 1] == 255 and got[0, 0] == 128


def test_no_rays_anywhere_gives_255():
    ids, P, N = flat_guide(4, 6)
    acc = state(np.zeros((4, 6), int), np.zeros((4, 6), int))
    got = rc.ao_filter(acc, ids, P, N, rc.ao_filter_params(3, "tent"))
    assert (got == 255).all()
    # a pixel without rays takes its accepted neighbours' estimate
    acc["rays"][1, 2], acc["open"][1, 2] = 16, 4
    got = rc.ao_filter(acc, ids, P, N, rc.ao_filter_params(1, "box"))
    assert got[1, 1] == got[1, 2] == (510 * 4 + 16) // 32 and got[3, 5] == 255


def test_the_1x1_image_and_a_3x3_image_at_radius_8():
    ids, P, N = flat_guide(1, 1)
    acc = state([[5]], [[16]])
    for r in (0, 1, 8):
        assert rc.ao_filter(acc, ids, P, N, rc.ao_filter_params(r, "tent"))[0, 0] == \
            (510 * 5 + 16) // 32
    ids, P, N = flat_guide(3, 3)
    rng = np.random.default_rng(3)
    acc = state(rng.integers(0, 17, (3, 3)), np.full((3, 3), 16))
    f = rc.ao_filter_params(8, "box", -INF, INF)
    got = rc.ao_filter(acc, ids, P, N, f)
    total = int(acc["open"].sum())
    assert (got == (510 * total + 144) // 288).all()     # every pixel pools all nine
    np.testing.assert_array_equal(got, gc.filter_pixel_by_pixel(acc, ids, P, N, f))


def test_the_thresholds():
    """dplane cuts a step in depth, nmin a crease; both are inclusive."""
    ids, P, N = flat_guide(1, 4)
    P[0, 2:, 2] = -5.5                                   # a step of 0.5 along the normal
    acc = state([[0, 0, 16, 16]], [[16, 16, 16, 16]])
    cut = rc.ao_filter(acc, ids, P, N, rc.ao_filter_params(3, "box", 0.9, 0.25))
    np.testing.assert_array_equal(cut, [[0, 0, 255, 255]])
    edge = rc.ao_filter(acc, ids, P, N, rc.ao_filter_params(3, "box", 0.9, 0.5))
    np.testing.assert_array_equal(edge, [[128, 128, 128, 128]])
    ids, P, N = flat_guide(1, 4)
    N[0, 2:] = (0.6, 0.0, 0.8)                           # nd = 0.8 across the crease
    P[..., 0] = 0.0                                      # pd = 0 whichever normal
    crease = rc.ao_filter(acc, ids, P, N, rc.ao_filter_params(3, "box", 0.9, 0.05))
    np.testing.assert_array_equal(crease, [[0, 0, 255, 255]])
    at = rc.ao_filter(acc, ids, P, N, rc.ao_filter_params(3, "box", float(F32(0.8)), 0.05))
    np.testing.assert_array_equal(at, [[128, 128, 128, 128]])
    nothing = rc.ao_filter(acc, ids, P, N, rc.ao_filter_params(3, "box", 2.0, 0.05))
    np.testing.assert_array_equal(nothing, rc.ao_byte(acc))


def test_the_vectorised_rule_is_the_pixel_by_pixel_rule():
    name, eye, m = rcs.CAMERAS[9]
    g = gc.planes(name, eye, m)
    acc = gc.state(name, eye, m, [rc.ao_dirs(5)])
    for f in (rc.ao_filter_params(1, [2, 1]), rc.ao_filter_params(3, [6, 4, 2, 1], 0.5, 0.2),
              rc.ao_filter_params(8, "tent", -INF, INF)):
        np.testing.assert_array_equal(rc.ao_filter(acc, g["id"], g["P"], g["N"], f),
                                      gc.filter_pixel_by_pixel(acc, g["id"], g["P"], g["N"], f))


def test_the_weight_cap_at_its_edge():
    edge = rc.ao_filter_params(8, [21] + [10] * 8)
    assert (21 + 2 * 80) ** 2 == 32761 and rc.ao_filter_check(edge)
    assert not rc.ao_filter_check(rc.ao_filter_params(8, [22] + [10] * 8))
    # at the edge the sums reach 32761 * 65535 < 2^31
    ids, P, N = flat_guide(17, 17)
    acc = state(np.full((17, 17), 65535), np.full((17, 17), 65535))
    got = rc.ao_filter(acc, ids, P, N, edge)
    assert (got == 255).all() and 32761 * 65535 < 2 ** 31


# ------------------------------------------------------------------------- rc.ao_compose --
def test_ao_compose_hand_cases():
    table = np.array([[10, 200, 255], [0, 1, 3]], np.uint8)
    rgb = np.array([[[0, 100, 250], [5, 5, 5], [7, 8, 9], [1, 2, 3], [4, 5, 6]]], np.uint8)
    ids = np.array([[0, 1, -1, 2, np.iinfo(I32).max]], I32)
    ao = np.array([[255, 128, 255, 255, 255]], np.uint8)
    got = rc.ao_compose(rgb, ids, ao, table)
    # saturation at 255; ao = 255 adds the table's entry itself
    np.testing.assert_array_equal(got[0, 0], [10, 255, 255])
    # the rounding: (1 * 128 + 127) // 255 = 1 (128/255 rounds up), (3 * 128 + 127) // 255 = 2
    np.testing.assert_array_equal(got[0, 1], [5, 6, 7])
    # ids outside [0, n) leave the pixel
    np.testing.assert_array_equal(got[0, 2:], rgb[0, 2:])
    # the tie: a * ao = 127.5 * 255 does not exist in integers; (a * ao + 127) // 255 rounds
    # 0.498 down and 0.502 up
    tie = rc.ao_compose(np.zeros((1, 2, 3), np.uint8), np.zeros((1, 2), I32),
                        np.array([[127, 128]], np.uint8), np.array([[1, 1, 1]], np.uint8))
    np.testing.assert_array_equal(tie[0, :, 0], [0, 1])
    assert (rc.ao_compose(rgb, ids, np.zeros_like(ao), table) == rgb).all()
    with pytest.raises(ValueError):
        rc.ao_compose(rgb, ids[:, :4], ao, table)


def test_the_shape_table_is_the_oracles_quant():
    sc = rcs.scene("quadric")
    d = gc.diffuse_colors(sc.js)
    assert d.shape == (sc.num_shapes, 3) and (d > 0).any()
    np.testing.assert_array_equal(gc.shape_table(sc.js, (0.0, 0.0, 0.0)), 0)
    one = gc.shape_table(sc.js, (1.0, 1.0, 1.0))
    np.testing.assert_array_equal(one, np.clip(np.floor(d * F32(255.0)), 0, 255).astype(np.uint8))
    assert (gc.shape_table(sc.js, (4.0, 4.0, 4.0))[d > 0.25] == 255).all()


# -------------------------------------------------------- constructors, check, exports --
def test_the_constructors():
    for r in range(9):
        box, tent = rc.ao_filter_params(r, "box"), rc.ao_filter_params(r, "tent")
        for f, want in ((box, [1] * (r + 1)), (tent, [r + 1 - d for d in range(r + 1)])):
            assert f.radius == r and f.pad == 0 and list(f.taps)[:r + 1] == want
            assert list(f.taps)[r + 1:] == [0] * (8 - r)
            assert f.nmin == F32(0.9) and f.dplane == F32(0.05) and rc.ao_filter_check(f)
    lib = rc.hip_lib()
    f = rc.RcAoFilter()
    for make in (lib.rc_ao_filter_box, lib.rc_ao_filter_tent):
        assert make(9, ctypes.byref(f)) == -1 and make(-1, ctypes.byref(f)) == -1
        assert make(3, None) == -1
    with pytest.raises(ValueError):
        rc.ao_filter_params(9)
    with pytest.raises(ValueError):
        rc.ao_filter_params(2, [1, 2])
    with pytest.raises(ValueError):
        rc.ao_filter_params(1, "gauss")


def test_the_exports_and_the_layout():
    for name in NEW_EXPORTS:
        assert name in rc.HIP_EXPORTS and hasattr(rc.hip_lib(), name), name
    F = rc.RcAoFilter
    assert ctypes.sizeof(F) == 32
    assert (F.radius.offset, F.nmin.offset, F.dplane.offset, F.taps.offset, F.pad.offset) == \
        (0, 4, 8, 12, 30)


def test_extreme_thresholds_pass_the_check():
    assert rc.ao_filter_check(rc.ao_filter_params(8, "box", -INF, INF))
    assert rc.ao_filter_check(rc.ao_filter_params(3, "tent", 2.0, 0.0))
    assert rc.ao_filter_check(rc.ao_filter_params(3, [1, 0, 0, 0], INF, 0.05))


# ------------------------------------------------------------------------------ refusals --
ODD4 = 4098      # a non-null "device pointer" that is not 4-byte aligned


def CAM(eye=(0.5, 0.25, 1.0), m=None):
    return rc._rc_camera(eye, m)


def FILT(radius=2, taps="tent", nmin=0.9, dplane=0.05, pad=0, count=None):
    f = rc.ao_filter_params(radius, taps, nmin, dplane)
    f.pad = pad
    if count is not None:
        f.radius = count
    return f


def PLANES(id_=FAKE, t=FAKE, P=FAKE, N=FAKE):
    return rc.RcGbuffer(id_, t, P, N)


def AMB(*c):
    return (ctypes.c_float * 3)(*c)


def DIRS(n=4, tmax=INF, count=None):
    d = rc._rc_ao_dirs(rc.ao_dirs(n, tmax), "test")
    if count is not None:
        d.n = count
    return d


def SETS(*ds):
    arr = (rc.RcAoDirs * len(ds))()
    for k, d in enumerate(ds):
        arr[k] = d
    return arr


GOODW = WIN(64, 48, 8, 4)
GOODF = FILT()
GOODA = AMB(0.2, 0.3, 0.4)
ONE = SETS(DIRS())
_PIX = np.full((8, 8, 3), 0x5a, np.uint8)
PIX = _PIX.ctypes.data
_PL = [np.full(8 * 8 * 3 * 4, 0x5a, np.uint8) for _ in range(4)]    # room for a float plane
HOSTG = rc.RcGbuffer(*[a.ctypes.data for a in _PL])
CASES = []


def case(tag, export, *args):
    CASES.append((f"{export}[{tag}]", export, args))


def gbuf(tag, opt, cam=CAM(), w=8, h=8, win=GOODW, planes=True, sc=S):
    """both forms of the camera G-buffer"""
    dev = PLANES() if planes is True else planes
    hst = HOSTG if planes is True else planes
    case(tag, "rc_render_camera_gbuffer", sc, ref(cam), ref(win), w, h, ref(opt), ref(hst), None)
    case(tag, "rc_render_camera_gbuffer_device", sc, ref(cam), ref(win), w, h, ref(opt), ref(dev),
         None, None)


def filt(tag, ao=FAKE, guide=PLANES(), w=8, h=8, f=GOODF, out=FAKE):
    case(tag, "rc_ao_filter_device", ao, ref(guide), w, h, ref(f), out, None)


def comp(tag, opt, ids=FAKE, ao=FAKE, amb=GOODA, rin=FAKE, rout=FAKE, w=8, h=8, sc=S):
    case(tag, "rc_ao_compose_device", sc, ref(opt), ids, ao, amb, rin, rout, w, h, None)


def host(tag, opt, cam=CAM(), sets_=ONE, nsets=1, f=GOODF, amb=GOODA, w=8, h=8, win=GOODW,
         out=PIX, sc=S):
    case(tag, "rc_render_ambient", sc, ref(cam), ref(win), w, h, ref(opt), sets_, nsets, ref(f),
         amb, out, None)


# the camera G-buffer: 1. null pointers
gbuf("null_scene", O(), sc=None)
gbuf("null_cam", O(), cam=None)
gbuf("null_opt", None)
gbuf("null_planes", O(), planes=None)
gbuf("two_null_cuda", O("cuda"), cam=None)
# 2. all four planes null
gbuf("no_plane", O(), planes=PLANES(None, None, None, None))
gbuf("two_no_plane_parity", O("parity"), planes=PLANES(None, None, None, None))
# 3. the camera family's mode clauses, then the window
for tag, opt in {"parity": O("parity"), "gpus2": O(gpus=2), "cuda": O("cuda"),
                 "two_cuda_gpus2": O("cuda", gpus=2), "two_parity_gpus2": O("parity", gpus=2),
                 "two_parity_ssaa2": O("parity", ssaa=2), "two_cuda_ssaa2": O("cuda", ssaa=2)}.items():
    gbuf(tag, opt)
    host(tag, opt)
    comp(tag, opt)
for tag, (w, h, win) in {"w0": (0, 8, GOODW), "h_neg": (8, -1, GOODW), "no_window_w0": (0, 8, None),
                         "window_outside": (8, 8, WIN(64, 48, 60, 0)),
                         "window_origin": (8, 8, WIN(64, 48, 0, -1))}.items():
    gbuf(tag, O(), w=w, h=h, win=win)
    host(tag, O(), w=w, h=h, win=win)
gbuf("two_cuda_window", O("cuda"), win=WIN(64, 48, 60, 0))
gbuf("two_window_ssaa2", O(ssaa=2), win=WIN(64, 48, 60, 0))
gbuf("two_window_eye_nan", O(), win=WIN(64, 48, 60, 0), cam=CAM((NAN, 0, 0)))
# 4. ssaa
for tag, opt in {"ssaa2": O(ssaa=2), "ssaa3": O(ssaa=3), "ssaa-1": O(ssaa=-1),
                 "ssaa4_adaptive": O(ssaa=4, adaptive=16),
                 "thr_no_factor": O(ssaa=1, adaptive=16)}.items():
    gbuf(tag, opt)
    host(tag, opt)
gbuf("two_ssaa2_eye_nan", O(ssaa=2), cam=CAM((NAN, 0, 0)))
# 5. the camera
gbuf("eye_nan", O(), cam=CAM((0, 0, NAN)))
gbuf("eye_inf", O(), cam=CAM((-INF, 0, 0)))
host("eye_nan", O(), cam=CAM((0, 0, NAN)))

# rc_ao_filter_check's clauses, and the filter entry saying the same
BAD_FILTERS = {"radius9": FILT(count=9), "radius_neg": FILT(count=-1), "pad": FILT(pad=1),
               "taps0": FILT(2, [0, 1, 1]), "cap": FILT(8, [22] + [10] * 8),
               "cap_r0": FILT(0, [182]), "nmin_nan": FILT(nmin=NAN), "dplane_nan": FILT(dplane=NAN),
               "dplane_neg": FILT(dplane=-0.5), "dplane_-inf": FILT(dplane=-INF),
               "two_radius_pad": FILT(pad=1, count=9), "two_pad_taps0": FILT(2, [0, 1, 1], pad=7),
               "two_taps0_cap": FILT(8, [0] + [200] * 8), "two_cap_nmin": FILT(0, [182], nmin=NAN),
               "two_nmin_dplane": FILT(nmin=NAN, dplane=-1.0)}
case("null", "rc_ao_filter_check", None)
for tag, f in BAD_FILTERS.items():
    case(tag, "rc_ao_filter_check", ref(f))
    filt("filter_" + tag, f=f)
case("null_out", "rc_ao_filter_box", 3, None)
case("radius9", "rc_ao_filter_box", 9, ref(rc.RcAoFilter()))
case("null_out", "rc_ao_filter_tent", 3, None)
case("radius_neg", "rc_ao_filter_tent", -1, ref(rc.RcAoFilter()))
# the filter entry: null pointers, the guide, the alignment, the sizes, then the check
filt("null_ao", ao=None)
filt("null_guide", guide=None)
filt("null_filter", f=None)
filt("null_out", out=None)
filt("two_null_odd", ao=ODD4, out=None)
filt("guide_no_id", guide=PLANES(id_=None))
filt("guide_no_P", guide=PLANES(P=None))
filt("guide_no_N", guide=PLANES(N=None))
filt("guide_no_t_is_fine_but_w0", guide=PLANES(t=None), w=0)
filt("two_guide_odd", guide=PLANES(N=None), ao=ODD4)
filt("odd_ao", ao=ODD4)
filt("two_odd_w0", ao=FAKE + 2, w=0)
filt("w0", w=0)
filt("h_neg", h=-3)
filt("one_grid_w", w=16 * 65535 + 1, h=1)
filt("one_grid_h", w=1, h=0x7fffffff)
filt("two_w0_filter", w=0, f=FILT(pad=1))
filt("two_grid_filter", w=1, h=16 * 65535 + 1, f=FILT(pad=1))
# the compose: null pointers, the modes (above), the ambient, the sizes
comp("null_scene", O(), sc=None)
comp("null_opt", None)
comp("null_id", O(), ids=None)
comp("null_ao", O(), ao=None)
comp("null_ambient", O(), amb=None)
comp("null_in", O(), rin=None)
comp("null_out", O(), rout=None)
comp("two_null_parity", O("parity"), ao=None)
comp("ambient_nan", O(), amb=AMB(0.1, NAN, 0.1))
comp("ambient_inf", O(), amb=AMB(INF, 0.1, 0.1))
comp("ambient_neg", O(), amb=AMB(0.1, 0.1, -0.25))
comp("two_cuda_ambient", O("cuda"), amb=AMB(-1.0, 0.0, 0.0))
comp("two_ambient_w0", O(), amb=AMB(0.0, -1.0, NAN), w=0)
comp("w0", O(), w=0)
comp("h_neg", O(), h=-1)
comp("one_grid", O(), w=16 * 65535 + 1, h=1)
comp("one_grid_pixels", O(), w=16 * 65535, h=16 * 65535)
comp("ssaa2_is_not_looked_at_but_w0", O(ssaa=2), w=0)
# the host form: null pointers, rc_render_ao's clauses (above), the filter, the ambient
host("null_scene", O(), sc=None)
host("null_cam", O(), cam=None)
host("null_opt", None)
host("null_sets", O(), sets_=None)
host("null_filter", O(), f=None)
host("null_ambient", O(), amb=None)
host("null_out", O(), out=None)
host("nsets0", O(), nsets=0)
host("second_set_tmax", O(), sets_=SETS(DIRS(), DIRS(tmax=0.0)), nsets=2)
host("two_eye_nan_nsets0", O(), cam=CAM((NAN, 0, 0)), nsets=0)
host("two_set_filter", O(), sets_=SETS(DIRS(count=65)), f=FILT(pad=1))
host("filter_pad", O(), f=FILT(pad=1))
host("filter_cap", O(), f=FILT(8, [22] + [10] * 8))
host("two_filter_ambient", O(), f=FILT(nmin=NAN), amb=AMB(-1.0, 0.0, 0.0))
host("ambient_neg", O(), amb=AMB(0.0, 0.0, -1.0))
host("ambient_nan", O(), amb=AMB(NAN, 0.0, 0.0))

assert len({c[0] for c in CASES}) == len(CASES), "duplicate case ids"


def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("cid,export,args", CASES, ids=[c[0] for c in CASES])
def test_refusal(cid, export, args):
    """-1 and one message, from the arguments alone: these run without a GPU, so no refusal can
    have touched a device, and the pre-filled host bytes stay as they were."""
    got = run_refusal(export, args)
    assert got["rc"] == -1
    assert got["stderr"].startswith("Error: rc_") and got["stderr"].count("\n") == 1
    assert got == golden()[cid]
    assert (_PIX == 0x5a).all() and all((a == 0x5a).all() for a in _PL)


def test_golden_has_no_stale_case():
    assert sorted(golden()) == sorted(c[0] for c in CASES)


def test_the_filter_checks_clauses_in_order():
    g = golden()
    chk = "rc_ao_filter_check[%s]"
    assert "a null filter" in g[chk % "null"]["stderr"]
    assert "radius 9 is not 0..8" in g[chk % "radius9"]["stderr"]
    assert "radius -1 is not 0..8" in g[chk % "radius_neg"]["stderr"]
    assert "pad 1 is not 0" in g[chk % "pad"]["stderr"]
    assert "taps[0] is 0" in g[chk % "taps0"]["stderr"]
    assert "181" not in g[chk % "cap"]["stderr"] and "182" in g[chk % "cap"]["stderr"]
    assert "33124" in g[chk % "cap"]["stderr"] and "33124" in g[chk % "cap_r0"]["stderr"]
    assert "nmin is NaN" in g[chk % "nmin_nan"]["stderr"]
    for tag in ("dplane_nan", "dplane_neg", "dplane_-inf"):
        assert "is NaN or negative" in g[chk % tag]["stderr"]
    assert "radius 9" in g[chk % "two_radius_pad"]["stderr"]
    assert "pad 7" in g[chk % "two_pad_taps0"]["stderr"]
    assert "taps[0] is 0" in g[chk % "two_taps0_cap"]["stderr"]
    assert "more than 32768" in g[chk % "two_cap_nmin"]["stderr"]
    assert "nmin is NaN" in g[chk % "two_nmin_dplane"]["stderr"]
    # the entry says what the check says, under the check's name
    for tag in BAD_FILTERS:
        assert g["rc_ao_filter_device[filter_%s]" % tag] == g[chk % tag], tag
    assert g["rc_render_ambient[filter_pad]"] == g[chk % "pad"]
    assert g["rc_render_ambient[filter_cap]"] == g[chk % "cap"]


def test_the_entries_refusals_order():
    """The documented orders, on calls that break two rules: the earlier clause speaks."""
    g = golden()
    flt, cmp_, hst = "rc_ao_filter_device[%s]", "rc_ao_compose_device[%s]", "rc_render_ambient[%s]"
    for e in ("rc_render_camera_gbuffer[%s]", "rc_render_camera_gbuffer_device[%s]"):
        assert "a null pointer" in g[e % "two_null_cuda"]["stderr"]
        assert "all four planes are null" in g[e % "two_no_plane_parity"]["stderr"]
        assert "num_gpus 2" in g[e % "two_cuda_gpus2"]["stderr"]
        assert "is for fast mode" in g[e % "two_parity_gpus2"]["stderr"]
        assert "is for fast mode" in g[e % "two_parity_ssaa2"]["stderr"]
        assert "rays with an origin are for fast mode" in g[e % "two_cuda_ssaa2"]["stderr"]
        assert "rays with an origin are for fast mode" in g[e % "two_cuda_window"]["stderr"]
        assert g[e % "two_window_ssaa2"]["stderr"].startswith("Error: rc_window_check: ")
        assert g[e % "two_window_eye_nan"]["stderr"].startswith("Error: rc_window_check: ")
        assert "ssaa 2 in the options" in g[e % "two_ssaa2_eye_nan"]["stderr"]
        assert g[e % "eye_nan"]["stderr"].startswith("Error: rc_camera_check: eye[2]")
    assert "a null pointer" in g[flt % "two_null_odd"]["stderr"]
    assert "needs its id, P and N" in g[flt % "two_guide_odd"]["stderr"]
    assert "not 4-byte aligned" in g[flt % "two_odd_w0"]["stderr"]
    assert "at least 1" in g[flt % "guide_no_t_is_fine_but_w0"]["stderr"]
    assert "at least 1" in g[flt % "two_w0_filter"]["stderr"]
    assert "past one grid" in g[flt % "two_grid_filter"]["stderr"]
    assert "past one grid" in g[flt % "one_grid_w"]["stderr"]
    assert "past one grid" in g[flt % "one_grid_h"]["stderr"]
    assert "a null pointer" in g[cmp_ % "two_null_parity"]["stderr"]
    assert "rays with an origin are for fast mode" in g[cmp_ % "two_cuda_ambient"]["stderr"]
    assert "num_gpus 2" in g[cmp_ % "two_cuda_gpus2"]["stderr"]
    assert "ambient[1] is -1" in g[cmp_ % "two_ambient_w0"]["stderr"]
    assert "at least 1" in g[cmp_ % "ssaa2_is_not_looked_at_but_w0"]["stderr"]
    assert "past one grid" in g[cmp_ % "one_grid_pixels"]["stderr"]
    assert g[hst % "two_eye_nan_nsets0"]["stderr"].startswith("Error: rc_camera_check: eye[0]")
    assert "sets[0] fails rc_ao_dirs_check: n 65" in g[hst % "two_set_filter"]["stderr"]
    assert "nmin is NaN" in g[hst % "two_filter_ambient"]["stderr"]
    assert "ambient[2] is -1" in g[hst % "ambient_neg"]["stderr"]


def test_the_occlusion_familys_words_carry_over():
    """What rc_render_ao refuses, rc_render_ambient refuses with the same words under its own
    name: both go through the same clauses."""
    with open(os.path.join(GOLDEN, "ao_refusals.json")) as f:
        old = json.load(f)
    own = golden()
    for tag in ("parity", "gpus2", "cuda", "w0", "window_outside", "ssaa2", "ssaa3", "eye_nan",
                "nsets0", "second_set_tmax"):
        assert own["rc_render_ambient[%s]" % tag]["stderr"] == \
            old["rc_render_ao[%s]" % tag]["stderr"].replace("rc_render_ao", "rc_render_ambient"), tag


# ---------------------------------------------- the inputs of tests/test_gpu_guided.py --
def shares(k, radius, taps):
    name, eye, m = rcs.CAMERAS[k]
    acc = gc.state(name, eye, m, [rc.ao_dirs(16, INF)])
    f = rc.ao_filter_params(radius, taps, gc.NMIN, gc.DPLANE)
    return gc.neighbour_shares(acc, gc.planes(name, eye, m), f)


@pytest.mark.parametrize("radius,taps", gc.SHORT, ids=["r1", "r3"])
@pytest.mark.parametrize("k", gc.MIXED_CAMS)
def test_the_inputs_have_accepted_and_rejected_neighbours(k, radius, taps):
    """So that the GPU cases cannot pass on a filter that does nothing, or on one that ignores its
    guide.  33 x 17, ao_dirs(16, inf), one reset pass, nmin 0.9, dplane 0.05.  Measured minima
    over the eight cases: 0.34, 0.41, 0.36."""
    mixed, changed, unguided, hits = shares(k, radius, taps)
    print(f"camera {k} radius {radius}: mixed {mixed:.3f} changed {changed:.3f} "
          f"unguided differs {unguided:.3f} of {hits} hit pixels")
    assert hits > 0.3 * gc.SIZE[0] * gc.SIZE[1]
    assert mixed >= 0.30
    assert changed >= 0.40
    assert unguided >= 0.30


@pytest.mark.parametrize("radius,taps", gc.SHORT, ids=["r1", "r3"])
def test_the_eye_inside_a_sphere_rejects_nothing(radius, taps):
    """Camera 1 is the all-accepted case: there the guided filter is the unguided one."""
    mixed, changed, unguided, hits = shares(gc.ALL_ACCEPTED_CAM, radius, taps)
    assert hits == gc.SIZE[0] * gc.SIZE[1]
    assert mixed == 0.0 and unguided == 0.0 and changed >= 0.40


@pytest.mark.parametrize("k", gc.CAMS)
def test_at_radius_8_nearly_every_window_is_mixed(k):
    mixed = shares(k, 8, "box")[0]
    print(f"camera {k} radius 8 box: mixed {mixed:.3f}")
    assert mixed >= 0.85


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_guided.py --record   (writes " + GOLDEN_FILE + ")")
    with open(GOLDEN_FILE, "w") as f:
        json.dump({cid: run_refusal(export, args) for cid, export, args in CASES}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
