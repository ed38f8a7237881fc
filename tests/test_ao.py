"""Any-hit visibility and ambient occlusion without a GPU: the yardstick (the
contract's rule at tmax = inf is the oracle's own shadow scan on every ray the GPU suite uses), the
contract's numpy side (rc.ao_step, rc.ao_byte, rc.ao_flip, rc.ao_dirs) on hand cases, the
Python-side argument errors, every refusal of the entries pinned byte for byte in
tests/golden/ao_refusals.json (recorded by this file run as a script with --record), and the
conditions on the inputs of tests/test_gpu_ao.py, from the oracle's side."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import ao_cases as aoc
import prim_cases as pc
import ray_cases as rcs
from helpers import GOLDEN, rc
from test_refusals import FAKE, O, S, WIN, ref, run_refusal

F32, I32 = np.float32, np.int32
INF = np.inf
GOLDEN_FILE = os.path.join(GOLDEN, "ao_refusals.json")
NEW_EXPORTS = ["rc_ao_dirs_check", "rc_occluded_rays", "rc_occluded_rays_device",
               "rc_ao_pass_device", "rc_ao_resolve_device", "rc_render_ao", "rc_ao_stats_get",
               "rc_ao_phase_ms"]
SET_SIZES = (1, 5, 16, 64)


def sets(n, tmax=INF):
    return rc.ao_dirs(n, tmax), rc.ao_dirs(n, tmax, aoc.ROT)


# ------------------------------------------------------------------------- the yardstick --
@pytest.mark.parametrize("k", aoc.CAMS)
def test_the_rule_at_inf_is_the_oracles_shadow_scan(k):
    """Passes without the feature: it pins the expectation itself.  Every occlusion ray of the
    GPU suite's state cases (both passes' sets at every size), skip = the hit shape."""
    name, eye, m = rcs.CAMERAS[k]
    sc = rcs.scene(name)
    total = 0
    for n in SET_SIZES:
        for u, _ in sets(n):
            Oh, D, skip, _ = aoc.hit_rays(name, eye, m, u)
            rule = aoc.blocked_rule(sc.js, sc.num_shapes, Oh, D, skip, INF)
            idx = pc.ref_nearest(sc.js, Oh, D, skip, shadow=True)[0]
            np.testing.assert_array_equal(rule, idx >= 0, err_msg=f"{name} {eye} n{n}")
            total += len(skip)
    assert total > 1000


def test_the_rule_at_inf_without_a_skip():
    """skip = -1 (the ray batch's default): the z rule off, nothing skipped."""
    name, eye, m = rcs.CAMERAS[9]
    sc = rcs.scene(name)
    Oh, D, skip, _ = aoc.hit_rays(name, eye, m, rc.ao_dirs(16)[0])
    none = np.full(len(skip), -1, I32)
    rule = aoc.blocked_rule(sc.js, sc.num_shapes, Oh, D, none, INF)
    np.testing.assert_array_equal(rule, pc.ref_nearest(sc.js, Oh, D, none, shadow=True)[0] >= 0)
    assert (rule != aoc.blocked_rule(sc.js, sc.num_shapes, Oh, D, skip, INF)).any()


# ----------------------------------------------------------------- the inputs' conditions --
@pytest.mark.parametrize("k", aoc.CAMS)
def test_the_inputs_are_not_constant_planes(k):
    """At 33 x 17 with ao_dirs(16): at least 30 % primary hits, at least 40 % of the hit pixels
    mixed (0 < open < n) at tmax = inf and at least 20 % at tmax = 2.0."""
    name, eye, m = rcs.CAMERAS[k]
    ids = aoc.primary(name, eye, m)[0]
    assert (ids >= 0).mean() >= 0.30
    assert aoc.mixed_share(name, eye, m, rc.ao_dirs(16, INF)) >= 0.40
    assert aoc.mixed_share(name, eye, m, rc.ao_dirs(16, 2.0)) >= 0.20


def test_the_bound_matters():
    """tmax = 2.0 opens rays that tmax = inf has blocked, and never the reverse."""
    for k in aoc.CAMS:
        name, eye, m = rcs.CAMERAS[k]
        far = aoc.open_add(name, eye, m, rc.ao_dirs(16, INF))[0]
        near = aoc.open_add(name, eye, m, rc.ao_dirs(16, 2.0))[0]
        assert (near >= far).all() and (near > far).any()


# -------------------------------------------------------------------- the numpy contract --
def state(open_, rays):
    acc = np.zeros(np.shape(open_), rc.AO_DTYPE)
    acc["open"], acc["rays"] = open_, rays
    return acc


def test_ao_byte_hand_cases():
    acc = state([[0, 7, 0, 1, 1, 3, 65535, 0]], [[0, 7, 9, 2, 510, 4, 65535, 65535]])
    # rays = 0: 255; open = rays: 255; open = 0: 0; 1/2: 127.5 -> 128 (the tie rounds up);
    # 1/510: exactly 0.5 -> 1; 3/4: 191.25 -> 191
    np.testing.assert_array_equal(rc.ao_byte(acc), [[255, 255, 0, 128, 1, 191, 255, 0]])


def test_ao_step_hand_cases():
    acc = state([[5, 0, 65000, 65472]], [[10, 0, 65532, 65531]])
    new, sat = rc.ao_step(acc, np.array([[3, 4, 2, 0]]), 4)
    assert sat == 1                                  # 65532 + 4 > 65535; 65531 + 4 is not
    np.testing.assert_array_equal(new["open"], [[8, 4, 65000, 65472]])
    np.testing.assert_array_equal(new["rays"], [[14, 4, 65532, 65535]])
    new, sat = rc.ao_step(acc, np.array([[3, 4, 2, 4]]), 4, reset=True)
    assert sat == 0
    np.testing.assert_array_equal(new["open"], [[3, 4, 2, 4]])
    np.testing.assert_array_equal(new["rays"], [[4, 4, 4, 4]])
    # saturation at 65535 exactly: 65472 + 63 fits, one more ray does not
    full, sat = rc.ao_step(state([[1]], [[65535 - 63]]), np.array([[63]]), 63)
    assert sat == 0 and full["rays"][0, 0] == 65535 and full["open"][0, 0] == 64
    again, sat = rc.ao_step(full, np.array([[1]]), 1)
    assert sat == 1
    np.testing.assert_array_equal(again, full)
    assert acc["rays"][0, 0] == 10                   # the argument is not written


def test_ao_flip():
    u = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, -2.0, 0.5]], F32)
    N = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [np.nan, 0.0, 0.0], [-0.0, 0.0, 0.0]], F32)
    got = rc.ao_flip(N, u)
    assert got.shape == (4, 3, 3) and got.dtype == F32
    # N = -z: u0 flips (dot -1), u1 stays (dot +0 - 0... = 0), u2 flips (dot -0.5)
    np.testing.assert_array_equal(got[0], [[0, 0, -1], [1, 0, 0], [0, 2, -0.5]])
    np.testing.assert_array_equal(got[1], u)
    np.testing.assert_array_equal(got[2], u)        # a NaN dot does not flip
    np.testing.assert_array_equal(got[3], u)        # dot = -0 is not below zero
    assert np.signbit(got[0][0][0]) and np.signbit(got[0][0][1])   # the flip is * -1.0f: +0 -> -0
    assert (np.signbit(got[3]) == np.signbit(u)).all()


def test_ao_dirs():
    for n in (1, 2, 5, 16, 64):
        u, tmax = rc.ao_dirs(n)
        assert u.shape == (n, 3) and u.dtype == F32 and tmax == INF
        ln = np.sqrt((u.astype(np.float64) ** 2).sum(axis=1))
        assert np.abs(ln - 1.0).max() < 1e-6
        assert (np.diff(u[:, 2]) < 0).all()
        same, _ = rc.ao_dirs(n, 2.0, np.eye(3))
        np.testing.assert_array_equal(same.view(np.uint32), u.view(np.uint32))
        turned, t2 = rc.ao_dirs(n, 2.0, aoc.ROT)
        assert t2 == 2.0 and (turned != u).any()
        assert np.abs(np.sqrt((turned.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() < 1e-6
        assert rc.ao_dirs_check((u, tmax)) and rc.ao_dirs_check((turned, 2.0))
    # n = 1: i + 1/2 = 1/2, z = 0, r = 1, phi = pi (3 - sqrt 5) / 2
    phi = np.pi * (3.0 - np.sqrt(5.0)) / 2.0
    np.testing.assert_array_equal(rc.ao_dirs(1)[0],
                                  np.array([[np.cos(phi), np.sin(phi), 0.0]]).astype(F32))


def test_argument_errors():
    for bad in (0, 65, -1):
        with pytest.raises(ValueError):
            rc.ao_dirs(bad)
    with pytest.raises(ValueError):
        rc.ao_dirs(4, rot=np.eye(2))
    for bad in (np.zeros((0, 3)), np.zeros((65, 3)), np.zeros((4, 2)), np.zeros(3)):
        with pytest.raises(ValueError):
            rc._rc_ao_dirs((bad, 1.0), "test")
    with pytest.raises(ValueError):
        rc._rc_ao_dirs(np.zeros((4, 3)), "test")
    acc = state([[0]], [[0]])
    for add, n in (([[5]], 4), ([[-1]], 4), ([[1]], 0), ([[1]], 65), ([[1, 1]], 4)):
        with pytest.raises(ValueError):
            rc.ao_step(acc, np.array(add), n)
    with pytest.raises(ValueError):
        rc.ao_step(np.zeros((1, 1), np.uint32), np.array([[1]]), 4)
    with pytest.raises(ValueError):
        rc.ao_byte(np.zeros((1, 1, 2), np.uint16))
    sc = rcs.scene("simple")
    d = np.zeros((4, 3), F32)
    with pytest.raises(ValueError):
        rc.occluded_rays(sc, np.zeros((3, 3), F32), d)
    with pytest.raises(ValueError):
        rc.occluded_rays(sc, d, d, skip=np.zeros(3, I32))
    with pytest.raises(ValueError):
        rc.occluded_rays(sc, d, d, tmax=np.zeros((4, 1), F32))
    with pytest.raises(ValueError):
        rc.render_ao(sc, (0, 0, 0), None, 8, 8, [])


def test_the_exports_and_the_layouts():
    for name in NEW_EXPORTS:
        assert name in rc.HIP_EXPORTS and hasattr(rc.hip_lib(), name), name
    assert ctypes.sizeof(rc.RcAoDirs) == 776 and rc.AO_DTYPE.itemsize == 4
    assert rc.RcAoDirs.tmax.offset == 4 and rc.RcAoDirs.u.offset == 8
    d = rc._rc_ao_dirs(rc.ao_dirs(5, 2.0), "test")
    assert d.n == 5 and d.tmax == 2.0
    np.testing.assert_array_equal(np.ctypeslib.as_array(d.u)[:5], rc.ao_dirs(5)[0])
    # rc_ao_px: open in the low half of the little-endian dword, rays in the high half
    acc = state([[3]], [[7]])
    assert acc.view(np.uint32)[0, 0] == 3 | (7 << 16)


# ------------------------------------------------------------------------------ refusals --
ODD4 = 4098      # a non-null "device pointer" that is not 4-byte aligned


def CAM(eye=(0.5, 0.25, 1.0), m=None):
    return rc._rc_camera(eye, m)


def DIRS(n=4, tmax=INF, edit=None, count=None):
    d = rc._rc_ao_dirs(rc.ao_dirs(n, tmax), "test")
    for (j, k), x in (edit or {}).items():
        d.u[j][k] = x
    if count is not None:
        d.n = count
    return d


def SETS(*ds):
    arr = (rc.RcAoDirs * len(ds))()
    for k, d in enumerate(ds):
        arr[k] = d
    return arr


def _bad_m(k, x):
    m = np.eye(3).ravel()
    m[k] = x
    return CAM(m=m)


ZERO2 = {(2, 0): 0.0, (2, 1): -0.0, (2, 2): 0.0}
GOODW = WIN(64, 48, 8, 4)
GOODD = DIRS()
ONE = SETS(GOODD)
_PIX = np.full((8, 8), 0x5a, np.uint8)
PIX = _PIX.ctypes.data
_RAYS = np.ones((4, 3), F32)
RAYS = _RAYS.ctypes.data
CASES = []


def case(tag, export, *args):
    CASES.append((f"{export}[{tag}]", export, args))


def a_pass(tag, opt, cam=CAM(), dirs=GOODD, w=8, h=8, win=GOODW, ao=FAKE, out=FAKE, sc=S):
    case(tag, "rc_ao_pass_device", sc, ref(cam), ref(win), w, h, ref(opt), ref(dirs), 1, ao, out,
         None, None)


def host(tag, opt, cam=CAM(), sets_=ONE, nsets=1, w=8, h=8, win=GOODW, out=PIX, sc=S):
    case(tag, "rc_render_ao", sc, ref(cam), ref(win), w, h, ref(opt), sets_, nsets, out, None)


def both(tag, opt, **kw):
    a_pass(tag, opt, **kw)
    host(tag, opt, **kw)


def rays(tag, opt, n=4, origins=RAYS, dirs=RAYS, out=PIX, sc=S):
    for export, o in (("rc_occluded_rays", out), ("rc_occluded_rays_device", out and FAKE)):
        case(tag, export, sc, ref(opt), n, origins, dirs, None, None, o, None, None)


# 1. null pointers (the window and the pass's bytes may be null)
a_pass("null_scene", O(), sc=None)
a_pass("null_cam", O(), cam=None)
a_pass("null_opt", None)
a_pass("null_dirs", O(), dirs=None)
a_pass("null_ao", O(), ao=None)
a_pass("two_null_odd", O(), dirs=None, ao=ODD4)
a_pass("two_null_cuda", O("cuda"), cam=None)
host("null_scene", O(), sc=None)
host("null_cam", O(), cam=None)
host("null_opt", None)
host("null_sets", O(), sets_=None)
host("null_out", O(), out=None)
rays("null_scene", O(), sc=None)
rays("null_opt", None)
rays("null_origins", O(), origins=None)
rays("null_dirs", O(), dirs=None)
rays("null_out", O(), out=None)
# 2. a misaligned state
a_pass("odd_ao", O(), ao=ODD4)
a_pass("odd_ao_2", O(), ao=FAKE + 2)
a_pass("two_odd_parity", O("parity"), ao=ODD4)
# 3. the camera family's clauses: parity, num_gpus, cuda, then the window
for tag, opt in {"parity": O("parity"), "gpus2": O(gpus=2), "cuda": O("cuda"),
                 "two_cuda_gpus2": O("cuda", gpus=2), "two_parity_gpus2": O("parity", gpus=2),
                 "two_parity_ssaa2": O("parity", ssaa=2), "two_cuda_ssaa2": O("cuda", ssaa=2)}.items():
    both(tag, opt)
    rays(tag, opt)
for tag, (w, h, win) in {"w0": (0, 8, GOODW), "h_neg": (8, -1, GOODW),
                         "no_window_w0": (0, 8, None),
                         "window_outside": (8, 8, WIN(64, 48, 60, 0)),
                         "window_origin": (8, 8, WIN(64, 48, 0, -1)),
                         "tile_rows": (1, 1 << 26, WIN(1 << 27, 1 << 27, 0, 0))}.items():
    both(tag, O(), w=w, h=h, win=win)
both("two_cuda_window", O("cuda"), win=WIN(64, 48, 60, 0))
both("two_window_ssaa2", O(ssaa=2), win=WIN(64, 48, 60, 0))
both("two_window_eye_nan", O(), win=WIN(64, 48, 60, 0), cam=CAM((np.nan, 0, 0)))
# 4. ssaa
for tag, opt in {"ssaa2": O(ssaa=2), "ssaa3": O(ssaa=3), "ssaa-1": O(ssaa=-1), "ssaa8": O(ssaa=8),
                 "ssaa4_adaptive": O(ssaa=4, adaptive=16),
                 "thr_no_factor": O(ssaa=1, adaptive=16)}.items():
    both(tag, opt)
    rays(tag, opt)
both("two_ssaa2_eye_nan", O(ssaa=2), cam=CAM((np.nan, 0, 0)))
a_pass("two_ssaa2_dirs", O(ssaa=2), dirs=DIRS(count=0))
rays("two_ssaa2_n0", O(ssaa=2), n=0)
# 5. the camera; the number of rays
both("eye_nan", O(), cam=CAM((0, 0, np.nan)))
both("eye_inf", O(), cam=CAM((-np.inf, 0, 0)))
both("m_inf", O(), cam=_bad_m(5, np.inf))
a_pass("two_eye_nan_dirs", O(), cam=CAM((np.nan, 0, 0)), dirs=DIRS(count=0))
host("two_eye_nan_nsets0", O(), cam=CAM((np.nan, 0, 0)), nsets=0)
for tag, n in {"n0": 0, "n_neg": -5, "n_2^24+1": (1 << 24) + 1}.items():
    rays(tag, O(), n=n)
# 6. the direction set
BAD_DIRS = {"n0": DIRS(count=0), "n65": DIRS(count=65), "n_neg": DIRS(count=-1),
            "tmax0": DIRS(tmax=0.0), "tmax_neg": DIRS(tmax=-2.0), "tmax_nan": DIRS(tmax=np.nan),
            "tmax_-inf": DIRS(tmax=-INF), "u_nan": DIRS(edit={(3, 1): np.nan}),
            "u_inf": DIRS(edit={(0, 2): INF}), "u_zero": DIRS(edit=ZERO2),
            "zero_before_nan": DIRS(8, edit={**ZERO2, (5, 0): np.nan}),
            "nan_before_zero": DIRS(8, edit={(1, 2): np.nan, **ZERO2}),
            "two_n65_tmax0": DIRS(tmax=0.0, count=65),
            "two_tmax_u": DIRS(tmax=-1.0, edit={(0, 0): np.nan}),
            "past_n_is_not_read": None}
for tag, d in BAD_DIRS.items():
    if d is not None:
        a_pass("dirs_" + tag, O(), dirs=d)
        case(tag, "rc_ao_dirs_check", ref(d))
case("null", "rc_ao_dirs_check", None)
for tag, n in {"nsets0": 0, "nsets_neg": -1, "nsets1025": 1025}.items():
    host(tag, O(), nsets=n)
host("second_set_tmax", O(), sets_=SETS(GOODD, DIRS(tmax=0.0)), nsets=2)
host("third_set_u", O(), sets_=SETS(GOODD, GOODD, DIRS(edit=ZERO2), DIRS(count=0)), nsets=4)
host("first_set_n", O(), sets_=SETS(DIRS(count=65), DIRS(tmax=0.0)), nsets=2)
host("two_nsets_set", O(), sets_=SETS(DIRS(count=65)), nsets=0)
# rc_ao_resolve_device
for tag, (ao, w, h, out) in {"null_ao": (None, 8, 8, FAKE), "null_out": (FAKE, 8, 8, None),
                             "odd_ao": (ODD4, 8, 8, FAKE), "two_odd_w0": (ODD4, 0, 8, FAKE),
                             "w0": (FAKE, 0, 8, FAKE), "h_neg": (FAKE, 8, -1, FAKE),
                             "one_grid": (FAKE, 0x7fffffff, 0x7fffffff, FAKE)}.items():
    case(tag, "rc_ao_resolve_device", ao, w, h, out, None)

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
    assert (_PIX == 0x5a).all()


def test_golden_has_no_stale_case():
    assert sorted(golden()) == sorted(c[0] for c in CASES)


def test_the_refusals_order():
    """The documented order, on calls that break two rules: the earlier clause speaks."""
    g = golden()
    dev, hst, ray = "rc_ao_pass_device[%s]", "rc_render_ao[%s]", "rc_occluded_rays[%s]"
    assert "a null pointer" in g[dev % "two_null_odd"]["stderr"]
    assert "a null pointer" in g[dev % "two_null_cuda"]["stderr"]
    assert "not 4-byte aligned" in g[dev % "two_odd_parity"]["stderr"]
    for e in (dev, hst, ray):
        assert "num_gpus 2" in g[e % "two_cuda_gpus2"]["stderr"]
        assert "are for fast mode: a parity image" in g[e % "two_parity_gpus2"]["stderr"]
        assert "are for fast mode: a parity image" in g[e % "two_parity_ssaa2"]["stderr"]
        assert "rays with an origin are for fast mode" in g[e % "two_cuda_ssaa2"]["stderr"]
        assert "ssaa 2 in the options" in g[e % "ssaa2"]["stderr"]
    for e in (dev, hst):
        assert "rays with an origin are for fast mode" in g[e % "two_cuda_window"]["stderr"]
        assert g[e % "two_window_ssaa2"]["stderr"].startswith("Error: rc_window_check: ")
        assert g[e % "two_window_eye_nan"]["stderr"].startswith("Error: rc_window_check: ")
        assert "ssaa 2 in the options" in g[e % "two_ssaa2_eye_nan"]["stderr"]
    assert "ssaa 2 in the options" in g[dev % "two_ssaa2_dirs"]["stderr"]
    assert "ssaa 2 in the options" in g[ray % "two_ssaa2_n0"]["stderr"]
    assert g[dev % "two_eye_nan_dirs"]["stderr"].startswith("Error: rc_camera_check: eye[0]")
    assert g[hst % "two_eye_nan_nsets0"]["stderr"].startswith("Error: rc_camera_check: eye[0]")
    assert "nsets 0 is not 1..1024" in g[hst % "two_nsets_set"]["stderr"]
    assert "sets[1] fails rc_ao_dirs_check: tmax 0" in g[hst % "second_set_tmax"]["stderr"]
    assert "sets[2] fails rc_ao_dirs_check: u[2] is the zero" in g[hst % "third_set_u"]["stderr"]
    assert "sets[0] fails rc_ao_dirs_check: n 65" in g[hst % "first_set_n"]["stderr"]
    assert "not 4-byte aligned" in g["rc_ao_resolve_device[two_odd_w0]"]["stderr"]


def test_the_direction_sets_refusals_name_the_first_offender():
    g = golden()
    chk = "rc_ao_dirs_check[%s]"
    assert "n 65 is not 1..64" in g[chk % "two_n65_tmax0"]["stderr"]
    assert "tmax -1 is not in (0, +inf]" in g[chk % "two_tmax_u"]["stderr"]
    assert "tmax nan" in g[chk % "tmax_nan"]["stderr"]
    assert "tmax -inf" in g[chk % "tmax_-inf"]["stderr"]
    assert "u[3][1] is not finite" in g[chk % "u_nan"]["stderr"]
    assert "u[0][2] is not finite" in g[chk % "u_inf"]["stderr"]
    assert "u[2] is the zero vector" in g[chk % "u_zero"]["stderr"]
    assert "u[2] is the zero vector" in g[chk % "zero_before_nan"]["stderr"]
    assert "u[1][2] is not finite" in g[chk % "nan_before_zero"]["stderr"]
    # the pass says what the check says, under the check's name
    for tag in BAD_DIRS:
        if BAD_DIRS[tag] is not None:
            assert g["rc_ao_pass_device[dirs_%s]" % tag] == g[chk % tag], tag


def test_directions_past_n_are_not_looked_at():
    d = DIRS(4)
    d.u[4][0] = np.nan
    assert rc.hip_lib().rc_ao_dirs_check(ctypes.byref(d)) == 0
    assert rc.ao_dirs_check((np.array([[0, 0, 3e38]], F32), INF))
    assert rc.ao_dirs_check((np.array([[0, 1e-45, 0]], F32), 1e-30))


def test_the_camera_familys_words_carry_over():
    """What rc_render_camera refuses of a camera and a window, the pass refuses with the same
    words: both go through rc_camera_check and rc_window_check."""
    with open(os.path.join(GOLDEN, "camera_refusals.json")) as f:
        old = json.load(f)
    own = golden()
    for e in ("rc_ao_pass_device", "rc_render_ao"):
        assert own[e + "[eye_nan]"] == old["rc_render_camera[eye_nan]"]
        assert own[e + "[window_outside]"]["stderr"] == old["rc_render_camera[outside]"][
            "stderr"].replace("a 16 x 16 window at (60, 4)", "a 8 x 8 window at (60, 0)")


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_ao.py --record   (writes " + GOLDEN_FILE + ")")
    with open(GOLDEN_FILE, "w") as f:
        json.dump({cid: run_refusal(export, args) for cid, export, args in CASES}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} refusals in {GOLDEN_FILE}", file=sys.stderr)
