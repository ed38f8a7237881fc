"""A free camera and rays with origins without a GPU: the yardstick of
tests/test_gpu_camera.py held against the oracle's own bounce loop, the Python-side helpers and
argument errors, and every refusal of the four entries, pinned byte for byte in
tests/golden/camera_refusals.json (recorded by this file run as a script with --record)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import prim_cases as pc
import ray_cases as rcs
import shade_cases as shc
import view_cases as vc
from helpers import GOLDEN, rc
from test_refusals import FAKE, ODD, HOST, O, S, WIN, ref, run_refusal

F32 = np.float32
GOLDEN_FILE = os.path.join(GOLDEN, "camera_refusals.json")
NEW_EXPORTS = ["rc_camera_check", "rc_render_camera", "rc_render_camera_device",
               "rc_trace_rays_from", "rc_trace_rays_from_device"]


# ------------------------------------------------------------------------ the yardstick --
@pytest.mark.parametrize("name", list(shc.lit_scenes()))
def test_ref_trace_from_at_the_origin_is_the_oracles_shoot(name):
    """ref_trace_from restates the fast-mode loop between rco_prim_nearest and rco_prim_shade; at
    O = 0 the oracle runs the same loop itself (rco_prim_shoot), and the two agree in every bit.
    This test validates the yardstick: it needs no new library entry."""
    js = shc.lit_scenes()[name].js
    d = shc.camera_dirs(js)
    assert len(d) == 64 * 48
    for maxrec in (1, 2, 3, 7):
        want = shc.ref_shoot(js, d, maxrec, "fast")[0]
        got, ids, t, P, N = rcs.ref_trace_from(js, np.zeros_like(d), d, maxrec)
        assert got.dtype == F32 and (pc.bits32(got) == pc.bits32(want)).all(), (name, maxrec)
        assert ((ids >= 0) == (t > 0)).all()


def test_the_cameras_are_not_vacuous():
    """Conditions on the inputs of tests/test_gpu_camera.py, from the oracle's side: every camera
    sees at least 30 % primary hits and, but for the far eye, a bounce changes some pixel."""
    for k, (name, eye, m) in enumerate(rcs.CAMERAS):
        ids = rcs.camera_samples(name, eye, m)[2]
        assert (ids >= 0).mean() >= 0.30, (name, eye)
        if k not in rcs.NO_BOUNCE:
            assert rcs.bounce_changes(name, eye, m) > 0.0, (name, eye)


def test_a_moved_eye_changes_the_image():
    a = rcs.camera_image("quadric", (0.0, 0.0, 0.0), rcs.IDENT)
    b = rcs.camera_image("quadric", (0.5, 0.25, 1.0), rcs.IDENT)
    assert (a != b).any(axis=2).mean() >= 0.10


# --------------------------------------------------------------------- the Python side --
def test_camera_helper():
    e, m = rc.camera((1, 2.5, -3))
    assert e.dtype == F32 and e.tolist() == [1.0, 2.5, -3.0]
    assert m.dtype == F32 and (m == np.eye(3)).all()
    e, m = rc.camera(np.array([-0.0, 0.0, 1e-40]), np.arange(9))
    assert np.signbit(e[0]) and not np.signbit(e[1]) and e[2] == F32(1e-40)   # used as given
    assert m.shape == (3, 3) and m.ravel().tolist() == list(range(9))
    for bad in ((1, 2), np.zeros((2, 2)), ()):
        with pytest.raises(ValueError):
            rc.camera(bad)
    with pytest.raises(ValueError):
        rc.camera((0, 0, 0), np.eye(4))
    cam = rc._rc_camera((-0.0, 2.0, 3.0), vc.VIEWS["ypr"])
    assert np.signbit(cam.eye[0]) and list(cam.eye)[1:] == [2.0, 3.0]
    assert list(cam.view.m) == vc.VIEWS["ypr"].ravel().tolist()


def test_camera_check():
    assert rc.camera_check((0, 0, 0)) and rc.camera_check((-0.0, 3e38, -3e38), vc.VIEWS["wide"])
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            eye = [1.0, 2.0, 3.0]
            eye[k] = bad
            assert run_refusal("rc_camera_check", [ctypes.byref(rc._rc_camera(eye, None))])["rc"] == -1
        m = np.eye(3)
        m[1, 2] = bad
        assert run_refusal("rc_camera_check", [ctypes.byref(rc._rc_camera((0, 0, 0), m))])["rc"] == -1


def test_exports_layouts_and_argument_errors():
    for name in NEW_EXPORTS:
        assert name in rc.HIP_EXPORTS and hasattr(rc.hip_lib(), name), name
    assert ctypes.sizeof(rc.RcCamera) == 48 and rc.RcCamera.view.offset == 12
    sc = vc.scene("simple")
    d = np.zeros((2, 3), F32)
    with pytest.raises(ValueError):
        rc.trace_rays_from(sc, np.zeros((3, 3), F32), d)             # another n
    with pytest.raises(ValueError):
        rc.trace_rays_from(sc, np.zeros(3, F32), d)
    with pytest.raises(ValueError):
        rc.trace_rays_from(sc, np.zeros((0, 3), F32), np.zeros((0, 3), F32))
    with pytest.raises(ValueError):
        rc.trace_rays_from(sc, d, d, outputs=("depth",))
    with pytest.raises(ValueError):
        rc.render_camera(sc, (0, 0), None, 8, 8)


# ------------------------------------------------------------------------------ refusals --
def CAM(eye=(0.5, 0.25, 1.0), m=None):
    return rc._rc_camera(eye, m)


def OUT(rgb8=None, rgb=None, hits=None, frame=0):
    return rc.RcRayOut(rgb8, rgb, hits, frame)


def _bad_m(k, x):
    m = np.eye(3).ravel()
    m[k] = x
    return CAM(m=m)


GOODC = CAM()
GOODW = WIN(64, 48, 8, 4)
_RAYS = np.zeros((4, 3), F32)
_RGB8 = np.full((4, 3), 0x5a, np.uint8)
_PIX = np.full((16, 16, 3), 0x5a, np.uint8)
RAYS = _RAYS.ctypes.data
RGB8 = _RGB8.ctypes.data
PIX = _PIX.ctypes.data
CASES = []


def case(tag, export, *args):
    CASES.append((f"{export}[{tag}]", export, args))


case("null", "rc_camera_check", None)
for tag, c in {"eye_nan": CAM((np.nan, 0, 0)), "eye_inf": CAM((0, np.inf, 0)),
               "eye_neg_inf": CAM((0, 0, -np.inf)), "m_nan": _bad_m(5, np.nan),
               "two_eye_nan_m_inf": CAM((0, np.nan, 0), np.full(9, np.inf))}.items():
    case(tag, "rc_camera_check", ref(c))


def camera_pair(tag, opt, cam=GOODC, win=GOODW, w=16, h=16):
    case(tag, "rc_render_camera", S, ref(cam), ref(win), w, h, ref(opt), PIX, None)
    case(tag, "rc_render_camera_device", S, ref(cam), ref(win), w, h, ref(opt), FAKE, None, None)


# everything rc_render_view refuses, then cuda mode
for tag, opt in {"ssaa3": O(ssaa=3), "ssaa-1": O(ssaa=-1), "thr_no_factor": O(ssaa=1, adaptive=16),
                 "ssaa4_adaptive": O(ssaa=4, adaptive=16), "parity": O("parity"),
                 "gpus2": O(gpus=2), "cuda": O("cuda"), "cuda_ssaa4": O("cuda", ssaa=4),
                 "two_cuda_gpus2": O("cuda", gpus=2),
                 "two_adaptive_parity": O("parity", ssaa=4, adaptive=16),
                 "two_parity_gpus2": O("parity", gpus=2)}.items():
    camera_pair(tag, opt)
camera_pair("eye_nan", O(), CAM((0, 0, np.nan)))
camera_pair("eye_inf", O(ssaa=2), CAM((-np.inf, 0, 0)))
camera_pair("m_nan", O(), _bad_m(2, np.nan))
camera_pair("two_cuda_eye_nan", O("cuda"), CAM((np.nan, 0, 0)))
camera_pair("two_gpus2_eye_nan", O(gpus=2), CAM((np.nan, 0, 0)))
camera_pair("two_eye_nan_outside", O(), CAM((np.nan, 0, 0)), WIN(64, 48, 60, 4))
camera_pair("outside", O(ssaa=2), GOODC, WIN(64, 48, 60, 4))
camera_pair("no_window_w0", O(), GOODC, None, 0, 16)
camera_pair("past_int", O(ssaa=4), GOODC, WIN(1 << 30, 48, 0, 0))
case("null_scene", "rc_render_camera", None, ref(GOODC), None, 8, 8, ref(O()), PIX, None)
case("null_camera", "rc_render_camera", S, None, None, 8, 8, ref(O()), PIX, None)
case("null_opt", "rc_render_camera_device", S, ref(GOODC), None, 8, 8, None, FAKE, None, None)
case("null_out", "rc_render_camera_device", S, ref(GOODC), None, 8, 8, ref(O()), None, None, None)
case("two_null_cuda", "rc_render_camera", S, ref(GOODC), None, 8, 8, ref(O("cuda")), None, None)


def rays_pair(tag, opt, n=4, out=None, dev_out=None):
    case(tag, "rc_trace_rays_from", S, ref(opt), n, RAYS, RAYS,
         ref(OUT(rgb8=RGB8) if out is None else out))
    case(tag, "rc_trace_rays_from_device", S, ref(opt), n, FAKE, FAKE,
         ref(OUT(rgb8=FAKE) if dev_out is None else dev_out), None)


# everything rc_trace_rays refuses, then cuda mode
for tag, opt in {"ssaa3": O(ssaa=3), "ssaa2": O(ssaa=2), "ssaa4_adaptive": O(ssaa=4, adaptive=16),
                 "parity": O("parity"), "gpus2": O(gpus=2), "cuda": O("cuda"),
                 "two_cuda_gpus2": O("cuda", gpus=2),
                 "two_ssaa2_parity": O("parity", ssaa=2)}.items():
    rays_pair(tag, opt)
rays_pair("all_null", O(), 4, OUT(), OUT())
rays_pair("frame_cuda", O("cuda"), 4, OUT(hits=HOST, frame=1), OUT(hits=FAKE, frame=1))
rays_pair("n0", O(), 0)
rays_pair("n_neg", O(), -1)
rays_pair("n_past", O(), (1 << 24) + 1)
rays_pair("two_all_null_n0", O(), 0, OUT(), OUT())
rays_pair("two_cuda_n0", O("cuda"), 0)
case("hits_unaligned", "rc_trace_rays_from_device", S, ref(O()), 4, FAKE, FAKE, ref(OUT(hits=ODD)),
     None)
case("two_unaligned_n0", "rc_trace_rays_from_device", S, ref(O()), 0, FAKE, FAKE,
     ref(OUT(hits=ODD)), None)
case("null_scene", "rc_trace_rays_from", None, ref(O()), 4, RAYS, RAYS, ref(OUT(rgb8=RGB8)))
case("null_opt", "rc_trace_rays_from", S, None, 4, RAYS, RAYS, ref(OUT(rgb8=RGB8)))
case("null_origins", "rc_trace_rays_from", S, ref(O()), 4, None, RAYS, ref(OUT(rgb8=RGB8)))
case("null_origins", "rc_trace_rays_from_device", S, ref(O()), 4, None, FAKE, ref(OUT(rgb8=FAKE)),
     None)
case("null_dirs", "rc_trace_rays_from", S, ref(O()), 4, RAYS, None, ref(OUT(rgb8=RGB8)))
case("null_out", "rc_trace_rays_from_device", S, ref(O()), 4, FAKE, FAKE, None, None)
case("two_null_origins_cuda", "rc_trace_rays_from", S, ref(O("cuda")), 4, None, RAYS,
     ref(OUT(rgb8=RGB8)))

assert len({c[0] for c in CASES}) == len(CASES), "duplicate case ids"


def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("cid,export,args", CASES, ids=[c[0] for c in CASES])
def test_refusal(cid, export, args):
    """-1 and one message, from the arguments alone: these run without a GPU, so no refusal can
    have touched a device, and the pre-filled host outputs stay as they were."""
    got = run_refusal(export, args)
    assert got["rc"] == -1
    assert got["stderr"].startswith("Error: rc_") and got["stderr"].count("\n") == 1
    assert got == golden()[cid]
    assert (_RGB8 == 0x5a).all() and (_PIX == 0x5a).all()


def test_golden_has_no_stale_case():
    assert sorted(golden()) == sorted(c[0] for c in CASES)


def test_the_view_familys_refusals_carry_over():
    """What rc_render_view and rc_trace_rays refuse, the camera entries refuse with the same words
    but for the entry's name and the family's noun."""
    with open(os.path.join(GOLDEN, "view_refusals.json")) as f:
        view = json.load(f)
    own = golden()
    for tag in ("ssaa3", "ssaa-1", "thr_no_factor", "outside", "no_window_w0", "past_int"):
        for dev in ("", "_device"):
            if tag == "past_int":      # the view's case is in cuda mode; the message is the window's
                assert own[f"rc_render_camera{dev}[{tag}]"]["stderr"].startswith(
                    "Error: rc_window_check: ")
                continue
            a = view[f"rc_render_view{dev}[{tag}]"]["stderr"]
            b = own[f"rc_render_camera{dev}[{tag}]"]["stderr"]
            assert a.replace("rc_render_view", "rc_render_camera") == b, tag
    for tag in ("ssaa3", "ssaa2", "ssaa4_adaptive", "gpus2", "all_null", "n0", "n_past"):
        for dev in ("", "_device"):
            a = view[f"rc_trace_rays{dev}[{tag}]"]["stderr"]
            b = own[f"rc_trace_rays_from{dev}[{tag}]"]["stderr"]
            assert a.replace("rc_trace_rays", "rc_trace_rays_from") == b, tag


if __name__ == "__main__":       # python tests/test_camera.py --record
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_camera.py --record   (writes " + GOLDEN_FILE + ")")
    with open(GOLDEN_FILE, "w") as f:
        json.dump({cid: run_refusal(export, args) for cid, export, args in CASES}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} refusals in {GOLDEN_FILE}", file=sys.stderr)
