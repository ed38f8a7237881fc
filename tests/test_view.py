"""Rotated camera views and ray batches without a GPU: the numpy contract
rc.view_dirs against the existing statements of the primary ray, the oracle image through it against
the oracle's own renders, view_euler, rc_view_check and every new refusal, pinned byte for byte in
tests/golden/view_refusals.json (recorded by this file run as a script)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import prim_cases as pc
import shade_cases as sc
import view_cases as vc
from helpers import GOLDEN, oracle_render, oracle_render_cuda, rc, scene_path
from test_refusals import FAKE, ODD, HOST, O, S, WIN, ref, run_refusal

F32 = np.float32
GOLDEN_FILE = os.path.join(GOLDEN, "view_refusals.json")
NEW_EXPORTS = ["rc_view_check", "rc_render_view", "rc_render_view_device", "rc_trace_rays",
               "rc_trace_rays_device", "rc_view_phase_ms"]


# ------------------------------------------------------------------ the numpy contract --
@pytest.mark.parametrize("cam,size", [((2.0, 2.0), (64, 48)), ((0.7, 1.3), (16, 12)),
                                      ((2.0, 2.03125), (97, 61)), ((2000.0, 1e-3), (5, 3))])
def test_identity_is_the_plain_camera(cam, size):
    xy = rc.view_grid(*size)
    got = rc.view_dirs(*cam, size, xy, rc.view_identity())
    want = pc.primary_dirs(*cam, *size)
    assert got.dtype == F32 and (pc.bits32(got) == pc.bits32(want)).all()


@pytest.mark.parametrize("name", pc.GOLDEN_SCENES)
def test_identity_is_the_plain_camera_cuda(name):
    js = vc.scene(name).js
    got = rc.view_dirs(js.camera_width, js.camera_height, (64, 48), rc.view_grid(64, 48),
                       rc.view_identity(), cuda=True)
    want = sc.camera_dirs_cuda(js)
    assert (pc.bits32(got) == pc.bits32(want)).all()


def test_identity_matches_primary_dir_ref_on_huge_images():
    cam, pix, xy = sc.family_primary_dir()
    want, _ = sc.primary_dir_ref(cam, pix, xy)
    # family rows are (camera, size, pixel) triples: group them by camera and size
    cw = (-2.0 * cam[:, 0]).astype(F32)
    ch = (2.0 * cam[:, 1]).astype(F32)
    checked = 0
    for W, H in ((33554433, 33554431), (1023, 767), (1, 1)):
        for c_w, c_h in ((2.0, 2.0), (0.7, 1.3)):
            sel = ((cw == F32(c_w)) & (ch == F32(c_h)) & (pix[:, 0] == F32(c_w) / F32(W)) &
                   (pix[:, 1] == F32(c_h) / F32(H)) & (xy[:, 0] < W) & (xy[:, 1] < H))
            assert sel.sum() >= 32
            got = rc.view_dirs(c_w, c_h, (W, H), xy[sel].astype(np.int64), rc.view_identity())
            assert (pc.bits32(got) == pc.bits32(want[sel])).all(), (W, H, c_w, c_h)
            checked += int(sel.sum())
    assert checked >= 6 * 32


def test_matrix_is_applied_before_the_single_normalisation():
    xy = rc.view_grid(7, 5)
    plain = rc.view_dirs(2.0, 2.0, (7, 5), xy, rc.view_identity())
    back = rc.view_dirs(2.0, 2.0, (7, 5), xy, vc.VIEWS["back"])
    assert (pc.bits32(back) == pc.bits32(plain * F32([-1, 1, -1]))).all() and (back[:, 2] > 0).all()
    swap = rc.view_dirs(2.0, 2.0, (7, 5), xy, vc.VIEWS["swap"])
    # the double sum of squares is taken in another order, so only the unit length is common
    np.testing.assert_allclose(swap[:, [1, 0, 2]], plain, rtol=0, atol=2.0 ** -23)
    wide = rc.view_dirs(2.0, 2.0, (7, 5), xy, vc.VIEWS["wide"])
    np.testing.assert_allclose(np.linalg.norm(wide.astype(np.float64), axis=1), 1.0, atol=1e-7)
    assert (wide != plain).any()
    # a zero matrix: q = 0; the C port leaves it and the CUDA port divides by zero
    zero = np.zeros((3, 3), F32)
    assert not rc.view_dirs(2.0, 2.0, (7, 5), xy, zero).any()
    assert np.isnan(rc.view_dirs(2.0, 2.0, (7, 5), xy, zero, cuda=True)).all()


@pytest.mark.parametrize("name", pc.GOLDEN_SCENES)
def test_oracle_image_through_the_identity_view(name):
    img, stats = oracle_render(vc.scene(name), *vc.FULL, vc.DEPTH, "fast")
    got, zero, _ = vc.view_image(name, "identity", 1, "fast")
    np.testing.assert_array_equal(got, img)
    assert zero == stats["zero_normalize"]
    np.testing.assert_array_equal(vc.view_image(name, "identity", 1, "cuda")[0],
                                  oracle_render_cuda(vc.scene(name), *vc.FULL, vc.DEPTH))


def test_supersampled_identity_view_is_the_window_contract():
    img, _ = oracle_render(vc.scene("quadric"), 2 * vc.FULL[0], 2 * vc.FULL[1], vc.DEPTH, "fast")
    np.testing.assert_array_equal(vc.view_image("quadric", "identity", 2, "fast")[0],
                                  rc.box_downsample(img, 2))


@pytest.mark.parametrize("view", vc.ROTATED)
def test_rotated_views_are_not_vacuous(view):
    """Conditions on the inputs of tests/test_gpu_view.py, from the oracle: every rotated view's
    expected image has at least 20 % non-black pixels and differs from the identity image in at
    least 10 % of the pixels."""
    for name in ("simple", "reflection", "quadric"):
        img = vc.view_image(name, view, 1, "fast")[0]
        plain = vc.view_image(name, "identity", 1, "fast")[0]
        lit = img.any(axis=2).mean()
        differ = (img != plain).any(axis=2).mean()
        assert lit >= 0.20 and differ >= 0.10, (name, view, lit, differ)


def test_backward_view_bounces_off_the_mirror_behind_the_eye():
    for name in ("simple", "reflection", "quadric"):
        assert vc.view_image(name, "back", 1, "fast")[2]["bounce_iters"] == 0
    img, _, cnt = vc.view_image("mirror_behind", "back", 1, "fast")
    assert cnt["bounce_iters"] > 0 and img.any(axis=2).mean() >= 0.20


# ---------------------------------------------------------------------------- view_euler --
def test_view_euler():
    assert pc.bits32(rc.view_euler(0, 0, 0)).tolist() == pc.bits32(np.eye(3, dtype=F32)).tolist()
    assert pc.bits32(rc.view_identity()).tolist() == pc.bits32(np.eye(3, dtype=F32)).tolist()
    rng = np.random.default_rng(2323)
    for yaw, pitch, roll in rng.uniform(-np.pi, np.pi, (64, 3)):
        m = rc.view_euler(yaw, pitch, roll).astype(np.float64)
        assert m.shape == (3, 3)
        np.testing.assert_allclose(m @ m.T, np.eye(3), rtol=0, atol=1e-6)
        assert abs(np.linalg.det(m) - 1.0) <= 1e-6
    # a positive yaw turns the camera to the left, a positive pitch up
    fwd = np.array([0.0, 0.0, -1.0])
    assert (rc.view_euler(0.5, 0, 0) @ fwd)[0] < 0 and (rc.view_euler(0, 0.5, 0) @ fwd)[1] > 0
    assert rc.view_euler(0.3, 0.2).dtype == F32


# ------------------------------------------------------------------------------ refusals --
def VIEW(m=None):
    v = rc.RcView()
    for k, x in enumerate(np.eye(3).ravel() if m is None else np.asarray(m, float).ravel()):
        v.m[k] = x
    return v


def OUT(rgb8=None, rgb=None, hits=None, frame=0):
    return rc.RcRayOut(rgb8, rgb, hits, frame)


def _bad(k, x):
    m = np.eye(3).ravel()
    m[k] = x
    return VIEW(m)


GOODV = VIEW()
GOODW = WIN(64, 48, 8, 4)
_DIRS = np.zeros((4, 3), F32)
_RGB8 = np.zeros((4, 3), np.uint8)
DIRS = _DIRS.ctypes.data
RGB8 = _RGB8.ctypes.data
CASES = []


def case(tag, export, *args):
    CASES.append((f"{export}[{tag}]", export, args))


case("null", "rc_view_check", None)
for tag, v in {"nan": _bad(0, np.nan), "inf": _bad(4, np.inf), "neg_inf": _bad(8, -np.inf),
               "nan_off_diagonal": _bad(5, np.nan), "two_inf_nan": VIEW([np.inf] + [np.nan] * 8)}.items():
    case(tag, "rc_view_check", ref(v))


def view_pair(tag, opt, view=GOODV, win=GOODW, w=16, h=16):
    case(tag, "rc_render_view", S, ref(view), ref(win), w, h, ref(opt), HOST, None)
    case(tag, "rc_render_view_device", S, ref(view), ref(win), w, h, ref(opt), FAKE, None, None)


for tag, opt in {"ssaa3": O(ssaa=3), "ssaa-1": O(ssaa=-1), "thr_no_factor": O(ssaa=1, adaptive=16),
                 "ssaa4_adaptive": O(ssaa=4, adaptive=16), "parity": O("parity"),
                 "gpus2": O(gpus=2), "cuda_gpus2": O("cuda", gpus=2),
                 "two_adaptive_parity": O("parity", ssaa=4, adaptive=16),
                 "two_parity_gpus2": O("parity", gpus=2)}.items():
    view_pair(tag, opt)
view_pair("nan", O(), _bad(2, np.nan))
view_pair("two_gpus2_nan", O(gpus=2), _bad(2, np.nan))
view_pair("two_nan_outside", O(), _bad(2, np.nan), WIN(64, 48, 60, 4))
view_pair("outside", O(ssaa=2), GOODV, WIN(64, 48, 60, 4))
view_pair("no_window_w0", O(), GOODV, None, 0, 16)
view_pair("past_int", O("cuda", ssaa=4), GOODV, WIN(1 << 30, 48, 0, 0))
case("null_scene", "rc_render_view", None, ref(GOODV), None, 8, 8, ref(O()), HOST, None)
case("null_view", "rc_render_view", S, None, None, 8, 8, ref(O()), HOST, None)
case("null_opt", "rc_render_view_device", S, ref(GOODV), None, 8, 8, None, FAKE, None, None)
case("null_out", "rc_render_view_device", S, ref(GOODV), None, 8, 8, ref(O()), None, None, None)
case("two_null_parity", "rc_render_view", S, ref(GOODV), None, 8, 8, ref(O("parity")), None, None)


def rays_pair(tag, opt, n=4, out=None, dev_out=None):
    case(tag, "rc_trace_rays", S, ref(opt), n, DIRS, ref(OUT(rgb8=RGB8) if out is None else out))
    case(tag, "rc_trace_rays_device", S, ref(opt), n, FAKE,
         ref(OUT(rgb8=FAKE) if dev_out is None else dev_out), None)


for tag, opt in {"ssaa3": O(ssaa=3), "ssaa2": O(ssaa=2), "ssaa4_adaptive": O(ssaa=4, adaptive=16),
                 "parity": O("parity"), "gpus2": O(gpus=2),
                 "two_ssaa2_parity": O("parity", ssaa=2)}.items():
    rays_pair(tag, opt)
rays_pair("all_null", O(), 4, OUT(), OUT())
rays_pair("frame_cuda", O("cuda"), 4, OUT(hits=HOST, frame=1), OUT(hits=FAKE, frame=1))
rays_pair("n0", O(), 0)
rays_pair("n_neg", O("cuda"), -1)
rays_pair("n_past", O(), (1 << 24) + 1)
rays_pair("two_all_null_n0", O(), 0, OUT(), OUT())
rays_pair("two_frame_cuda_n0", O("cuda"), 0, OUT(hits=HOST, frame=1), OUT(hits=FAKE, frame=1))
rays_pair("two_gpus2_frame_cuda", O("cuda", gpus=2), 4, OUT(hits=HOST, frame=1),
          OUT(hits=FAKE, frame=1))
case("hits_unaligned", "rc_trace_rays_device", S, ref(O()), 4, FAKE, ref(OUT(hits=ODD)), None)
case("two_unaligned_n0", "rc_trace_rays_device", S, ref(O()), 0, FAKE, ref(OUT(hits=ODD)), None)
case("null_scene", "rc_trace_rays", None, ref(O()), 4, DIRS, ref(OUT(rgb8=RGB8)))
case("null_opt", "rc_trace_rays", S, None, 4, DIRS, ref(OUT(rgb8=RGB8)))
case("null_dirs", "rc_trace_rays", S, ref(O()), 4, None, ref(OUT(rgb8=RGB8)))
case("null_out", "rc_trace_rays_device", S, ref(O()), 4, FAKE, None, None)

assert len({c[0] for c in CASES}) == len(CASES), "duplicate case ids"


def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("cid,export,args", CASES, ids=[c[0] for c in CASES])
def test_refusal(cid, export, args):
    got = run_refusal(export, args)
    assert got["rc"] == -1
    assert got["stderr"].startswith("Error: rc_") and got["stderr"].count("\n") == 1
    assert got == golden()[cid]


def test_golden_has_no_stale_case():
    assert sorted(golden()) == sorted(c[0] for c in CASES)
    assert not _RGB8.any()      # no refused call wrote an output


def test_view_check():
    assert rc.view_check(rc.view_identity()) and rc.view_check(np.zeros(9))
    assert rc.view_check(vc.VIEWS["wide"]) and rc.view_check(np.full((3, 3), 3e38))
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(9):
            m = np.eye(3).ravel()
            m[k] = bad
            assert run_refusal("rc_view_check", [ctypes.byref(VIEW(m))])["rc"] == -1


def test_exports_and_layouts():
    for name in NEW_EXPORTS:
        assert name in rc.HIP_EXPORTS and hasattr(rc.hip_lib(), name), name
    assert ctypes.sizeof(rc.RcView) == 36 and ctypes.sizeof(rc.RcRayOut) == 32
    with pytest.raises(ValueError):
        rc.view_dirs(2.0, 2.0, (4, 4), np.zeros((3, 2)), rc.view_identity())     # float pixels
    with pytest.raises(ValueError):
        rc.view_dirs(2.0, 2.0, (4, 4), rc.view_grid(2, 2), np.eye(4))
    with pytest.raises(ValueError):
        rc.trace_rays(vc.scene("simple"), np.zeros((0, 3), F32))
    with pytest.raises(ValueError):
        rc.trace_rays(vc.scene("simple"), np.zeros((2, 3), F32), outputs=("depth",))


if __name__ == "__main__":       # record tests/golden/view_refusals.json
    with open(GOLDEN_FILE, "w") as f:
        json.dump({cid: run_refusal(export, args) for cid, export, args in CASES}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    print(f"recorded {len(CASES)} refusals in {GOLDEN_FILE}", file=sys.stderr)
