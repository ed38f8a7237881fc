"""Accumulation through a free camera on the GPU (rc_accum_pass_camera_device,
rc_render_camera_accum).  Every comparison is exact: records and image bytes.  The
expectation is tests/camera_accum_cases.py's: the oracle's samples through each camera
(ray_cases.camera_samples, which tests/test_gpu_camera.py holds k_camera against) put through the
pass's contract in numpy (rc.accum_step, rc.accum_add).  tests/test_camera_accum.py checks on the
CPU that these inputs are not vacuous."""
import ctypes

import numpy as np
import pytest

import camera_accum_cases as cac
import ray_cases as rcs
from helpers import rc
from test_gpu_camera import eye_with_an_edge, first_sphere_centre

pytestmark = pytest.mark.gpu

DEPTH = cac.DEPTH
G, HIER4 = cac.G, cac.HIER4
IDENT_CAM = ((0.0, 0.0, 0.0), None)


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


class State:
    """An accumulator and its image in device memory, with `guard` bytes of 0x5a on either side of
    both."""

    def __init__(self, torch, w, h, fill=77, guard=64):
        self.torch, self.w, self.h, self.g = torch, w, h, guard
        self.raw_acc = torch.full((guard + h * w * 8 + guard,), 0x5a, dtype=torch.uint8,
                                  device="cuda")
        self.raw_out = torch.full((guard + h * w * 3 + guard,), 0x5a, dtype=torch.uint8,
                                  device="cuda")
        self.raw_acc[guard:guard + h * w * 8] = 0
        self.raw_out[guard:guard + h * w * 3] = fill
        self.acc_ptr, self.out_ptr = self.raw_acc.data_ptr() + guard, self.raw_out.data_ptr() + guard
        assert self.acc_ptr % 8 == 0
        torch.cuda.synchronize()

    def cam(self, scene, cams, window, seq, first, count, t=0, reset=False, stream=None):
        rc.accum_pass_camera_device(scene, cams, window, self.w, self.h, seq, first, count,
                                    self.acc_ptr, self.out_ptr, threshold=t, reset=reset,
                                    depth=DEPTH,
                                    stream_ptr=stream.cuda_stream if stream else None)

    def win(self, scene, window, seq, first, count, t=0, reset=False):
        if window is None:
            rc.accum_pass_device(scene, self.w, self.h, seq, first, count, self.acc_ptr,
                                 self.out_ptr, threshold=t, reset=reset, depth=DEPTH)
        else:
            rc.accum_pass_window_device(scene, window, self.w, self.h, seq, first, count,
                                        self.acc_ptr, self.out_ptr, threshold=t, reset=reset,
                                        depth=DEPTH)

    def read(self):
        self.torch.cuda.synchronize()
        g, h, w = self.g, self.h, self.w
        acc, out = self.raw_acc.cpu().numpy(), self.raw_out.cpu().numpy()
        for raw in (acc, out):
            assert (raw[:g] == 0x5a).all() and (raw[-g:] == 0x5a).all(), "guard bytes"
        return (acc[g:-g].view(np.uint16).reshape(h, w, 4).copy(),
                out[g:-g].reshape(h, w, 3).copy())


def check_state(st, acc, out, tag):
    got_acc, got_out = st.read()
    np.testing.assert_array_equal(got_acc, acc, err_msg=f"acc {tag}")
    np.testing.assert_array_equal(got_out, out, err_msg=f"out {tag}")


def dense_stats(w, h, count):
    return {"passes": 1, "active_pixels": w * h, "saturated": 0, "rays": w * h * count}


# ------------------------------------------------------------------ 1. one camera, dense --
def check_prefixes(torch, name, eye, m, window, size):
    sc, (w, h) = rcs.scene(name), size
    big = rcs.camera_samples(name, eye, m, G, size, window)[0]
    acc, out = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8)
    st = State(torch, w, h)
    first = 0
    for upto in cac.PREFIXES:
        count = upto - first
        acc, out, _, _ = rc.accum_step(acc, out, big, G, HIER4[first:upto], 0, reset=first == 0)
        st.cam(sc, (eye, m), window, "hier4", first, count, reset=first == 0)
        tag = f"{name} {eye} hier4[0..{upto}) {window}"
        check_state(st, acc, out, tag)
        assert rc.accum_stats() == dense_stats(w, h, count), tag
        first = upto
    # all of hier4 is the camera's ssaa = 4 image: the oracle's, and k_camera's bytes
    np.testing.assert_array_equal(out, rcs.camera_image(name, eye, m, 4, size, window))
    d_img = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    rc.render_camera_device(sc, eye, m, w, h, d_img.data_ptr(), window=window, ssaa=4, depth=DEPTH)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_img.cpu().numpy(), out)


@pytest.mark.parametrize("k", range(len(cac.DENSE)), ids=["in_sphere", "in_quadric", "eye_neg0"])
def test_one_camera_dense(k, torch):
    name, eye, m = cac.DENSE[k]
    check_prefixes(torch, name, eye, m, cac.WINDOW, cac.SIZE)
    check_prefixes(torch, name, eye, m, cac.CORNER, cac.CORNER_SIZE)


# ------------------------------------------------------------------------------ 2. origin --
def test_origin_camera_is_the_window_accumulation(torch):
    """Eye +0 with the identity view: the general nearest at +0 gives the records, the bytes and
    the stats of the reference camera's kernels, device against device."""
    sc, (w, h) = rcs.scene("quadric"), cac.SIZE
    passes = ((0, 1, 0, True), (1, 4, 0, False), (5, 11, 0, False), (0, 3, 16, False))
    for window in (cac.WINDOW, None):
        a, b = State(torch, w, h), State(torch, w, h)
        for first, count, t, reset in passes:
            a.win(sc, window, "hier4", first, count, t=t, reset=reset)
            want_stats = rc.accum_stats()
            b.cam(sc, IDENT_CAM, window, "hier4", first, count, t=t, reset=reset)
            tag = f"{window} [{first}, {first + count}) t{t}"
            assert rc.accum_stats() == want_stats, tag
            check_state(b, *a.read(), tag)
        acc = a.read()[0]
        assert (acc[:, :, 3] >= 16).all() and 0 < want_stats["active_pixels"] < w * h


# ---------------------------------------------------------------- 3. one camera a sample --
def test_one_camera_a_sample(torch):
    sc, (w, h) = rcs.scene(cac.LENS_SCENE), cac.SIZE
    zero = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8)
    # a reset pass through the centre, then five lens cameras for samples 3..7: camera j belongs
    # to sample 3 + j, not to camera 3 + j
    acc, out, _, _ = rc.accum_add(*zero, cac.planes(cac.LENS_SCENE, cac.LENS[:1], HIER4[:3]), 0,
                                  reset=True)
    acc5, out5, _, _ = rc.accum_add(acc, out, cac.planes(cac.LENS_SCENE, cac.LENS[:5], HIER4[3:8]))
    st = State(torch, w, h)
    st.cam(sc, cac.LENS[0], cac.WINDOW, "hier4", 0, 3, reset=True)
    check_state(st, acc, out, "lens centre, hier4[0..3)")
    st.cam(sc, cac.LENS[:5], cac.WINDOW, "hier4", 3, 5)
    assert rc.accum_stats() == dense_stats(w, h, 5)
    check_state(st, acc5, out5, "five lens cameras, hier4[3..8)")
    # one pass of 5 with cams[5] is five passes of 1 with cams[j], record for record
    one = State(torch, w, h)
    one.cam(sc, cac.LENS[0], cac.WINDOW, "hier4", 0, 3, reset=True)
    for j in range(5):
        one.cam(sc, cac.LENS[j], cac.WINDOW, "hier4", 3 + j, 1)
    check_state(one, *st.read(), "five passes of one")
    # 16 cameras in one pass
    acc, out, _, _ = rc.accum_add(*zero, cac.planes(cac.LENS_SCENE, cac.LENS, HIER4), 0, reset=True)
    st.cam(sc, cac.LENS, cac.WINDOW, "hier4", 0, 16, reset=True)
    assert rc.accum_stats() == dense_stats(w, h, 16)
    check_state(st, acc, out, "16 lens cameras")
    assert (out != rcs.camera_image(cac.LENS_SCENE, *cac.LENS[0], 4, cac.SIZE, cac.WINDOW)).any()


# ------------------------------------------------------------------------- 4. masked pass --
def test_masked_pass(torch):
    name, eye, m = cac.MASKED
    sc, (w, h) = rcs.scene(name), cac.SIZE
    acc0, out0, acc1, out1, active = cac.masked_pass()
    assert 0 < active < w * h
    st = State(torch, w, h)
    st.cam(sc, (eye, m), cac.WINDOW, "hier4", 0, 1, reset=True)
    check_state(st, acc0, out0, "reset")
    st.cam(sc, (eye, m), cac.WINDOW, "hier4", 1, 3, t=cac.MASK_T)
    assert rc.accum_stats() == {"passes": 1, "active_pixels": active, "saturated": 0,
                                "rays": 3 * active}
    check_state(st, acc1, out1, "masked")                # read() checks the guard bytes
    got_acc, got_out = st.read()
    outside = ~rc.edge_mask(out0, cac.MASK_T)
    assert outside.sum() == w * h - active
    assert (got_acc[outside] == acc0[outside]).all() and (got_out[outside] == out0[outside]).all()
    assert (got_acc[~outside][:, 3] == 4).all()
    # a masked pass with a camera a sample, over the state as it stands
    lens = cac.LENS[5:8]
    acc2, out2, active2, _ = rc.accum_add(acc1, out1, cac.planes(name, lens, HIER4[4:7]),
                                          cac.MASK_T)
    st.cam(sc, lens, cac.WINDOW, "hier4", 4, 3, t=cac.MASK_T)
    assert rc.accum_stats()["active_pixels"] == active2 and 0 < active2 < w * h
    check_state(st, acc2, out2, "masked, three lens cameras")


# -------------------------------------------------------------------------- 5. saturation --
def test_saturation(torch):
    name, eye, m = cac.MASKED
    sc, (w, h), window = rcs.scene(name), (9, 5), (*cac.FULL, 10, 3)    # a window with an edge
    pl = cac.planes(name, [(eye, m)], HIER4, (w, h), window)
    acc, out = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8)
    st = State(torch, w, h)
    for k in range(16):
        acc, out, _, sat = rc.accum_add(acc, out, pl, 0, reset=k == 0)
        st.cam(sc, (eye, m), window, "hier4", 0, 16, reset=k == 0)
        assert sat == 0
    assert (acc[:, :, 3] == 256).all()
    check_state(st, acc, out, "16 passes of 16")
    assert rc.accum_stats() == dense_stats(w, h, 16)
    st.cam(sc, (eye, m), window, "hier4", 0, 16)
    assert rc.accum_stats() == {"passes": 1, "active_pixels": 45, "saturated": 45, "rays": 0}
    check_state(st, acc, out, "the 17th pass")
    st.cam(sc, (eye, m), window, "hier4", 3, 1, t=1)          # the listed kernel saturates too
    stats = rc.accum_stats()
    assert stats["saturated"] == stats["active_pixels"] > 0 and stats["rays"] == 0
    check_state(st, acc, out, "a masked pass on a saturated state")


# ---------------------------------------------------------------------- 6. unstaged scene --
@pytest.mark.parametrize("name", ["random65", "quadric40"])
def test_scene_too_large_to_stage(name, torch):
    """More shapes than the LDS copy of the scene holds: one dense pass and one masked pass.
    random65 is the 65-shape scene of tests/test_gpu_camera.py, from its first sphere's centre; it
    is black from every eye, so its masked pass lists nothing.  quadric40 (camera_accum_cases) is
    lit, and its masked pass takes some pixels and leaves some."""
    if name == "quadric40":
        assert cac.lit_unstaged_scene() == name
    sc, (w, h) = rcs.scene(name), cac.SIZE
    assert sc.num_shapes + 1 > 32
    cam = ((first_sphere_centre(sc.js), rc.view_euler(0.2, 0.1)) if name == "random65"
           else cac.MASKED[1:])
    ids = rcs.camera_samples(name, *cam, 1, cac.SIZE, cac.WINDOW)[2]
    assert (ids >= 0).mean() >= 0.30 and (name == "random65" or len(np.unique(ids)) >= 3)
    zero = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8)
    acc, out, _, _ = rc.accum_add(*zero, cac.planes(name, [cam], HIER4[:3]), 0, reset=True)
    st = State(torch, w, h)
    st.cam(sc, cam, cac.WINDOW, "hier4", 0, 3, reset=True)
    check_state(st, acc, out, "dense")
    assert rc.accum_stats() == dense_stats(w, h, 3)
    acc, out, active, _ = rc.accum_add(acc, out, cac.planes(name, [cam], HIER4[3:5]), 16)
    assert (active == 0) if name == "random65" else (0 < active < w * h)
    st.cam(sc, cam, cac.WINDOW, "hier4", 3, 2, t=16)
    assert rc.accum_stats() == {"passes": 1, "active_pixels": active, "saturated": 0,
                                "rays": 2 * active}
    check_state(st, acc, out, "masked")


# ------------------------------------------------------------------ 7. huge virtual image --
def test_window_of_a_huge_virtual_image(torch):
    full, at, size = (33554433, 33554431), (33554000, 1000003), (40, 24)
    win = (*full, *at)
    eye = eye_with_an_edge("quadric", win, size, (-2.0, -2.0, 1.0), (-6.0, -5.0, 0.0))
    g, pts = rc.SAMPLE_SEQS["hier2"]
    w, h = size
    acc, out = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8)
    st = State(torch, w, h)
    for first, count in ((0, 1), (1, 3)):
        pl = cac.planes("quadric", [(eye, rcs.IDENT)], pts[first:first + count], size, win, g)
        acc, out, _, _ = rc.accum_add(acc, out, pl, 0, reset=first == 0)
        st.cam(rcs.scene("quadric"), (eye, rcs.IDENT), win, "hier2", first, count,
               reset=first == 0)
        check_state(st, acc, out, f"hier2[{first}, {first + count}) {eye}")
    want = rcs.camera_image("quadric", eye, rcs.IDENT, 2, size, win)
    assert len(np.unique(want.reshape(-1, 3), axis=0)) >= 2, eye      # the window looks at an edge
    np.testing.assert_array_equal(out, want)


# ----------------------------------------------------------------------------- 8. streams --
def test_two_states_on_two_streams(torch):
    """Two passes of 16 through different cameras enqueued back to back on two streams, each into
    its own state: the cameras are the launch's argument, nothing is shared between the two."""
    sc, (w, h) = rcs.scene("quadric"), cac.SIZE
    cams = [rcs.CAMERAS[8][1:], cac.LENS[1:] + cac.LENS[:1]]         # one camera; 16 lens cameras
    serial = []
    for c in cams:
        st = State(torch, w, h)
        st.cam(sc, c, cac.WINDOW, "hier4", 0, 16, reset=True)
        serial.append(st.read())
    assert (serial[0][0] != serial[1][0]).any()
    zero = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8)
    want, _, _, _ = rc.accum_add(*zero, cac.planes("quadric", cams[1], HIER4), 0, reset=True)
    np.testing.assert_array_equal(serial[1][0], want)
    states = [State(torch, w, h), State(torch, w, h)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(2):
        for st, c, s in zip(states, cams, streams):
            st.cam(sc, c, cac.WINDOW, "hier4", 0, 16, reset=True, stream=s)
    for st, ref in zip(states, serial):
        check_state(st, *ref, "two streams")


# --------------------------------------------------------------------------- 9. host form --
def test_host_form():
    sc, size = rcs.scene("quadric"), (37, 29)
    eye, m = (0.5, 0.25, 1.0), rc.view_euler(0.1, -0.05)
    want = rcs.camera_image("quadric", eye, m, 2, size)
    assert want.any(axis=2).mean() >= 0.30
    tim = {}
    got = rc.render_camera_accum(sc, (eye, m), *size, "hier2", depth=DEPTH, timing=tim)
    np.testing.assert_array_equal(got, want)
    assert rc.accum_stats() == {"passes": 1, "active_pixels": 37 * 29, "saturated": 0,
                                "rays": 4 * 37 * 29}
    assert tim["total_ms"] > 0.0
    g, pts = rc.SAMPLE_SEQS["hier2"]
    lens = rc.thin_lens(eye, m, cac.LENS_FOCUS, cac.lens_points(4))
    zero = np.zeros((29, 37, 4), np.uint16), np.zeros((29, 37, 3), np.uint8)
    _, want4, _, _ = rc.accum_add(*zero, cac.planes("quadric", lens, pts, size, None, g), 0,
                                  reset=True)
    assert (want4 != want).any()
    np.testing.assert_array_equal(rc.render_camera_accum(sc, lens, *size, "hier2", depth=DEPTH),
                                  want4)
    # a window, and a sequence of more than one chunk: hier8's 64 samples are the ssaa = 8 image
    win = (*cac.FULL, 50, 40)
    got = rc.render_camera_accum(sc, (eye, m), 9, 5, "hier8", window=win, depth=DEPTH)
    np.testing.assert_array_equal(got, rcs.camera_image("quadric", eye, m, 8, (9, 5), win))
    assert rc.accum_stats()["passes"] == 4 and rc.accum_stats()["rays"] == 64 * 45


# ---------------------------------------------------------------------- 10. live refusals --
def test_refusals_leave_device_buffers_untouched(torch):
    """The messages are pinned in tests/golden/camera_accum_refusals.json (tests/test_camera_accum.py,
    which runs without a GPU); here every kind of refusal meets real device buffers."""
    sc, (w, h) = rcs.scene("simple"), (16, 16)
    cam = ((0.5, 0.25, 1.0), None)
    d_acc = torch.full((h, w, 8), 0x5a, dtype=torch.uint8, device="cuda")
    d_out = torch.full((h, w, 3), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a, o = d_acc.data_ptr(), d_out.data_ptr()

    def refused(cams=cam, window=None, seq="hier4", first=0, count=1, acc=a, out=o, **kw):
        with pytest.raises(RuntimeError):
            rc.accum_pass_camera_device(sc, cams, window, w, h, seq, first, count, acc, out, **kw)

    refused(acc=0)
    refused(out=0)
    refused(acc=a + 4)
    for mode in ("cuda", "parity"):
        refused(mode=mode)
    refused(threshold=256)
    refused(threshold=16, reset=True)
    refused(window=(64, 48, 60, 40))
    refused(first=16)
    refused(count=17)
    for bad in (np.nan, np.inf, -np.inf):
        refused(((0.0, bad, 0.0), None))
        refused([cam, ((0.5, 0.25, 1.0), np.diag([1.0, bad, 1.0]))], count=2)
    # the number of cameras: the Python side raises ValueError first, so through the C entry
    arr = rc._rc_cameras([cam, cam], 2, "test")
    opt, seq = rc.options(DEPTH, "fast"), rc._rc_sample_seq("hier4")
    assert rc.hip_lib().rc_accum_pass_camera_device(
        sc.packed(), arr, 2, None, w, h, ctypes.byref(opt), ctypes.byref(seq), 0, 3, 0, 1,
        ctypes.c_void_p(a), ctypes.c_void_p(o), None, None) == -1
    pix = np.full((h, w, 3), 0x5a, np.uint8)
    for kw in ({"mode": "cuda"}, {"window": (64, 48, 60, 40)}):
        with pytest.raises(RuntimeError):
            rc.render_camera_accum(sc, cam, w, h, "hier2", out=pix, **kw)
    with pytest.raises(RuntimeError):
        rc.render_camera_accum(sc, ((np.nan, 0, 0), None), w, h, "hier2", out=pix)
    torch.cuda.synchronize()
    assert (d_acc.cpu().numpy() == 0x5a).all() and (d_out.cpu().numpy() == 0x5a).all()
    assert (pix == 0x5a).all()


# ------------------------------------------ 11. state of the other families (§15) --
def test_other_families_keep_their_bytes(torch):
    """A window accumulation pass and a camera frame give the same bytes (and the former the same
    stats) after the new calls as before them."""
    sc, (w, h) = rcs.scene("quadric"), cac.SIZE
    eye, m = rcs.CAMERAS[11][1:]

    def others():
        st = State(torch, w, h)
        st.win(sc, cac.WINDOW, "hier4", 0, 3, reset=True)
        st.win(sc, cac.WINDOW, "hier4", 3, 2, t=16)
        acc, out = st.read()
        stats = rc.accum_stats()
        img = rc.render_camera(sc, eye, m, w, h, window=cac.WINDOW, ssaa=2, depth=DEPTH)
        view_ms = rc.view_phase_ms()
        assert view_ms["kernel"] > 0.0
        return acc, out, stats, img

    before = others()
    st = State(torch, w, h)
    st.cam(sc, cac.LENS, cac.WINDOW, "hier4", 0, 16, reset=True)
    st.cam(sc, (eye, m), cac.WINDOW, "hier4", 0, 2, t=16)
    ms = rc.accum_phase_ms()                       # the new passes record the family's spans
    assert sorted(ms) == ["mark", "shoot"] and ms["mark"] > 0.0 and ms["shoot"] > 0.0
    rc.render_camera_accum(sc, (eye, m), w, h, "hier2", depth=DEPTH)
    assert rc.accum_phase_ms()["mark"] == 0.0
    after = others()
    for a, b in zip(before[:2] + before[3:], after[:2] + after[3:]):
        np.testing.assert_array_equal(a, b)
    assert before[2] == after[2]
