"""Rotated camera views on the GPU (rc_render_view*): a view frame is the box filter
of the CPU oracle's own bounce loop (rco_prim_shoot, rco_prim_shoot_cuda) along the directions of
the numpy contract rc.view_dirs, cropped to the window, byte for byte: no tolerance anywhere."""
import numpy as np
import pytest

import view_cases as vc
from helpers import rc

pytestmark = pytest.mark.gpu

FULL = vc.FULL
SCENES = ["simple", "reflection", "quadric"]
DEPTH = vc.DEPTH


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def windows():
    """(33, 17) at (0, 0), at (5, 3) (odd: a multiple neither of 8 nor of s) and flush right and
    bottom; and one pixel."""
    w, h = 33, 17
    return [((*FULL, 0, 0), w, h), ((*FULL, 5, 3), w, h), ((*FULL, FULL[0] - w, FULL[1] - h), w, h),
            ((*FULL, 41, 29), 1, 1)]


def gpu_view(torch, name, view, window, w, h, s, mode, timing=None, fill=0x5a):
    d_out = torch.full((h, w, 3), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc.render_view_device(vc.scene(name), vc.VIEWS[view], w, h, d_out.data_ptr(), window=window,
                          ssaa=s, depth=DEPTH, mode=mode, timing=timing)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def assert_not_vacuous(name, view, mode):
    """Conditions on the input, computed from the oracle: a rotated view's expected image has at
    least 20 % non-black pixels and differs from the identity image in at least 10 % of them."""
    if view == "identity":
        return
    img = vc.view_image(name, view, 1, mode)[0]
    plain = vc.view_image(name, "identity", 1, mode)[0]
    assert img.any(axis=2).mean() >= 0.20, (name, view, mode)
    assert (img != plain).any(axis=2).mean() >= 0.10, (name, view, mode)


def check_windows(torch, name, view, s, mode):
    want_full = vc.view_image(name, view, s, mode)[0]
    for win, w, h in windows():
        want = rc.window_crop(want_full, 1, win, w, h)
        got = gpu_view(torch, name, view, win, w, h, s, mode)
        np.testing.assert_array_equal(got, want, err_msg=f"{name} {view} {mode} s{s} {win} {w}x{h}")


# ---------------------------------------------------------------------------- 1. views --
@pytest.mark.parametrize("view", list(vc.VIEWS))
@pytest.mark.parametrize("name", SCENES)
def test_views_fast(name, view, torch):
    assert_not_vacuous(name, view, "fast")
    for s in (1, 2, 4):
        check_windows(torch, name, view, s, "fast")


def test_view_fast_s8(torch):
    check_windows(torch, "quadric", "yaw30", 8, "fast")


@pytest.mark.parametrize("view", list(vc.VIEWS))
@pytest.mark.parametrize("name", ["quadric", "reflection"])
def test_views_cuda(name, view, torch):
    assert_not_vacuous(name, view, "cuda")
    for s in (1, 4):
        check_windows(torch, name, view, s, "cuda")


def test_whole_image_without_a_window(torch):
    for mode in ("fast", "cuda"):
        got = gpu_view(torch, "quadric", "ypr", None, *FULL, 2, mode)
        np.testing.assert_array_equal(got, vc.view_image("quadric", "ypr", 2, mode)[0], err_msg=mode)


# ------------------------------------------------------------------------- 2. identity --
@pytest.mark.parametrize("mode", ["fast", "cuda"])
def test_identity_view_is_render_window(mode, torch):
    """Device against device: k_view with the identity and k_window store equal bytes."""
    for name in SCENES:
        for s in (1, 2, 4, 8):
            for win, w, h in windows():
                d_ref = torch.full((h, w, 3), 0xa5, dtype=torch.uint8, device="cuda")
                rc.render_window_device(vc.scene(name), win, w, h, d_ref.data_ptr(), ssaa=s,
                                        depth=DEPTH, mode=mode)
                torch.cuda.synchronize()
                got = gpu_view(torch, name, "identity", win, w, h, s, mode)
                np.testing.assert_array_equal(got, d_ref.cpu().numpy(),
                                              err_msg=f"{name} {mode} s{s} {win}")


# ------------------------------------------------------------- 3. a huge virtual image --
def oracle_pixels(name, view, full, xy):
    js = vc.scene(name).js
    d = rc.view_dirs(js.camera_width, js.camera_height, full, xy, vc.VIEWS[view])
    return vc.oracle_quant(vc.oracle_shoot(name, d, "fast")[0])


def find_edge(name, view, full):
    """A pixel (column, row) of the virtual image beside the largest colour step of a row under the
    view: the row is sampled at 4097 columns and the largest step between neighbours bisected down
    to one pixel (tests/test_gpu_window.py's search, through view_dirs)."""
    fw, fh = full
    for frac in (0.5, 0.45, 0.55, 0.4, 0.6):
        row = int(fh * frac)
        cols = np.linspace(0, fw - 1, 4097).astype(np.int64)
        rgb = oracle_pixels(name, view, full, np.stack([cols, np.full_like(cols, row)], 1))
        step = np.abs(np.diff(rgb.astype(np.int64), axis=0)).sum(axis=1)
        if step.max() == 0:
            continue
        k = int(step.argmax())
        lo, hi, c_lo = int(cols[k]), int(cols[k + 1]), rgb[k]
        while hi - lo > 1:
            mid = (lo + hi) // 2
            c_mid = oracle_pixels(name, view, full, np.array([[mid, row]]))[0]
            if (c_mid != c_lo).any():
                hi = mid
            else:
                lo, c_lo = mid, c_mid
        return hi, row
    raise AssertionError("every sampled row is flat")


def test_huge_virtual_image(torch):
    full = (33554433, 33554431)
    w, h = 33, 17
    col, row = find_edge("quadric", "yaw10", full)
    x0 = min(max(col - w // 2, 0), full[0] - w)
    y0 = min(max(row - h // 2, 0), full[1] - h)
    want = oracle_pixels("quadric", "yaw10", full, rc.view_grid(w, h, x0, y0)).reshape(h, w, 3)
    # a condition on the input, not a tolerance: the window looks at an edge
    assert len(np.unique(want.reshape(-1, 3), axis=0)) >= 2, (x0, y0)
    got = gpu_view(torch, "quadric", "yaw10", (*full, x0, y0), w, h, 1, "fast")
    np.testing.assert_array_equal(got, want, err_msg=str((x0, y0)))
    # flush in the far corner
    x0, y0 = full[0] - w, full[1] - h
    want = oracle_pixels("quadric", "yaw10", full, rc.view_grid(w, h, x0, y0)).reshape(h, w, 3)
    got = gpu_view(torch, "quadric", "yaw10", (*full, x0, y0), w, h, 1, "fast")
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------ 4. the host-pixmap entry --
def test_host_pixmap_entry_and_zero_normalize():
    win = (*FULL, 5, 3)
    for mode in ("fast", "cuda"):
        full, zero, _ = vc.view_image("quadric", "ypr", 4, mode)
        tim = {}
        got = rc.render_view(vc.scene("quadric"), vc.VIEWS["ypr"], 33, 17, window=win, ssaa=4,
                             depth=DEPTH, mode=mode, timing=tim)
        np.testing.assert_array_equal(got, rc.window_crop(full, 1, win, 33, 17), err_msg=mode)
        assert tim["kernel_ms"] > 0.0 and tim["total_ms"] >= tim["d2h_ms"] >= 0.0
        assert rc.view_phase_ms()["kernel"] == pytest.approx(tim["kernel_ms"])
    # the count: a light exactly on the hit point of the backward view's centre ray
    want, events, _ = vc.view_image("light_on_plane_behind", "back", 1, "fast", (5, 3))
    assert events > 0
    tim = {}
    got = rc.render_view(vc.scene("light_on_plane_behind"), vc.VIEWS["back"], 5, 3, depth=DEPTH,
                         timing=tim)
    np.testing.assert_array_equal(got, want)
    assert tim["zero_normalize"] == events, (tim, events)
    # and a window that does not hold the centre pixel reports none
    none = oracle_pixels("light_on_plane_behind", "back", (5, 3), rc.view_grid(2, 1, 0, 0))
    tim = {}
    got = rc.render_view(vc.scene("light_on_plane_behind"), vc.VIEWS["back"], 2, 1,
                         window=(5, 3, 0, 0), depth=DEPTH, timing=tim)
    np.testing.assert_array_equal(got, none.reshape(1, 2, 3))
    assert tim["zero_normalize"] == 0


# ------------------------------------------- 5. bounces with backward primary rays --
@pytest.mark.parametrize("mode", ["fast", "cuda"])
def test_backward_view_bounces(mode, torch):
    for name in SCENES:      # nothing behind the eye of the golden scenes bounces
        assert vc.view_image(name, "back", 1, "fast")[2]["bounce_iters"] == 0
    for s in (1, 2):
        want, _, cnt = vc.view_image("mirror_behind", "back", s, mode)
        assert cnt["bounce_iters"] > 0 and want.any(axis=2).mean() >= 0.20
        got = gpu_view(torch, "mirror_behind", "back", None, *FULL, s, mode)
        np.testing.assert_array_equal(got, want, err_msg=f"{mode} s{s}")
    # the same scene looked at forwards sees the sphere and the mirror behind does nothing
    want = vc.view_image("mirror_behind", "yaw10", 1, mode)[0]
    np.testing.assert_array_equal(gpu_view(torch, "mirror_behind", "yaw10", None, *FULL, 1, mode),
                                  want)


# --------------------------------------------------------------------------- 6. streams --
def test_views_on_two_streams(torch):
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    views = ["yaw10", "yaw30", "ypr", "back"]
    bufs = [torch.zeros((FULL[1], FULL[0], 3), dtype=torch.uint8, device="cuda") for _ in views]
    torch.cuda.synchronize()
    for k, v in enumerate(views):
        rc.render_view_device(vc.scene("quadric"), vc.VIEWS[v], *FULL, bufs[k].data_ptr(), ssaa=2,
                              depth=DEPTH, stream_ptr=streams[k % 2].cuda_stream)
    torch.cuda.synchronize()
    for v, buf in zip(views, bufs):
        np.testing.assert_array_equal(buf.cpu().numpy(), vc.view_image("quadric", v, 2, "fast")[0],
                                      err_msg=v)
