"""Windows of a virtual image on the GPU (rc_render_window*, rc_accum_pass_window_device): a
window is the crop of the image the CPU oracle produces at the virtual size, byte for byte, for
virtual images of 97 x 61 pixels and of 33 554 433 x 33 554 431: no tolerance anywhere."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import (ROOT, oracle_lib, oracle_render, oracle_render_cuda, rc, read_p3,
                     scene_path)

pytestmark = pytest.mark.gpu

SCENES = ["simple", "reflection", "quadric"]
FULL = (97, 61)
SIZES = [(1, 1), (7, 3), (33, 17), (64, 48)]
CUDA_SIZES = [(7, 3), (64, 48)]
FACTORS = [1, 2, 4, 8]
DEPTH = 6


@pytest.fixture(scope="module")
def scenes():
    return {n: rc.Scene.from_file(scene_path(n)) for n in SCENES}


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


_oracle = {}


def oracle_image(scenes, name, w, h, mode):
    """The oracle's w x h image at DEPTH: computed once per key, read-only."""
    key = (name, w, h, mode)
    if key not in _oracle:
        if mode == "cuda":
            img = oracle_render_cuda(scenes[name], w, h, DEPTH)
        else:
            img, stats = oracle_render(scenes[name], w, h, DEPTH, mode)
            assert stats["parity_defined"] == 1, key
        img.setflags(write=False)
        _oracle[key] = img
    return _oracle[key]


def virtual_image(scenes, name, s, mode, full=FULL):
    """V_s: the box filter of the oracle's s*full_w x s*full_h image."""
    key = (name, s, mode, full, "V")
    if key not in _oracle:
        img = rc.box_downsample(oracle_image(scenes, name, s * full[0], s * full[1], mode), s)
        img.setflags(write=False)
        _oracle[key] = img
    return _oracle[key]


def oracle_pixels(scene, W, H, pix):
    """Oracle per-pixel shade (rco_pixels), fast mode at DEPTH, of the pixels y*W + x of the W x H
    image: rgb and zero-normalize events."""
    lib = oracle_lib()
    lib.rco_pixels.argtypes = [ctypes.POINTER(rc.JsonDataT)] + [ctypes.c_int] * 4 + [
        ctypes.c_int64] + [ctypes.c_void_p] * 6
    pix = np.ascontiguousarray(pix, dtype=np.int64)
    n = len(pix)
    rgb = np.zeros((n, 3), np.uint8)
    cout = np.zeros((n, 3), np.float32)
    cls = np.zeros(n, np.uint8)
    z = np.zeros(n, np.int64)
    assert lib.rco_pixels(ctypes.byref(scene.js), W, H, DEPTH + 1, rc.MODES["fast"], n,
                          pix.ctypes.data, None, rgb.ctypes.data, cout.ctypes.data,
                          cls.ctypes.data, z.ctypes.data) == 0
    return rgb, z


def oracle_window(scene, window, w, h, s):
    """The expected window from rco_pixels alone: the s*w x s*h subsamples of the window in the
    s*full_w x s*full_h image, box-filtered; and their zero-normalize events."""
    fw, fh, x0, y0 = window
    ys, xs = np.mgrid[s * y0:s * (y0 + h), s * x0:s * (x0 + w)].astype(np.int64)
    rgb, z = oracle_pixels(scene, s * fw, s * fh, (ys * (s * fw) + xs).ravel())
    return rc.box_downsample(rgb.reshape(s * h, s * w, 3), s), int(z.sum())


def gpu_window(torch, scene, window, w, h, s, mode, stream=None, timing=None, fill=0x5a):
    d_out = torch.full((h, w, 3), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc.render_window_device(scene, window, w, h, d_out.data_ptr(), ssaa=s, depth=DEPTH, mode=mode,
                            stream_ptr=stream.cuda_stream if stream else None, timing=timing)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def origins(w, h):
    """(0, 0); (5, 3), odd: a multiple neither of 8 nor of s; flush right and bottom."""
    return [(0, 0), (5, 3), (FULL[0] - w, FULL[1] - h)]


# ---------------------------------------------------------------------------- 1. crops --
@pytest.mark.parametrize("mode", ["fast", "cuda"])
@pytest.mark.parametrize("scene", SCENES)
def test_crops(scene, mode, scenes, torch):
    for s in FACTORS:
        full = virtual_image(scenes, scene, s, mode)
        for w, h in (SIZES if mode == "fast" else CUDA_SIZES):
            for x0, y0 in origins(w, h):
                win = (*FULL, x0, y0)
                want = rc.window_crop(full, 1, win, w, h)
                got = gpu_window(torch, scenes[scene], win, w, h, s, mode)
                np.testing.assert_array_equal(got, want,
                                              err_msg=f"{scene} {mode} s{s} {w}x{h}+{x0}+{y0}")


def test_host_pixmap_entry(scenes):
    win = (*FULL, 5, 3)
    for mode in ("fast", "cuda"):
        want = rc.window_crop(virtual_image(scenes, "quadric", 4, mode), 1, win, 33, 17)
        tim = {}
        got = rc.render_window(scenes["quadric"], win, 33, 17, ssaa=4, depth=DEPTH, mode=mode,
                               timing=tim)
        np.testing.assert_array_equal(got, want, err_msg=mode)
        assert tim["kernel_ms"] > 0.0 and tim["total_ms"] >= tim["d2h_ms"] >= 0.0


# ------------------------------------------------------------------------- 2. identity --
@pytest.mark.parametrize("mode", ["fast", "cuda"])
def test_identity_window(mode, scenes, torch):
    w, h = 33, 17
    for name in SCENES:
        for s in FACTORS:
            d_ref = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
            rc.render_device(scenes[name], w, h, d_ref.data_ptr(), depth=DEPTH, mode=mode, ssaa=s)
            torch.cuda.synchronize()
            ref = d_ref.cpu().numpy()
            got = gpu_window(torch, scenes[name], (w, h, 0, 0), w, h, s, mode)
            tag = f"{name} {mode} s{s}"
            np.testing.assert_array_equal(got, ref, err_msg=tag)
            np.testing.assert_array_equal(
                got, rc.box_downsample(oracle_image(scenes, name, s * w, s * h, mode), s),
                err_msg=tag)


# ---------------------------------------------------------------------------- 3. tiles --
@pytest.mark.parametrize("s", [1, 4])
def test_tiles(s, scenes, torch):
    fw, fh = 64, 48
    tiles = rc.window_tiles(fw, fh, 24, 20)
    assert [t[1] for t in tiles[:3]] == [24, 24, 16] and tiles[-1][2] == 8
    for mode in ("fast", "cuda"):
        want = virtual_image(scenes, "quadric", s, mode, (fw, fh))
        img = np.zeros((fh, fw, 3), np.uint8)
        for win, w, h in tiles:
            img[win[3]:win[3] + h, win[2]:win[2] + w] = gpu_window(torch, scenes["quadric"], win,
                                                                  w, h, s, mode)
        np.testing.assert_array_equal(img, want, err_msg=f"{mode} s{s}")
    # the same tiles enqueued on two streams, with no wait between a stream's tiles
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for _, w, h in tiles]
    torch.cuda.synchronize()
    for k, (win, w, h) in enumerate(tiles):
        rc.render_window_device(scenes["quadric"], win, w, h, bufs[k].data_ptr(), ssaa=s,
                                depth=DEPTH, mode="fast",
                                stream_ptr=streams[k % 2].cuda_stream)
    torch.cuda.synchronize()
    img = np.zeros((fh, fw, 3), np.uint8)
    for (win, w, h), buf in zip(tiles, bufs):
        img[win[3]:win[3] + h, win[2]:win[2] + w] = buf.cpu().numpy()
    np.testing.assert_array_equal(img, virtual_image(scenes, "quadric", s, "fast", (fw, fh)))


# ------------------------------------------------------------- 4. huge virtual images --
def find_edge(scene, sw, sh):
    """A subsample (column, row) of the sw x sh image beside the largest colour step of a row:
    the row is sampled at 4097 columns, and the largest step between neighbours is bisected down
    to one pixel.  Rows at 0.5, 0.45, 0.55, 0.4, 0.6 of the height until one is not flat."""
    for frac in (0.5, 0.45, 0.55, 0.4, 0.6):
        row = int(sh * frac)
        cols = np.linspace(0, sw - 1, 4097).astype(np.int64)
        rgb, _ = oracle_pixels(scene, sw, sh, row * sw + cols)
        step = np.abs(np.diff(rgb.astype(np.int64), axis=0)).sum(axis=1)
        if step.max() == 0:
            continue
        k = int(step.argmax())
        lo, hi = int(cols[k]), int(cols[k + 1])
        c_lo = rgb[k]
        while hi - lo > 1:
            mid = (lo + hi) // 2
            c_mid = oracle_pixels(scene, sw, sh, [row * sw + mid])[0][0]
            if (c_mid != c_lo).any():
                hi = mid
            else:
                lo, c_lo = mid, c_mid
        return hi, row
    raise AssertionError("every sampled row is flat")


HUGE = [(1000003, 700001), (33554433, 33554431)]


@pytest.mark.parametrize("s", [1, 8])
@pytest.mark.parametrize("full", HUGE)
@pytest.mark.parametrize("scene", SCENES)
def test_huge_virtual_images(scene, full, s, scenes, torch):
    fw, fh = full
    w, h = 33, 17
    col, row = find_edge(scenes[scene], s * fw, s * fh)
    x0 = min(max(col // s - w // 2, 0), fw - w)
    y0 = min(max(row // s - h // 2, 0), fh - h)
    win = (fw, fh, x0, y0)
    want, _ = oracle_window(scenes[scene], win, w, h, s)
    # a condition on the input, not a tolerance: the window looks at an edge
    assert len(np.unique(want.reshape(-1, 3), axis=0)) >= 2, win
    got = gpu_window(torch, scenes[scene], win, w, h, s, "fast")
    np.testing.assert_array_equal(got, want, err_msg=f"{scene} {win} s{s}")
    # flush in the far corner
    win = (fw, fh, fw - w, fh - h)
    want, _ = oracle_window(scenes[scene], win, w, h, s)
    got = gpu_window(torch, scenes[scene], win, w, h, s, "fast")
    np.testing.assert_array_equal(got, want, err_msg=f"{scene} {win} s{s}")


# ------------------------------------------------------------------ 5. zero_normalize --
def test_zero_normalize_counts_the_windows_rays(tmp_path, torch):
    """A point light exactly on the hit point of the 5 x 3 image's centre ray (the plane-and-light
    scene of test_gpu.py's zero-normalize test): the window that holds pixel (2, 1) reports its
    events, the one that does not reports none.  The view plane is 5 x 3 instead of that test's
    2 x 2: there the pixel size 2 / 5 rounds as a float, the centre ray of the 5 x 3 image misses
    the light by 1e-7 and the oracle counts no event in either window; with a pixel size of
    exactly 1 the centre ray is (0, 0, -1) and the event is there."""
    path = tmp_path / "z.scene"
    path.write_text("camera, width: 5.0, height: 3.0\n"
                    "plane, normal: [0, 0, 1], diffuse_color: [0.3, 0.5, 0.7], "
                    "specular_color: [1, 1, 1], position: [0, 0, -5], reflectivity: 0.5\n"
                    "light, color: [4, 4, 4], radial-a2: 0.01, radial-a1: 0.0125, "
                    "radial-a0: 0.0125, position: [0, 0, -5]\n")
    sc = rc.Scene.from_file(str(path))
    counts = []
    for x0, y0 in ((2, 1), (0, 0)):
        win = (5, 3, x0, y0)
        want, events = oracle_window(sc, win, 2, 1, 1)
        tim = {}
        got = gpu_window(torch, sc, win, 2, 1, 1, "fast", timing=tim)
        np.testing.assert_array_equal(got, want, err_msg=str(win))
        assert tim["zero_normalize"] == events, (win, tim, events)
        counts.append(events)
    assert counts[0] > 0 and counts[1] == 0


# --------------------------------------------------- 6. accumulation through a window --
class State:
    """An accumulator and an image in device memory ([H, W, 4] int16 bits, [H, W, 3] uint8)."""

    def __init__(self, torch, w, h, fill=77):
        self.torch, self.w, self.h = torch, w, h
        self.d_acc = torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
        self.d_out = torch.full((h, w, 3), fill, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def run(self, scene, window, seq, first, count, t=0, reset=False, mode="fast"):
        if window is None:
            rc.accum_pass_device(scene, self.w, self.h, seq, first, count, self.d_acc.data_ptr(),
                                 self.d_out.data_ptr(), threshold=t, reset=reset, depth=DEPTH,
                                 mode=mode)
        else:
            rc.accum_pass_window_device(scene, window, self.w, self.h, seq, first, count,
                                        self.d_acc.data_ptr(), self.d_out.data_ptr(), threshold=t,
                                        reset=reset, depth=DEPTH, mode=mode)

    def read(self):
        self.torch.cuda.synchronize()
        return self.d_acc.cpu().numpy().view(np.uint16), self.d_out.cpu().numpy()


def check_state(st, acc, out, tag):
    got_acc, got_out = st.read()
    np.testing.assert_array_equal(got_acc, acc, err_msg=f"acc {tag}")
    np.testing.assert_array_equal(got_out, out, err_msg=f"out {tag}")


def window_big(scenes, name, g, window, w, h, mode):
    """The window's g*w x g*h samples: the crop of the oracle's g*full_w x g*full_h image."""
    big = oracle_image(scenes, name, g * window[0], g * window[1], mode)
    return rc.window_crop(big, g, window, w, h)


def check_window_passes(torch, scenes, name, mode, window, w, h):
    sc = scenes[name]
    g, pts = rc.SAMPLE_SEQS["hier4"]
    big = window_big(scenes, name, g, window, w, h, mode)
    acc, out = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8)
    st = State(torch, w, h)
    first = 0
    for upto in (1, 3, 5, 16):   # the prefixes hier4[0..1), [0..3), [0..5), [0..16)
        count = upto - first
        acc, out, active, sat = rc.accum_step(acc, out, big, g, pts[first:upto], 0,
                                              reset=first == 0)
        st.run(sc, window, "hier4", first, count, reset=first == 0, mode=mode)
        tag = f"{name} {mode} hier4[0..{upto}) {window}"
        check_state(st, acc, out, tag)
        assert rc.accum_stats() == {"passes": 1, "active_pixels": w * h, "saturated": 0,
                                    "rays": w * h * count}, tag
        first = upto
    # all of hier4 is the window of the ssaa = 4 image
    np.testing.assert_array_equal(
        out, rc.window_crop(virtual_image(scenes, name, 4, mode, window[:2]), 1, window, w, h))
    # rgss4 whole, in one reset pass
    g, pts = rc.SAMPLE_SEQS["rgss4"]
    acc, out, _, _ = rc.accum_step(acc, out, big, g, pts, 0, reset=True)
    st.run(sc, window, "rgss4", 0, 4, reset=True, mode=mode)
    check_state(st, acc, out, f"{name} {mode} rgss4 {window}")
    assert rc.accum_stats()["rays"] == 4 * w * h
    # a masked pass at t = 16 after a reset pass
    g, pts = rc.SAMPLE_SEQS["hier4"]
    acc, out, _, _ = rc.accum_step(acc, out, big, g, pts[:1], 0, reset=True)
    st.run(sc, window, "hier4", 0, 1, reset=True, mode=mode)
    acc, out, active, sat = rc.accum_step(acc, out, big, g, pts[1:4], 16)
    st.run(sc, window, "hier4", 1, 3, t=16, mode=mode)
    check_state(st, acc, out, f"{name} {mode} masked {window}")
    assert rc.accum_stats() == {"passes": 1, "active_pixels": active, "saturated": 0,
                                "rays": 3 * active}
    return active


@pytest.mark.parametrize("scene", SCENES)
def test_accumulation_through_a_window(scene, scenes, torch):
    active = check_window_passes(torch, scenes, scene, "fast", (*FULL, 5, 3), 33, 17)
    # a condition on the input: the masked pass took some pixels and left some (116 and 305 by
    # the oracle); the reflection scene has no edge in this window, its list is empty
    assert (active == 0) if scene == "reflection" else (0 < active < 33 * 17)
    check_window_passes(torch, scenes, scene, "fast", (*FULL, FULL[0] - 7, FULL[1] - 3), 7, 3)


def test_accumulation_through_a_window_cuda(scenes, torch):
    check_window_passes(torch, scenes, "quadric", "cuda", (*FULL, 5, 3), 33, 17)


@pytest.mark.parametrize("mode", ["fast", "cuda"])
def test_accumulation_identity_window(mode, scenes, torch):
    w, h = 33, 17
    sc = scenes["quadric"]
    a, b = State(torch, w, h), State(torch, w, h)
    for first, count, t, reset in ((0, 1, 0, True), (1, 4, 0, False), (5, 2, 16, False)):
        a.run(sc, None, "hier4", first, count, t=t, reset=reset, mode=mode)
        want_stats = rc.accum_stats()
        b.run(sc, (w, h, 0, 0), "hier4", first, count, t=t, reset=reset, mode=mode)
        assert rc.accum_stats() == want_stats
        acc, out = a.read()
        check_state(b, acc, out, f"{mode} [{first}, {first + count}) t{t}")
    assert (a.read()[0][:, :, 3] >= 5).all()


# ------------------------------------------------------------------------------ 7. pan --
def test_pan_keeps_the_overlap(scenes, torch):
    """Two windows of one virtual image, each given hier4[0..5) at t = 0: the overlap's records do
    not depend on the window, so the second state is the first moved by the pan plus the exposed
    strips, rendered as windows of their own."""
    sc = scenes["quadric"]
    w, h = 40, 24
    (ax, ay), (bx, by) = (5, 3), (17, 9)
    dx, dy = bx - ax, by - ay

    def state_of(x0, y0, sw, sh):
        st = State(torch, sw, sh)
        st.run(sc, (*FULL, x0, y0), "hier4", 0, 1, reset=True)
        st.run(sc, (*FULL, x0, y0), "hier4", 1, 4)
        return st.read()

    acc_a, out_a = state_of(ax, ay, w, h)
    acc_b, out_b = state_of(bx, by, w, h)
    assert (acc_a[:, :, 3] == 5).all() and (acc_b[:, :, 3] == 5).all()
    np.testing.assert_array_equal(acc_a[dy:, dx:], acc_b[:h - dy, :w - dx])
    np.testing.assert_array_equal(out_a[dy:, dx:], out_b[:h - dy, :w - dx])
    assert len(np.unique(out_a[dy:, dx:].reshape(-1, 3), axis=0)) > 1
    # the viewer's move: the overlap shifted by (-dx, -dy), then the two exposed strips
    acc, out = np.zeros_like(acc_a), np.zeros_like(out_a)
    acc[:h - dy, :w - dx], out[:h - dy, :w - dx] = acc_a[dy:, dx:], out_a[dy:, dx:]
    right = state_of(bx + w - dx, by, dx, h)            # dx columns, the window's full height
    acc[:, w - dx:], out[:, w - dx:] = right
    below = state_of(bx, by + h - dy, w - dx, dy)       # dy rows under the overlap
    acc[h - dy:, :w - dx], out[h - dy:, :w - dx] = below
    np.testing.assert_array_equal(acc, acc_b)
    np.testing.assert_array_equal(out, out_b)


# ---------------------------------------------------------------------- 8. environment --
def run_cli(tmp_path, name, **env_set):
    exe = os.path.join(ROOT, "raytracing-programs_amd", "bin", "raytrace")
    out = tmp_path / name
    env = dict(os.environ)
    for k in ("RAYCAST_MODE", "RAYCAST_DEPTH", "RAYCAST_SSAA", "RAYCAST_SSAA_ADAPTIVE",
              "RAYCAST_FILTER", "RAYCAST_PATTERN", "RAYCAST_GPUS", "RAYCAST_WINDOW"):
        env.pop(k, None)
    env.update(env_set)
    r = subprocess.run([exe, "33", "17", scene_path("quadric"), str(out)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return read_p3(str(out)), r.stderr


def test_cli_env(tmp_path, scenes):
    """RAYCAST_WINDOW reaches the kernel through raycast(): the drop-in CLI's 33 x 17 file is the
    window of the 97 x 61 image; in parity mode the variable is ignored with a warning."""
    got, err = run_cli(tmp_path, "win.ppm", RAYCAST_MODE="fast", RAYCAST_SSAA="2",
                       RAYCAST_WINDOW="97x61+5+3")
    assert got.shape == (17, 33, 3) and "Warning" not in err
    want = rc.window_crop(virtual_image(scenes, "quadric", 2, "fast"), 1, (*FULL, 5, 3), 33, 17)
    np.testing.assert_array_equal(got, want)
    got, err = run_cli(tmp_path, "par.ppm", RAYCAST_SSAA="2", RAYCAST_WINDOW="97x61+5+3")
    assert "Warning: RAYCAST_WINDOW" in err and "ignored" in err
    whole = rc.box_downsample(oracle_image(scenes, "quadric", 66, 34, "parity"), 2)
    np.testing.assert_array_equal(got, whole)
    assert (whole != want).any()


# --------------------------------------------------- 9. state of the other families --
def test_other_families_keep_their_state(scenes, torch):
    sc = scenes["simple"]
    w, h = 64, 48
    d_out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    st = State(torch, w, h)
    torch.cuda.synchronize()
    rc.render_pattern_device(sc, w, h, "rgss4", d_out.data_ptr(), threshold=16, depth=DEPTH,
                             mode="fast")
    pattern = rc.pattern_stats()
    assert 0 < pattern["refined_pixels"] < w * h
    rc.pattern_phase_ms()
    st.run(sc, None, "hier4", 0, 3, reset=True)
    accum = rc.accum_stats()
    assert accum == {"passes": 1, "active_pixels": w * h, "saturated": 0, "rays": 3 * w * h}
    # window frames: the pattern's spans go (one event set, one owner), every count stays
    for s in (1, 4):
        rc.render_window_device(sc, (97, 61, 5, 3), w, h, d_out.data_ptr(), ssaa=s, depth=DEPTH,
                                timing={})
    with pytest.raises(RuntimeError):
        rc.pattern_phase_ms()
    with pytest.raises(RuntimeError):
        rc.accum_phase_ms()
    assert rc.pattern_stats() == pattern and rc.accum_stats() == accum
    # and the other way round: a window frame's bytes are unchanged by the families' frames
    # around it, and an accumulation pass through a window answers as the family's last call
    before = gpu_window(torch, sc, (97, 61, 5, 3), w, h, 4, "fast")
    rc.render_pattern_device(sc, w, h, "rgss4", d_out.data_ptr(), threshold=0, depth=DEPTH,
                             mode="fast")
    st.run(sc, (97, 61, 5, 3), "hier4", 3, 2)
    assert rc.pattern_stats() == {"refined_pixels": w * h, "rays": 4 * w * h}
    assert rc.accum_stats() == {"passes": 1, "active_pixels": w * h, "saturated": 0,
                                "rays": 2 * w * h}
    ms = rc.accum_phase_ms()
    assert ms["mark"] == 0.0 and ms["shoot"] >= 0.0
    np.testing.assert_array_equal(gpu_window(torch, sc, (97, 61, 5, 3), w, h, 4, "fast"), before)
    np.testing.assert_array_equal(
        before, rc.window_crop(virtual_image(scenes, "simple", 4, "fast"), 1, (97, 61, 5, 3), w, h))
