"""Scrolling an accumulated view on the GPU (rc_accum_scroll_device): the destination state is
the source moved where the two windows overlap and freshly accumulated where the pan exposed
pixels, record for record and byte for byte: the state the device builds from scratch through the
new window, and the numpy model on the CPU oracle's image.  No tolerance anywhere.  Every
destination is pre-filled with 0x5a5a / 0x5a, so a pixel nobody stored to shows.

Where the old window of a case would lie outside the virtual image (it is no argument of the
call), the source is a state of another valid window: the contract moves the kept records
whatever their history, and the expectation is the model's on the source as it was read back."""
import numpy as np
import pytest

from helpers import rc, scene_path
from test_gpu_window import (DEPTH, FULL, SCENES, find_edge, oracle_image, oracle_pixels,
                             virtual_image, window_big)

pytestmark = pytest.mark.gpu

PANS = [(12, 6), (-5, 0), (0, -3), (-4, 5), (0, 0), (40, 0), (-60, 30)]
CASES = [("simple", "fast"), ("reflection", "fast"), ("quadric", "fast"), ("quadric", "cuda")]


@pytest.fixture(scope="module")
def scenes():
    return {n: rc.Scene.from_file(scene_path(n)) for n in SCENES}


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def exposed_count(w, h, dx, dy):
    return w * h - max(0, w - abs(dx)) * max(0, h - abs(dy))


def clamped(window, w, h, dx, dy):
    """The window after the pan, clamped into the virtual image."""
    fw, fh, x0, y0 = window
    return fw, fh, min(max(x0 + dx, 0), fw - w), min(max(y0 + dy, 0), fh - h)


class State:
    """An accumulator and an image in device memory ([H, W, 4] int16 bits, [H, W, 3] uint8)."""

    def __init__(self, torch, w, h, acc_fill=0x5a5a, out_fill=0x5a):
        self.torch, self.w, self.h = torch, w, h
        self.d_acc = torch.full((h, w, 4), acc_fill, dtype=torch.int16, device="cuda")
        self.d_out = torch.full((h, w, 3), out_fill, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    def run(self, scene, window, seq, first, count, t=0, reset=False, mode="fast", stream=None):
        rc.accum_pass_window_device(scene, window, self.w, self.h, seq, first, count,
                                    self.d_acc.data_ptr(), self.d_out.data_ptr(), threshold=t,
                                    reset=reset, depth=DEPTH, mode=mode,
                                    stream_ptr=stream.cuda_stream if stream else None)

    def built(self, scene, window, seq, upto, mode="fast"):
        """A reset pass [0, 1) and, for upto > 1, a pass [1, upto)."""
        self.run(scene, window, seq, 0, 1, reset=True, mode=mode)
        if upto > 1:
            self.run(scene, window, seq, 1, upto - 1, mode=mode)
        return self

    def scrolled(self, scene, window, seq, count, dx, dy, mode="fast", stream=None, timing=None):
        """A fresh destination state: this one scrolled by (dx, dy) into `window`."""
        dst = State(self.torch, self.w, self.h)
        rc.accum_scroll_device(scene, window, self.w, self.h, seq, count, dx, dy,
                               self.d_acc.data_ptr(), self.d_out.data_ptr(), dst.d_acc.data_ptr(),
                               dst.d_out.data_ptr(), depth=DEPTH, mode=mode, timing=timing,
                               stream_ptr=stream.cuda_stream if stream else None)
        return dst

    def read(self):
        self.torch.cuda.synchronize()
        return self.d_acc.cpu().numpy().view(np.uint16), self.d_out.cpu().numpy()


def check(st, acc, out, tag):
    got_acc, got_out = st.read()
    np.testing.assert_array_equal(got_acc, acc, err_msg=f"acc {tag}")
    np.testing.assert_array_equal(got_out, out, err_msg=f"out {tag}")


def stats_of(exposed, count):
    if exposed == 0:
        return {"passes": 0, "active_pixels": 0, "saturated": 0, "rays": 0}
    return {"passes": (count + 15) // 16, "active_pixels": exposed, "saturated": 0,
            "rays": exposed * count}


# -------------------------------------------------------------------------- 1. scrolls --
@pytest.mark.parametrize("scene,mode", CASES, ids=[f"{s}-{m}" for s, m in CASES])
def test_scrolls(scene, mode, scenes, torch):
    sc = scenes[scene]
    w, h = 40, 24
    old = (*FULL, 5, 3)
    g, pts = rc.SAMPLE_SEQS["hier4"]
    src = State(torch, w, h).built(sc, old, "hier4", 5, mode)
    src_acc, src_out = src.read()
    assert (src_acc[:, :, 3] == 5).all()
    for dx, dy in PANS:
        new = clamped(old, w, h, dx, dy)   # a clamp only for (-60, 30): nothing is kept there
        tag = f"{scene} {mode} pan ({dx}, {dy}) {new}"
        dst = src.scrolled(sc, new, "hier4", 5, dx, dy, mode)
        exposed = exposed_count(w, h, dx, dy)
        assert rc.accum_stats() == stats_of(exposed, 5), tag
        got_acc, got_out = dst.read()
        scratch_acc, scratch_out = State(torch, w, h).built(sc, new, "hier4", 5, mode).read()
        np.testing.assert_array_equal(got_acc, scratch_acc, err_msg=f"acc, the device, {tag}")
        np.testing.assert_array_equal(got_out, scratch_out, err_msg=f"out, the device, {tag}")
        acc, out, e = rc.accum_scroll(src_acc, src_out, window_big(scenes, scene, g, new, w, h, mode),
                                      g, pts[:5], dx, dy)
        assert e == exposed
        np.testing.assert_array_equal(got_acc, acc, err_msg=f"acc, the model, {tag}")
        np.testing.assert_array_equal(got_out, out, err_msg=f"out, the model, {tag}")
        check(src, src_acc, src_out, f"the source after {tag}")


# -------------------------------------- 2. shapes where the index mapping can go wrong --
@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (33, 17), (64, 48)])
def test_shapes(w, h, scenes, torch):
    """The source is a state of the window at (5, 3) (or (0, 0) where that does not fit) with 3
    samples a pixel and the scroll takes 2, so a kept record and an exposed one differ in n."""
    sc = scenes["quadric"]
    g, pts = rc.SAMPLE_SEQS["hier4"]
    some = (*FULL, min(5, FULL[0] - w), min(3, FULL[1] - h))
    src = State(torch, w, h).built(sc, some, "hier4", 3)
    src_acc, src_out = src.read()
    for x0, y0 in ((0, 0), (FULL[0] - w, FULL[1] - h)):
        new = (*FULL, x0, y0)
        big = window_big(scenes, "quadric", g, new, w, h, "fast")
        for dx, dy in ((1, 0), (0, 1), (-1, -1), (w - 1, h - 1), (-(w - 1), 0),
                       (-2 ** 31, 2 ** 31 - 1)):   # and the ends of int: nothing is kept
            tag = f"{w}x{h} {new} pan ({dx}, {dy})"
            dst = src.scrolled(sc, new, "hier4", 2, dx, dy)
            assert rc.accum_stats() == stats_of(exposed_count(w, h, dx, dy), 2), tag
            acc, out, _ = rc.accum_scroll(src_acc, src_out, big, g, pts[:2], dx, dy)
            check(dst, acc, out, tag)
    check(src, src_acc, src_out, "the source")


# --------------------------------------------------------------------------- 3. chunks --
def test_chunks(scenes, torch):
    sc = scenes["quadric"]
    w, h, dx, dy = 33, 17, 3, 2
    old, new = (*FULL, 5, 3), (*FULL, 8, 5)
    g, pts = rc.SAMPLE_SEQS["hier8"]
    big = window_big(scenes, "quadric", g, new, w, h, "fast")
    src = State(torch, w, h).built(sc, old, "hier8", 2)
    src_acc, src_out = src.read()
    exposed = exposed_count(w, h, dx, dy)
    for count, passes in ((1, 1), (16, 1), (17, 2), (64, 4)):
        dst = src.scrolled(sc, new, "hier8", count, dx, dy)
        assert rc.accum_stats() == {"passes": passes, "active_pixels": exposed, "saturated": 0,
                                    "rays": exposed * count}, count
        acc, out, _ = rc.accum_scroll(src_acc, src_out, big, g, pts[:count], dx, dy)
        check(dst, acc, out, f"count {count}")
    # all of hier8: the exposed pixels' bytes are the window of the ssaa = 8 image
    want = rc.window_crop(virtual_image(scenes, "quadric", 8, "fast"), 1, new, w, h)
    np.testing.assert_array_equal(out[h - dy:], want[h - dy:])
    np.testing.assert_array_equal(out[:, w - dx:], want[:, w - dx:])
    assert (acc[h - dy:, :, 3] == 64).all() and (acc[:, w - dx:, 3] == 64).all()


# -------------------------------------------------------------------- 4. verbatim move --
def test_kept_records_move_verbatim(scenes, torch):
    sc = scenes["quadric"]
    w, h, dx, dy = 33, 17, 3, 2
    old, new = (*FULL, 5, 3), (*FULL, 8, 5)
    g, pts = rc.SAMPLE_SEQS["hier4"]
    src = State(torch, w, h)
    src.run(sc, old, "hier4", 0, 1, reset=True)
    src.run(sc, old, "hier4", 1, 3, t=16)
    active = rc.accum_stats()["active_pixels"]
    # a condition on the input: the masked pass took some pixels and left some
    assert 0 < active < w * h
    src_acc, src_out = src.read()
    assert sorted(np.unique(src_acc[:, :, 3])) == [1, 4]
    dst = src.scrolled(sc, new, "hier4", 2, dx, dy)
    got_acc, got_out = dst.read()
    np.testing.assert_array_equal(got_acc[:h - dy, :w - dx], src_acc[dy:, dx:])
    np.testing.assert_array_equal(got_out[:h - dy, :w - dx], src_out[dy:, dx:])
    assert len(np.unique(got_acc[:h - dy, :w - dx, 3])) == 2
    assert (got_acc[h - dy:, :, 3] == 2).all() and (got_acc[:, w - dx:, 3] == 2).all()
    acc, out, _ = rc.accum_scroll(src_acc, src_out,
                                  window_big(scenes, "quadric", g, new, w, h, "fast"), g, pts[:2],
                                  dx, dy)
    check(dst, acc, out, "masked source")


# --------------------------------------------------------------- 5. huge virtual image --
def test_huge_virtual_image(scenes, torch):
    sc = scenes["quadric"]
    fw, fh = 33554433, 33554431
    w, h, dx, dy, count = 33, 17, 5, -2, 3
    g, pts = rc.SAMPLE_SEQS["hier8"]
    col, row = find_edge(sc, g * fw, g * fh)
    new = (fw, fh, min(max(col // g - w // 2, 0), fw - w), min(max(row // g - h // 2, 0), fh - h))
    old = (fw, fh, new[2] - dx, new[3] - dy)
    src = State(torch, w, h).built(sc, old, "hier8", count)
    src_acc, src_out = src.read()
    dst = src.scrolled(sc, new, "hier8", count, dx, dy)
    got_acc, got_out = dst.read()
    # kept: rows [2, 17) and columns [0, 28) of the destination, from the source
    np.testing.assert_array_equal(got_acc[-dy:, :w - dx], src_acc[:h + dy, dx:])
    np.testing.assert_array_equal(got_out[-dy:, :w - dx], src_out[:h + dy, dx:])
    # exposed: the three samples of each pixel from rco_pixels, at the subsample image's scale
    mask = np.ones((h, w), bool)
    mask[-dy:, :w - dx] = False
    ys, xs = np.nonzero(mask)
    sums = np.zeros((len(ys), 3), np.uint32)
    for px, py in pts[:count]:
        sx = g * (new[2] + xs.astype(np.int64)) + px
        sy = g * (new[3] + ys.astype(np.int64)) + py
        rgb, _ = oracle_pixels(sc, g * fw, g * fh, sy * (g * fw) + sx)
        sums += rgb
    want = np.concatenate([sums, np.full((len(ys), 1), count, np.uint32)], axis=1).astype(np.uint16)
    np.testing.assert_array_equal(got_acc[mask], want)
    np.testing.assert_array_equal(got_out[mask], rc.accum_resolve(want[None])[0])
    assert rc.accum_stats() == stats_of(int(mask.sum()), count)
    # a condition on the input, not a tolerance: the window looks at an edge
    assert len(np.unique(got_out.reshape(-1, 3), axis=0)) >= 2, new
    check(src, src_acc, src_out, "the source")


# ------------------------------------------------------------------- 6. zero_normalize --
def test_zero_normalize_counts_the_exposed_rays(tmp_path, torch):
    """test_gpu_window.py's 5 x 3 plane-and-light scene with the light moved.  A lattice of 2, 4
    or 8 has no point at the pixel centre, and with the light on the centre ray's hit point the
    oracle counts no event for any subsample of the 10 x 6, 20 x 12 or 40 x 24 image.  At
    (1.25, 1.25, -5) the light lies exactly where the ray of subsample (5, 2) of the 10 x 6 image
    ends: point (1, 0) of pixel (2, 1) on the lattice of 2.  A pan that exposes that pixel counts
    its event, the pan that exposes its neighbour counts none; the kept pixel's rays are not shot
    and not counted in either."""
    path = tmp_path / "z.scene"
    path.write_text("camera, width: 5.0, height: 3.0\n"
                    "plane, normal: [0, 0, 1], diffuse_color: [0.3, 0.5, 0.7], "
                    "specular_color: [1, 1, 1], position: [0, 0, -5], reflectivity: 0.5\n"
                    "light, color: [4, 4, 4], radial-a2: 0.01, radial-a1: 0.0125, "
                    "radial-a0: 0.0125, position: [1.25, 1.25, -5]\n")
    sc = rc.Scene.from_file(str(path))
    seq = (2, [(1, 0), (0, 1)])
    new = (5, 3, 1, 1)               # virtual pixels (1, 1) and (2, 1)
    counts = []
    for dx, exposed_x in ((1, 1), (-1, 0)):
        src = State(torch, 2, 1).built(sc, (5, 3, 1 - dx, 1), seq, 2)
        src_acc, src_out = src.read()
        events = 0
        for px, py in seq[1]:
            _, z = oracle_pixels(sc, 10, 6, [(2 * 1 + py) * 10 + 2 * (1 + exposed_x) + px])
            events += int(z.sum())
        tim = {}
        dst = src.scrolled(sc, new, seq, 2, dx, 0, timing=tim)
        assert tim["zero_normalize"] == events, (dx, tim, events)
        assert tim["kernel_ms"] > 0.0
        got_acc, got_out = dst.read()
        np.testing.assert_array_equal(got_acc[0, 1 - exposed_x], src_acc[0, exposed_x])
        np.testing.assert_array_equal(got_out[0, 1 - exposed_x], src_out[0, exposed_x])
        np.testing.assert_array_equal(got_acc, State(torch, 2, 1).built(sc, new, seq, 2).read()[0])
        counts.append(events)
    assert counts[0] > 0 and counts[1] == 0


# --------------------------------------------------------------------- 7. stream order --
def test_stream_order(scenes, torch):
    """Pass, scroll and pass on a non-default stream with no synchronisation in between."""
    sc = scenes["quadric"]
    w, h, dx, dy = 40, 24, 12, 6
    old, new = (*FULL, 5, 3), (*FULL, 17, 9)
    g, pts = rc.SAMPLE_SEQS["hier4"]
    stream = torch.cuda.Stream()
    src, dst = State(torch, w, h), State(torch, w, h)
    src.run(sc, old, "hier4", 0, 5, reset=True, stream=stream)
    rc.accum_scroll_device(sc, new, w, h, "hier4", 5, dx, dy, src.d_acc.data_ptr(),
                           src.d_out.data_ptr(), dst.d_acc.data_ptr(), dst.d_out.data_ptr(),
                           stream_ptr=stream.cuda_stream, depth=DEPTH)
    dst.run(sc, new, "hier4", 5, 2, stream=stream)
    stream.synchronize()
    acc, out = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8)
    acc, out, _, _ = rc.accum_step(acc, out, window_big(scenes, "quadric", g, old, w, h, "fast"), g,
                                   pts[:5], 0, reset=True)
    big = window_big(scenes, "quadric", g, new, w, h, "fast")
    acc, out, _ = rc.accum_scroll(acc, out, big, g, pts[:5], dx, dy)
    acc, out, _, _ = rc.accum_step(acc, out, big, g, pts[5:7], 0)
    check(dst, acc, out, "pass, scroll, pass")
    assert (acc[:, :, 3] == 7).all()


# ---------------------------------------------------- 8. state of the other families --
def test_other_families_keep_their_state(scenes, torch):
    sc = scenes["simple"]
    w, h = 64, 48
    d_out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc.render_pattern_device(sc, w, h, "rgss4", d_out.data_ptr(), threshold=16, depth=DEPTH,
                             mode="fast")
    pattern = rc.pattern_stats()
    assert 0 < pattern["refined_pixels"] < w * h
    rc.pattern_phase_ms()
    src = State(torch, w, h).built(sc, (97, 61, 5, 3), "hier4", 3)
    src.scrolled(sc, (97, 61, 8, 5), "hier4", 3, 3, 2)
    assert rc.accum_stats() == stats_of(exposed_count(w, h, 3, 2), 3)
    ms = rc.accum_phase_ms()
    assert ms["mark"] >= 0.0 and ms["shoot"] >= 0.0
    with pytest.raises(RuntimeError):
        rc.pattern_phase_ms()
    assert rc.pattern_stats() == pattern
    # a scroll that exposes nothing: a copy, no pass, four zeros, and its spans are there
    src.scrolled(sc, (97, 61, 5, 3), "hier4", 3, 0, 0)
    assert rc.accum_stats() == stats_of(0, 3)
    ms = rc.accum_phase_ms()
    assert ms["mark"] >= 0.0 and ms["shoot"] >= 0.0
    assert rc.pattern_stats() == pattern
