"""The list machinery of the sampling family, plane by plane ("Plane-by-plane tests of
the lists"): k_aa_mark (rc_lists.hpp) and the binning block of k_rates_render (rc_rates_bin.inc),
run by tests/tools/list_check.hip (make listcheck) with the launchers' own grid and block shapes
on the designed planes of tests/list_cases.py, against the sequential definitions there; and the
stride loops of the list consumers through the shipped entries on designed lists.  Everything is
exact and no case is left out: whole buffers come back, so every slot nobody should have written
must still hold the harness's sentinel.  The order inside a list is not asserted (it follows the
atomics' arrival): a list is compared sorted, which also finds an entry listed twice.
Teeth: eight wrong builds of the harness, each caught by the family built for it and unseen by
the families that cannot see it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import list_cases as lc
from helpers import ROOT, rc, scene_path
from test_gpu_prims import _ok, _p

pytestmark = pytest.mark.gpu

U8, U32, I32, I64 = np.uint8, np.uint32, np.int32, np.int64


class ListHarness:
    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        V, I = ctypes.c_void_p, ctypes.c_int
        lib.lv_mark.argtypes = [V, I, I, I, V, I, V, V]
        lib.lv_bin.argtypes = [V, I, I, I, V, V, V]
        self.wrong = int(lib.lv_wrong())
        self.fill32 = int(np.array([int(lib.lv_fill())] * 4, U8).view(U32)[0])
        assert (int(lib.lv_mark_block()), int(lib.lv_mark_rows())) == (lc.MARK_BLOCK, lc.MARK_ROWS)
        assert int(lib.lv_rate_chunk()) == lc.RATE_CHUNK
        assert int(lib.lv_tile_w()) == int(lib.lv_tile_h()) == lc.TILE

    def mark(self, imgs, ts, odd):
        """count [B] and the whole list buffers [B, P] of images [B, H, W, 3] at thresholds ts."""
        imgs = np.ascontiguousarray(imgs, U8)
        B, H, W, _ = imgs.shape
        ts = np.ascontiguousarray(np.broadcast_to(np.asarray(ts, I32), (B,)))
        count, lst = np.zeros(B, U32), np.zeros((B, H * W), U32)
        _ok(self.lib.lv_mark(_p(imgs), B, W, H, _p(ts), int(odd), _p(count), _p(lst)),
            f"lv_mark({B} x {W}x{H}, odd {odd})")
        return count, lst

    def bin(self, maps):
        """cnt [B, 5], list4 [B, P] and list28 [B, P] of maps [B, H, W]."""
        maps = np.ascontiguousarray(maps, U8)
        B, H, W = maps.shape
        cnt, l4, l28 = np.zeros((B, 5), U32), np.zeros((B, H * W), U32), np.zeros((B, H * W), U32)
        _ok(self.lib.lv_bin(_p(maps), B, W, H, _p(cnt), _p(l4), _p(l28)), f"lv_bin({B} x {W}x{H})")
        return cnt, l4, l28


def _lib(name):
    return os.path.join(ROOT, "tests", "build", name)


@pytest.fixture(scope="module")
def built():
    """The harness libraries; built here (no build, no pass)."""
    subprocess.run(["make", "-s", "-j6", "listcheck"], cwd=ROOT, check=True, capture_output=True)
    rc.hip_lib()   # first: it settles which HIP runtime the process has (torch's, where torch is)


@pytest.fixture(scope="module")
def hw(built):
    h = ListHarness(_lib("liblistcheck.so"))
    assert h.wrong == 0
    return h


def _wrong(k):
    h = ListHarness(_lib(f"liblistcheck_w{k}.so"))
    assert h.wrong == k
    return h


# ---------------------------------------------------------------------------- checking --
def _listed(got, member, where, sent):
    """[B] bool: the slots `where` [B, P] of the buffers `got` hold exactly the indices that
    `member` [B, P] marks, each once, in any order (both sides sorted, the other slots taken as the
    sentinel).  That the other slots do hold the sentinel is the caller's second check."""
    P = got.shape[1]
    idx = np.arange(P, dtype=U32)[None, :]
    have = np.sort(np.where(where, got, U32(sent)), axis=1)
    want = np.sort(np.where(member, idx, U32(sent)), axis=1)
    return (have == want).all(axis=1)


def mark_bad(h, imgs, ts):
    """[2, B] bool: the images whose count, list (as a set, without duplicates) or untouched slots
    differ from mark_ref's, at the aligned and at the odd address.  The harness itself compares the
    guards and the image (_ok)."""
    imgs = np.asarray(imgs)
    B, H, W, _ = imgs.shape
    mask = lc.mark_ref(imgs, np.broadcast_to(np.asarray(ts), (B,))).reshape(B, H * W)
    n = mask.sum(axis=1)
    slot = np.arange(H * W)[None, :] < n[:, None]
    out = []
    for odd in (0, 1):
        count, lst = h.mark(imgs, ts, odd)
        good = (count == n) & _listed(lst, mask, slot, h.fill32) & ((lst != h.fill32) == slot).all(axis=1)
        out.append(~good)
    return np.array(out)


def bin_bad(h, maps):
    """[B] bool: the maps whose five counters, three lists or untouched slots differ from the
    definition's (lc.bin_masks, the batched form of bin_ref)."""
    maps = np.asarray(maps)
    B, H, W = maps.shape
    P = H * W
    m2, m4, m8, want = lc.bin_masks(maps)
    cnt, l4, l28 = h.bin(maps)
    at = np.arange(P)[None, :]
    up, down, s4 = at < want[:, 0:1], at >= P - want[:, 2:3], at < want[:, 1:2]
    good = (cnt == want).all(axis=1)
    good &= _listed(l4, m4, s4, h.fill32) & ((l4 != h.fill32) == s4).all(axis=1)
    good &= _listed(l28, m2, up, h.fill32) & _listed(l28, m8, down, h.fill32)
    good &= ((l28 != h.fill32) == (up | down)).all(axis=1)
    return ~good


# a family is a generator of (tag, images, thresholds) or (tag, maps) batches
def small_batches(shapes=None, ts=lc.THRESHOLDS):
    for k, (w, h) in enumerate(shapes or lc.shapes_upto(8)):
        for t in ts:
            yield f"small {w}x{h} t{t}", lc.mark_small(t, w, h, k), t


def spike_batches(ws=lc.SPIKE_W, hs=lc.SPIKE_H, ts=lc.THRESHOLDS):
    for w in ws:
        for h in hs:
            imgs = [lc.spike_lattice(t, w, h)[0] for t in ts]
            yield f"spikes {w}x{h}", np.concatenate(imgs), np.repeat(np.array(ts), 16)


def split_batches(ts=lc.THRESHOLDS):
    for t in ts:
        yield f"split t{t}", np.stack([lc.split_contrast(t, f)[0] for f in (0, 1)]), t


def noise_batches(ts=lc.THRESHOLDS, shapes=lc.NOISE_SHAPES):
    for k, (w, h) in enumerate(shapes):
        for t in ts:
            yield f"noise {w}x{h} t{t}", lc.near_threshold_noise(t, w, h, k)[None], t


def strip_batches():
    for k, (w, h) in enumerate(lc.STRIPS):
        t = (16, 2)[k]
        yield f"strip noise {w}x{h}", lc.near_threshold_noise(t, w, h, len(lc.NOISE_SHAPES) + k)[None], t
        imgs, _ = lc.spike_lattice(t, w, h, phases=(5 * k + 3,))
        yield f"strip spikes {w}x{h}", imgs, t


def run_mark(h, batches):
    """(image runs, image runs that differ, the first differing tag)."""
    ran = bad = 0
    first = None
    for tag, imgs, ts in batches:
        b = mark_bad(h, imgs, ts)
        ran += b.size
        bad += int(b.sum())
        if b.any() and first is None:
            o, i = np.argwhere(b)[0]
            first = f"{tag} image {i} {'odd' if o else 'aligned'}"
    return ran, bad, first


def bin_random_batches(shapes=None):
    for w, h in shapes or lc.bin_shapes():
        yield f"maps {w}x{h}", np.stack([lc.random_map(w, h, s) for s in (0, 1)])


def bin_small_batches():
    for w, h in lc.shapes_upto(6):
        yield f"small maps {w}x{h}", lc.bin_small(w, h)


def bin_extreme_batches():
    for w, h in lc.BIN_EXTREME_SHAPES:
        ex = lc.bin_extremes(w, h)
        yield f"extremes {w}x{h} {' '.join(ex)}", np.stack(list(ex.values()))


def run_bin(h, batches):
    ran = bad = 0
    first = None
    for tag, maps in batches:
        b = bin_bad(h, maps)
        ran += b.size
        bad += int(b.sum())
        if b.any() and first is None:
            first = f"{tag} map {int(np.flatnonzero(b)[0])}"
    return ran, bad, first


def _clean(name, res):
    ran, bad, first = res
    print(f"[gpu_lists] {name}: {ran} runs, {bad} differ")
    assert bad == 0, f"{name}: {bad} of {ran} differ, first {first}"
    return ran


# -------------------------------------------------------------------------------- mark --
@pytest.mark.parametrize("t", lc.THRESHOLDS)
def test_mark_small(hw, t):
    """Every image of <= 8 pixels over {base, base + t - 1, base + t}, one batch a shape."""
    ran = _clean(f"mark small t{t}", run_mark(hw, small_batches(ts=(t,))))
    assert ran >= 2 * 4 * (2 if t == 1 else 3) ** 8   # t = 1: base + t - 1 is base


@pytest.mark.parametrize("w", lc.SPIKE_W)
def test_mark_spike_lattice(hw, w):
    """Single-pixel spikes of height t and t - 1 at every phase of a 4 x 4 lattice: the flagged
    pixels beside a wave's, a workgroup's and a row block's edge are flagged for one neighbour."""
    assert _clean(f"mark spikes W{w}", run_mark(hw, spike_batches(ws=(w,)))) == 2 * 80 * len(lc.SPIKE_H)


def test_mark_split_noise_extremes_strips(hw):
    _clean("mark split contrast", run_mark(hw, split_batches()))
    _clean("mark near-threshold noise", run_mark(hw, noise_batches()))
    _clean("mark strips", run_mark(hw, strip_batches()))
    for w, h in lc.EXTREME_SHAPES:
        for t in lc.THRESHOLDS:
            for odd in (0, 1):
                count, lst = hw.mark(lc.flat_image(t, w, h)[None], t, odd)
                assert count[0] == 0 and (lst == hw.fill32).all(), (w, h, t)   # the list untouched
                count, lst = hw.mark(lc.checkerboard(w, h)[None], t, odd)
                assert count[0] == w * h and np.array_equal(np.sort(lst[0]), np.arange(w * h)), (w, h, t)
    _clean("mark extremes", run_mark(hw, ((f"extreme {w}x{h} t{t}", np.stack(
        [lc.flat_image(t, w, h), lc.checkerboard(w, h)]), t) for w, h in lc.EXTREME_SHAPES
        for t in lc.THRESHOLDS)))


# ----------------------------------------------------------------------------- binning --
def test_bin_small(hw):
    """Every map of <= 6 pixels over {0, 1, 2, 4, 8, 3}, one batch a shape."""
    assert _clean("bin small", run_bin(hw, bin_small_batches())) > 4 * 6 ** 6


def test_bin_random_and_extremes(hw):
    """Every workgroup count of the family wide and tall, the last partial chunks nobody's turn
    would bin, pixel counts around multiples of 2 048; one class filling the shared buffer."""
    _clean("bin random maps", run_bin(hw, bin_random_batches()))
    _clean("bin extremes", run_bin(hw, bin_extreme_batches()))
    for w, h in lc.BIN_EXTREME_SHAPES:   # the two lists of the shared buffer meet exactly
        cnt, l4, l28 = hw.bin(lc.bin_extremes(w, h)["half28"][None])
        n = w * h
        assert cnt[0].tolist() == [n // 2, 0, n - n // 2, 0, 0] and (l4 == hw.fill32).all()
        assert np.array_equal(np.sort(l28[0]), np.arange(n))


# ------------------------------------------------- designed lists through the entries --
@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def simple():
    return rc.Scene.from_file(scene_path("simple"))


def _masked_pass(torch, scene, form, img, t, rng):
    """One masked pass of one sample over the image `img` and a random valid state: n rises by
    exactly 1 on mark_ref's pixels, every other pixel keeps all 11 of its bytes, and the pass
    counts mark_ref's pixels."""
    from test_gpu_accum import State, random_state
    h, w = img.shape[:2]
    acc_in = random_state(rng, h, w, 200)
    st = State(torch, w, h, acc_in, img)
    a, o = st.d_acc.data_ptr(), st.d_out.data_ptr()
    if form == "plain":
        rc.accum_pass_device(scene, w, h, "queens8", 5, 1, a, o, threshold=t)
    elif form == "window":
        rc.accum_pass_window_device(scene, (2 * w, 2 * h + 3, 3, 2), w, h, "queens8", 5, 1, a, o, threshold=t)
    else:
        rc.accum_pass_camera_device(scene, rc.camera((0.25, -0.5, 0.0)), None, w, h, "queens8", 5, 1, a, o,
                                    threshold=t)
    got_acc, got_out = st.read()
    mask = lc.mark_ref(img, t)
    tag = f"{form} {w}x{h} t{t}"
    np.testing.assert_array_equal(got_acc[~mask], acc_in[~mask], err_msg=tag)
    np.testing.assert_array_equal(got_out[~mask], img[~mask], err_msg=tag)
    np.testing.assert_array_equal(got_acc[mask][:, 3], acc_in[mask][:, 3] + 1, err_msg=tag)
    assert rc.accum_stats()["active_pixels"] == int(mask.sum()), tag
    return int(mask.sum())


@pytest.mark.parametrize("form", ["plain", "window", "camera"])
def test_masked_passes_on_designed_images(form, torch, simple):
    """Spike and step images through the shipped k_aa_mark and accum_listed: a missed entry adds
    0 to n and an entry listed twice could add 2 (two lanes' unsynchronised updates of one record
    may also add 1: it is the harness's sorted lists that exclude a duplicate)."""
    rng = np.random.default_rng(77)
    imgs = [(lc.spike_lattice(16, 129, 17, phases=(0,))[0][0], 16), (lc.spike_lattice(2, 257, 9, phases=(7,))[0][0], 2),
            (lc.spike_lattice(255, 65, 16, phases=(3,))[0][0], 255), (lc.step_image(129, 17), 16),
            (lc.step_image(257, 9, 128), 128), (lc.split_contrast(16, 0)[0], 16)]
    for img, t in imgs:
        n = _masked_pass(torch, simple, form, img, t, rng)
        assert 0 < n < img.shape[0] * img.shape[1]


@pytest.mark.parametrize("form", ["plain", "window", "camera"])
def test_list_lengths_around_a_wave_and_the_grid_step(form, torch, simple):
    """H = 1 images with exactly n flagged pixels: a wave of accum_listed partly past the list's
    end (63, 64, 65, 255, 256, 257 entries), and lists one below, at and one above the step of a
    grid of one and of two workgroups (256 and 512 entries)."""
    rng = np.random.default_rng(78)
    for n in (63, 64, 65, 255, 256, 257):
        assert _masked_pass(torch, simple, form, lc.line_image(n), 16, rng) == n
    for blocks in (1, 2):
        with rc.tuned(adaptive_blocks=blocks):
            for n in (256 * blocks - 1, 256 * blocks, 256 * blocks + 1):
                assert _masked_pass(torch, simple, form, lc.line_image(n), 16, rng) == n


def test_rate_lists_around_a_wave_step_and_the_grid_step(torch, simple):
    """rc_render_rates_device on maps with exactly per - 1, per, per + 1 and step - 1, step, step
    + 1 pixels of rates 2, 4 and 8 (per = 16, 4, 1 listed pixels a wave step; step = 4 * blocks *
    per), over a random base, against the GPU's own ssaa = s images: a missed entry leaves the
    base's bytes."""
    w, h = 33, 17
    images = {s: rc.render(simple, w, h, depth=6, mode="fast", ssaa=s) for s in (1, 2, 4, 8)}
    rng = np.random.default_rng(79)
    base = rng.integers(0, 256, size=(h, w, 3), dtype=U8)
    per = {2: 16, 4: 4, 8: 1}
    seed = 0
    for blocks in (1, 2):
        with rc.tuned(adaptive_blocks=blocks):
            for around in ("per", "step"):
                for d in (-1, 0, 1):
                    counts = {s: (p if around == "per" else 4 * blocks * p) + d for s, p in per.items()}
                    rates = lc.counted_map(w, h, counts, seed)
                    seed += 1
                    want = rc.rates_compose(base, images, rates)
                    d_rates = torch.from_numpy(rates).cuda()
                    d_out = torch.from_numpy(base.copy()).cuda()
                    torch.cuda.synchronize()
                    rc.render_rates_device(simple, w, h, d_rates.data_ptr(), d_out.data_ptr())
                    torch.cuda.synchronize()
                    tag = f"blocks {blocks} {counts}"
                    np.testing.assert_array_equal(d_out.cpu().numpy(), want, err_msg=tag)
                    st = rc.rate_stats()
                    assert st["pixels"] == {1: 0, **counts} and st["invalid"] == 0, tag


# ------------------------------------------------------------------------------- teeth --
H1_SHAPES = [(w, 1) for w in range(1, 9)]
TALL_SHAPES = [(w, h) for w, h in lc.shapes_upto(8) if h >= 2]


def _teeth(name, k, caught, unseen=()):
    """Wrong build k: every `caught` family differs somewhere, no `unseen` family does."""
    h = _wrong(k)
    line = []
    for tag, run, batches in caught:
        ran, bad, _ = run(h, batches)
        assert bad > 0, f"teeth {k} ({name}): {tag} did not catch it"
        line.append(f"{tag} {bad} of {ran}")
    for tag, run, batches in unseen:
        ran, bad, first = run(h, batches)
        assert bad == 0, f"teeth {k} ({name}): {tag} cannot see it, and {bad} differ, first {first}"
        line.append(f"{tag} 0 of {ran} (cannot see it)")
    print(f"[gpu_lists] teeth {k} ({name}) caught: " + "; ".join(line))


def test_teeth_lane_63_and_lane_0(built):
    for k, name in ((1, "lane 63 keeps its own pixel"), (2, "lane 0 keeps its own pixel")):
        _teeth(name, k, [("spikes W 65", run_mark, spike_batches(ws=(65,))),
                         ("spikes W 257", run_mark, spike_batches(ws=(257,))),
                         ("split contrast", run_mark, split_batches())],
               [("small", run_mark, small_batches(ts=(16,))),
                ("spikes W 63", run_mark, spike_batches(ws=(63,)))])


def test_teeth_first_row(built):
    _teeth("the window starts at y0", 3, [("spikes H 9..17", run_mark, spike_batches(ws=(3, 65), hs=(9, 15, 16, 17))),
                                          ("split contrast", run_mark, split_batches())],
           [("small", run_mark, small_batches(ts=(2,))),
            ("spikes H <= 8", run_mark, spike_batches(ws=(3, 65), hs=(1, 2, 7, 8)))])


def test_teeth_threshold(built):
    flat_and_board = ((f"extreme t{t}", np.stack([lc.flat_image(t, 65, 9), lc.checkerboard(65, 9)]), t)
                      for t in lc.THRESHOLDS[:-1])
    _teeth("con > thr", 4, [("small", run_mark, small_batches(ts=(1, 255))),
                            ("spikes", run_mark, spike_batches(ws=(3,))),
                            ("split contrast", run_mark, split_batches())],
           [("flat and full-range images below 255", run_mark, flat_and_board)])


def test_teeth_row_base(built):
    _teeth("a row's base += popcount dropped", 5, [("small, H >= 2", run_mark, small_batches(TALL_SHAPES, (16,))),
                                                   ("noise", run_mark, noise_batches(ts=(16,)))],
           [("small, H = 1", run_mark, small_batches(H1_SHAPES, (16,)))])


def test_teeth_channel(built):
    red_green = [s for k, s in enumerate(lc.shapes_upto(8)) if k % 3 != 2]
    blue = [s for k, s in enumerate(lc.shapes_upto(8)) if k % 3 == 2]
    assert len(blue) == 6

    def only(shapes):
        return ((tag, imgs, t) for k, (w, h) in enumerate(lc.shapes_upto(8)) if (w, h) in shapes
                for tag, imgs, t in [(f"small {w}x{h}", lc.mark_small(16, w, h, k), 16)])
    _teeth("blue unpacked from red's bits", 8, [("small, blue", run_mark, only(blue)),
                                                ("spikes", run_mark, spike_batches(ws=(3, 65)))],
           [("small, red and green", run_mark, only(red_green))])


def test_teeth_binning(built):
    missing = [s for s in lc.bin_shapes() if lc.missing_duty(*s) and s[0] * s[1] > 2048]
    present = [s for s in lc.bin_shapes() if not lc.missing_duty(*s)]
    assert len(missing) >= 3
    _teeth("no duty = 0 fallback", 6, [("maps whose last chunk is nobody's turn", run_bin, bin_random_batches(missing))],
           [("small maps", run_bin, bin_small_batches()), ("the other maps", run_bin, bin_random_batches(present))])
    one_wave = [s for s in lc.bin_shapes() if s[0] * s[1] <= 64]
    assert len(one_wave) >= 10
    _teeth("a wave's base without the earlier waves", 7, [("maps", run_bin, bin_random_batches()),
                                                         ("extremes", run_bin, bin_extreme_batches())],
           [("small maps", run_bin, bin_small_batches()), ("maps of one wave", run_bin, bin_random_batches(one_wave))])
