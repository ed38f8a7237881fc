"""Separable reconstruction filters (rc_filter): the contract in numpy against a plain triple
loop, the tap rules in Python and in the library, and the refusals, all without a GPU."""
import ctypes

import numpy as np
import pytest

from helpers import rc, scene_path

# the signed vectors of tests/test_gpu_filter.py: halo h = s, sum 256
SIGNED = {2: [-4, 24, 108, 108, 24, -4],
          4: [-1, -2, 5, 22, 44, 60, 60, 44, 22, 5, -2, -1],
          8: [0, -1, -1, -1, 1, 4, 8, 14, 19, 25, 29, 31, 31, 29, 25, 19, 14, 8, 4, 1, -1, -1, -1,
              0]}


def loop_filter(img, s, taps):
    """include/raycast_hip.h's filter contract, one output sample at a time."""
    sh, sw, ch = img.shape
    oh, ow = sh // s, sw // s
    n = len(taps)
    h = (n - s) // 2
    total = sum(taps)
    s2 = total * total
    out = np.zeros((oh, ow, ch), dtype=np.uint8)
    for y in range(oh):
        for x in range(ow):
            for c in range(ch):
                acc = 0
                for j in range(n):
                    yy = min(max(s * y - h + j, 0), sh - 1)
                    for i in range(n):
                        xx = min(max(s * x - h + i, 0), sw - 1)
                        acc += taps[j] * taps[i] * int(img[yy, xx, c])
                out[y, x, c] = min(max((acc + s2 // 2) // s2, 0), 255)
    return out


@pytest.mark.parametrize("s", [2, 4, 8])
def test_numpy_contract_equals_the_loop(s):
    rng = np.random.default_rng(40 + s)
    img = rng.integers(0, 256, size=(3 * s, 5 * s, 3), dtype=np.uint8)
    for taps in (rc.filter_tent(s), SIGNED[s]):
        np.testing.assert_array_equal(rc.filter_downsample(img, s, taps),
                                      loop_filter(img, s, taps))


@pytest.mark.parametrize("s", [2, 4, 8])
def test_box_taps_are_the_box_filter(s):
    rng = np.random.default_rng(50 + s)
    img = rng.integers(0, 256, size=(3 * s, 5 * s, 3), dtype=np.uint8)
    np.testing.assert_array_equal(rc.filter_downsample(img, s, [1] * s),
                                  rc.box_downsample(img, s))
    assert rc.filter_box(s) == [1] * s


@pytest.mark.parametrize("s", [2, 4, 8])
def test_constant_image_maps_to_itself(s):
    vectors = [rc.filter_box(s), rc.filter_tent(s), SIGNED[s], [1024] * 2 + [0] * (s - 2),
               [-3] + [7] * s + [-3], [50, -43] * (3 * s // 2)]
    for v in (0, 1, 127, 254, 255):
        img = np.full((2 * s, 3 * s, 3), v, dtype=np.uint8)
        for taps in vectors:
            rc.filter_check(taps, s)
            out = rc.filter_downsample(img, s, taps)
            assert out.shape == (2, 3, 3)
            assert (out == v).all(), (s, v, taps)


def test_tent_vectors():
    assert rc.filter_tent(2) == [1, 3, 3, 1]
    assert rc.filter_tent(4) == [1, 3, 5, 7, 7, 5, 3, 1]
    assert rc.filter_tent(8) == [1, 3, 5, 7, 9, 11, 13, 15, 15, 13, 11, 9, 7, 5, 3, 1]
    for s in (2, 4, 8):
        assert sum(rc.filter_tent(s)) == 2 * s * s
        assert rc.filter_check(rc.filter_tent(s), s) == s // 2
    for bad in (0, 1, 3, 16, -2):
        with pytest.raises(ValueError):
            rc.filter_tent(bad)
        with pytest.raises(ValueError):
            rc.filter_box(bad)


def test_library_vectors_agree():
    lib = rc.hip_lib()
    for s in (2, 4, 8):
        for fn, want in ((lib.rc_filter_box, rc.filter_box(s)),
                         (lib.rc_filter_tent, rc.filter_tent(s))):
            f = rc.RcFilter()
            assert fn(s, ctypes.byref(f)) == 0
            assert [f.taps[i] for i in range(f.ntaps)] == want
            assert lib.rc_filter_check(ctypes.byref(f), s) == 0
    f = rc.RcFilter()
    for bad in (0, 1, 3, 16, -2):
        assert lib.rc_filter_box(bad, ctypes.byref(f)) == -1
        assert lib.rc_filter_tent(bad, ctypes.byref(f)) == -1
    assert lib.rc_filter_box(2, None) == -1 and lib.rc_filter_tent(2, None) == -1


def lib_check(taps, s):
    f = rc.RcFilter()
    f.ntaps = len(taps)
    for i, k in enumerate(taps[:rc.FILTER_MAX_TAPS]):
        f.taps[i] = k
    return rc.hip_lib().rc_filter_check(ctypes.byref(f), s)


BAD = {"L - s odd": ([1, 2, 1], 2),
       "L below s": ([1, 1], 4),
       "h > s": ([1] * 8, 2),
       "L > 24": ([1] * 26, 8),
       "S = 0": ([1, -1, -1, 1], 2),
       "S < 0": ([1, -3, -3, 1], 2),
       "sum |k| = 2049": ([1024, 1025], 2),
       "sum |k| = 2049, signed": ([-1, 1024, 1024, 0], 2)}


@pytest.mark.parametrize("rule", sorted(BAD))
def test_check_refuses(rule, capfd):
    taps, s = BAD[rule]
    with pytest.raises(ValueError):
        rc.filter_check(taps, s)
    assert lib_check(taps, s) == -1
    assert "rc_filter_check" in capfd.readouterr().err   # a message names the rule


def test_check_accepts():
    for taps, s in (([1024, 1024], 2), ([-512, 1536], 2), ([1] * 24, 8), ([1] * 6, 2),
                    (SIGNED[2], 2), (SIGNED[4], 4), (SIGNED[8], 8)):
        rc.filter_check(taps, s)
        assert lib_check(taps, s) == 0, taps
    assert sum(abs(k) for k in [-512, 1536]) == 2048
    for s in (0, 1, 3, 16):
        with pytest.raises(ValueError):
            rc.filter_check([1] * max(s, 1), s)
        assert lib_check([1] * max(s, 1), s) == -1
    assert rc.hip_lib().rc_filter_check(None, 2) == -1


def test_downsample_refuses_bad_images():
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    with pytest.raises(ValueError):
        rc.filter_downsample(img.astype(np.int32), 2, [1, 3, 3, 1])
    with pytest.raises(ValueError):
        rc.filter_downsample(img[:7], 2, [1, 3, 3, 1])
    with pytest.raises(ValueError):
        rc.filter_downsample(img[:, :7], 2, [1, 3, 3, 1])
    with pytest.raises(ValueError):
        rc.filter_downsample(img[0], 2, [1, 3, 3, 1])
    with pytest.raises(ValueError):
        rc.filter_downsample(img, 2, [1, 3, 1])
    with pytest.raises(ValueError):
        rc.filter_downsample(img, 3, [1, 1, 1])


def test_layout_and_exports():
    assert ctypes.sizeof(rc.RcFilter) == 52
    lib = rc.hip_lib()
    for name in ("rc_filter_box", "rc_filter_tent", "rc_filter_check", "rc_filter_env",
                 "rc_render_filtered", "rc_render_filtered_device", "rc_filter_image_device",
                 "rc_filter_phase_ms"):
        assert name in rc.HIP_EXPORTS, name
        assert hasattr(lib, name), name
    # the pinned layouts are untouched
    assert rc.version().startswith("raycast-mi355x 0.3")
    assert rc.TUNING_FIELDS[-1] == "adaptive_blocks"
    assert ctypes.sizeof(rc.RcOptions) == 20
    assert set(rc.FILTER_TILES) == {2, 4, 8}


def test_refusals_come_before_any_device_work():
    """Everything the filtered entry points refuse is refused from the arguments alone, before
    the first HIP call: the refusals hold on a machine without a GPU, and the pixmap is
    untouched."""
    sc = rc.Scene.from_file(scene_path("simple"))
    lib = rc.hip_lib()
    fake = 4096   # a non-null "device pointer" that a refused call never follows
    tent = rc.filter_tent(2)
    base = np.random.default_rng(3).integers(0, 256, size=(8, 8, 3), dtype=np.uint8)
    out = base.copy()

    def both(opt, f, w=8, h=8):
        pf = ctypes.byref(f) if f is not None else None
        assert lib.rc_render_filtered(sc.packed(), w, h, ctypes.byref(opt), pf,
                                      out.ctypes.data_as(ctypes.c_void_p), None) == -1
        assert lib.rc_render_filtered_device(sc.packed(), w, h, ctypes.byref(opt), pf, fake,
                                             None, None) == -1

    good = rc.RcFilter()
    assert lib.rc_filter_tent(2, ctypes.byref(good)) == 0
    # the factor: off, not a factor, with a threshold; more than one GPU
    for bad in (dict(ssaa=0), dict(ssaa=1), dict(ssaa=3), dict(ssaa=16), dict(ssaa=-1),
                dict(ssaa=2, adaptive=16), dict(ssaa=1, adaptive=16), dict(ssaa=2, gpus=2)):
        for mode in ("fast", "parity", "cuda"):
            both(rc.options(6, mode, **bad), good)
    # a filter that fails the check (here: for this factor), a null filter
    for taps, s in BAD.values():
        f = rc.RcFilter()
        f.ntaps = len(taps)
        for i, k in enumerate(taps[:rc.FILTER_MAX_TAPS]):
            f.taps[i] = k
        both(rc.options(6, "fast", ssaa=s), f)
        assert lib.rc_filter_image_device(fake, 8, 8, s, ctypes.byref(f), 2 * fake, None) == -1
    both(rc.options(6, "fast", ssaa=2), None)
    # the size limits: W, H <= 2^28 / s; nothing below 1
    for w, h in (((1 << 27) + 1, 1), (1, (1 << 27) + 1), (0, 8), (8, 0), (-1, 8)):
        both(rc.options(6, "fast", ssaa=2), good, w, h)
        assert lib.rc_filter_image_device(fake, w, h, 2, ctypes.byref(good), 1 << 40, None) == -1
    # null pointers, the scene included
    opt = rc.options(6, "fast", ssaa=2)
    assert lib.rc_render_filtered(None, 8, 8, ctypes.byref(opt), ctypes.byref(good),
                                  out.ctypes.data_as(ctypes.c_void_p), None) == -1
    assert lib.rc_render_filtered(sc.packed(), 8, 8, ctypes.byref(opt), ctypes.byref(good), None,
                                  None) == -1
    assert lib.rc_render_filtered(sc.packed(), 8, 8, None, ctypes.byref(good),
                                  out.ctypes.data_as(ctypes.c_void_p), None) == -1
    assert lib.rc_render_filtered_device(sc.packed(), 8, 8, ctypes.byref(opt), ctypes.byref(good),
                                         None, None, None) == -1
    # the filter pass alone: null pointers, source == destination and overlaps, bad factors
    g = ctypes.byref(good)
    assert lib.rc_filter_image_device(None, 8, 8, 2, g, fake, None) == -1
    assert lib.rc_filter_image_device(fake, 8, 8, 2, g, None, None) == -1
    assert lib.rc_filter_image_device(fake, 8, 8, 2, None, 1 << 20, None) == -1
    assert lib.rc_filter_image_device(fake, 8, 8, 2, g, fake, None) == -1
    assert lib.rc_filter_image_device(fake, 8, 8, 2, g, fake + 8 * 8 * 3 * 4 - 1, None) == -1
    assert lib.rc_filter_image_device(fake, 8, 8, 2, g, fake - 8 * 8 * 3 + 1, None) == -1
    for s in (0, 1, 3, 16):
        assert lib.rc_filter_image_device(fake, 8, 8, s, g, 1 << 20, None) == -1
    # the Python wrappers raise
    with pytest.raises(RuntimeError):
        rc.filter_image_device(fake, 8, 8, 2, tent, fake)
    with pytest.raises(RuntimeError):
        rc.render_filtered_device(sc, 1 << 28, 8, tent, 2, fake, mode="fast")
    with pytest.raises(ValueError):
        rc.render_filtered(sc, 8, 8, [1, 2, 1], 2, mode="fast", out=out)
    with pytest.raises(ValueError):
        rc.render_filtered_device(sc, 8, 8, tent, 3, fake, mode="fast")
    np.testing.assert_array_equal(out, base)


def test_env_decision(monkeypatch, capfd):
    """RAYCAST_FILTER as raycast() reads it (rc_filter_env): the tent goes through the filtered
    path only with a plain factor of 2, 4 or 8; everything else warns and keeps today's path."""
    monkeypatch.delenv("RAYCAST_FILTER", raising=False)
    for s in (1, 2, 4, 8):
        assert rc.filter_from_env(s) is None
    assert capfd.readouterr().err == ""          # unset: silent, today's behaviour
    monkeypatch.setenv("RAYCAST_FILTER", "tent")
    for s in (2, 4, 8):
        assert rc.filter_from_env(s) == rc.filter_tent(s)
    assert capfd.readouterr().err == ""
    for kw in (dict(ssaa=1), dict(ssaa=0)):
        assert rc.filter_from_env(**kw) is None
        err = capfd.readouterr().err
        assert err.startswith("Warning: RAYCAST_FILTER") and "RAYCAST_SSAA" in err
    assert rc.filter_from_env(4, adaptive=32) is None
    err = capfd.readouterr().err
    assert err.startswith("Warning: RAYCAST_FILTER") and "RAYCAST_SSAA_ADAPTIVE" in err
    monkeypatch.setenv("RAYCAST_FILTER", "box")
    assert rc.filter_from_env(2) is None
    assert capfd.readouterr().err == ""
    assert rc.filter_from_env(1) is None
    assert capfd.readouterr().err.startswith("Warning: RAYCAST_FILTER")
    for other in ("gauss", "", "TENT", "tent "):
        monkeypatch.setenv("RAYCAST_FILTER", other)
        assert rc.filter_from_env(2) is None
        err = capfd.readouterr().err
        assert err.startswith("Warning: RAYCAST_FILTER") and "using box" in err
