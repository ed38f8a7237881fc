"""Variable-rate supersampling from a per-pixel rate map (rc_render_rates), the parts that need no
GPU: the numpy statement of the contract, the statistics record's layout, the exported names and
the layouts the feature must leave alone."""
import ctypes

import numpy as np
import pytest

from helpers import rc


def naive_compose(base, images, rates):
    """include/raycast_hip.h's rate-map contract, one pixel at a time."""
    out = base.copy()
    for y in range(base.shape[0]):
        for x in range(base.shape[1]):
            r = int(rates[y, x])
            if r:
                out[y, x] = images[r][y, x]
    return out


SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 3), (12, 10)]   # (W, H), test_adaptive.py's


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rates_compose_matches_definition(seed):
    rng = np.random.default_rng(2000 + seed)
    for w, h in SHAPES:
        base = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        images = {s: rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for s in (1, 2, 4, 8)}
        rates = rng.choice(np.array(rc.RATE_VALUES, dtype=np.uint8), size=(h, w))
        before = base.copy()
        got = rc.rates_compose(base, images, rates)
        assert got.dtype == np.uint8 and got.shape == (h, w, 3)
        np.testing.assert_array_equal(got, naive_compose(base, images, rates),
                                      err_msg=f"{w}x{h}")
        np.testing.assert_array_equal(base, before)   # the base is not written to


def test_rates_compose_uniform_maps():
    rng = np.random.default_rng(7)
    base = rng.integers(0, 256, size=(5, 6, 3), dtype=np.uint8)
    images = {s: np.full((5, 6, 3), s, dtype=np.uint8) for s in (1, 2, 4, 8)}
    np.testing.assert_array_equal(
        rc.rates_compose(base, {}, np.zeros((5, 6), dtype=np.uint8)), base)
    for s in (1, 2, 4, 8):
        # only the image of the rate that occurs is needed
        got = rc.rates_compose(base, {s: images[s]}, np.full((5, 6), s, dtype=np.uint8))
        np.testing.assert_array_equal(got, images[s])


def test_rates_compose_errors():
    base = np.zeros((4, 5, 3), dtype=np.uint8)
    images = {s: np.zeros((4, 5, 3), dtype=np.uint8) for s in (1, 2, 4, 8)}
    ok = np.ones((4, 5), dtype=np.uint8)
    rc.rates_compose(base, images, ok)
    for bad in (3, 5, 16, 255):
        r = ok.copy()
        r[2, 3] = bad
        with pytest.raises(ValueError):
            rc.rates_compose(base, images, r)
    with pytest.raises(ValueError):   # the map's shape
        rc.rates_compose(base, images, np.ones((5, 4), dtype=np.uint8))
    with pytest.raises(ValueError):   # the map's dtype
        rc.rates_compose(base, images, np.ones((4, 5), dtype=np.int32))
    with pytest.raises(ValueError):   # the base's dtype
        rc.rates_compose(base.astype(np.float32), images, ok)
    with pytest.raises(ValueError):   # an image's shape
        rc.rates_compose(base, {1: np.zeros((4, 6, 3), dtype=np.uint8)}, ok)
    with pytest.raises(ValueError):   # an image's dtype
        rc.rates_compose(base, {1: np.zeros((4, 5, 3), dtype=np.int16)}, ok)
    with pytest.raises(ValueError):   # a rate whose image is missing
        rc.rates_compose(base, {1: images[1]}, np.full((4, 5), 2, dtype=np.uint8))


def test_rate_stats_layout_and_names():
    assert ctypes.sizeof(rc.RcRateStats) == 48
    assert [n for n, _ in rc.RcRateStats._fields_] == ["pixels", "invalid", "rays"]
    assert rc.RcRateStats.invalid.offset == 32 and rc.RcRateStats.rays.offset == 40
    assert rc.RATE_VALUES == (0, 1, 2, 4, 8)
    for name in ("rc_render_rates", "rc_render_rates_device", "rc_rate_stats_get",
                 "rc_rate_phase_ms"):
        assert name in rc.HIP_EXPORTS, name
        assert hasattr(rc.hip_lib(), name), name
    for name in ("rates_compose", "render_rates", "render_rates_device", "rate_stats",
                 "rate_phase_ms"):
        assert callable(getattr(rc, name)), name


def test_render_rates_checks_the_map_before_the_library():
    class NoScene:
        def packed(self):
            raise AssertionError("the map is checked first")
    with pytest.raises(ValueError):
        rc.render_rates(NoScene(), 4, 3, np.ones((4, 3), dtype=np.uint8))   # (W, H) swapped
    with pytest.raises(ValueError):
        rc.render_rates(NoScene(), 4, 3, np.ones((3, 4), dtype=np.int64))


def test_refusals_come_before_any_device_work():
    """Everything rc_render_rates* refuses is refused from the arguments alone, before the
    first HIP call: the refusals hold on a machine without a GPU, and the pixmap is untouched."""
    from helpers import scene_path
    sc = rc.Scene.from_file(scene_path("simple"))
    lib = rc.hip_lib()
    fake = 4096   # a non-null "device pointer" that a refused call never follows
    # sizes: W*H = 2^32, 8*W or 8*H past INT_MAX, more than 65535 rows of tiles
    for w, h in ((1 << 16, 1 << 16), (1 << 28, 1), (1, 1 << 28), (1, 16 * 65535 + 1)):
        with pytest.raises(RuntimeError):
            rc.render_rates_device(sc, w, h, fake, fake)
    with pytest.raises(RuntimeError):   # parity mode
        rc.render_rates_device(sc, 8, 8, fake, fake, mode="parity")
    for ptrs in ((0, fake), (fake, 0)):   # null pointers
        with pytest.raises(RuntimeError):
            rc.render_rates_device(sc, 8, 8, *ptrs)
    rates = np.ones((8, 8), dtype=np.uint8)
    base = np.random.default_rng(3).integers(0, 256, size=(8, 8, 3), dtype=np.uint8)
    out = base.copy()
    with pytest.raises(RuntimeError):
        rc.render_rates(sc, 8, 8, rates, mode="parity", out=out)
    # the options: a factor or a threshold (the map carries the factor), more than one GPU
    for bad in (dict(ssaa=2), dict(ssaa=8), dict(ssaa=4, adaptive=16), dict(ssaa=1, adaptive=16),
                dict(ssaa=3), dict(ssaa=-1), dict(gpus=2)):
        opt = rc.options(6, "fast", **bad)
        assert lib.rc_render_rates(sc.packed(), 8, 8, ctypes.byref(opt),
                                   rates.ctypes.data_as(ctypes.c_void_p),
                                   out.ctypes.data_as(ctypes.c_void_p), None) == -1, bad
        assert lib.rc_render_rates_device(sc.packed(), 8, 8, ctypes.byref(opt), fake, fake,
                                          None, None) == -1, bad
    # the host-map call checks the map before it enqueues anything
    for v in (3, 5, 16, 255):
        bad_map = rates.copy()
        bad_map[7, 7] = v
        with pytest.raises(RuntimeError):
            rc.render_rates(sc, 8, 8, bad_map, out=out)
    np.testing.assert_array_equal(out, base)


def test_pinned_layouts_are_untouched():
    assert rc.version().startswith("raycast-mi355x 0.3")
    assert rc.TUNING_FIELDS[-1] == "adaptive_blocks"
    assert ctypes.sizeof(rc.RcOptions) == 20
    assert rc.RcOptions._fields_[-1][0] == "ssaa"
