"""Adaptive supersampling (rc_options.ssaa = RC_SSAA_ADAPTIVE(s, t)), the parts that need no GPU:
the numpy statement of the contract, the option's encoding, default and environment, and the
refinement kernel's lane map."""
import ctypes

import numpy as np
import pytest

from helpers import rc


def naive_mask(a, t):
    """include/raycast_hip.h's contrast, one pixel at a time."""
    h, w, _ = a.shape
    out = np.zeros((h, w), dtype=bool)
    for y in range(h):
        for x in range(w):
            con = 0
            for c in range(3):
                vals = [int(a[yy, xx, c])
                        for yy in range(max(y - 1, 0), min(y + 1, h - 1) + 1)
                        for xx in range(max(x - 1, 0), min(x + 1, w - 1) + 1)]
                con = max(con, max(vals) - min(vals))
            out[y, x] = con >= t
    return out


def naive_compose(a, f, t):
    m = naive_mask(a, t)
    out = a.copy()
    for y in range(a.shape[0]):
        for x in range(a.shape[1]):
            if m[y, x]:
                out[y, x] = f[y, x]
    return out


SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 3), (12, 10)]   # (W, H)


@pytest.mark.parametrize("t", [1, 16, 64, 255])
def test_edge_mask_and_compose_match_definition(t):
    rng = np.random.default_rng(1000 + t)
    for w, h in SHAPES:
        for smooth in (False, True):
            a = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
            if smooth:   # small steps, so that some pixels fall below the larger thresholds
                a = (a // 16 + 100).astype(np.uint8)
            f = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
            m = rc.edge_mask(a, t)
            assert m.dtype == bool and m.shape == (h, w)
            np.testing.assert_array_equal(m, naive_mask(a, t), err_msg=f"{w}x{h} t{t}")
            got = rc.adaptive_compose(a, f, t)
            assert got.dtype == np.uint8 and got.shape == (h, w, 3)
            np.testing.assert_array_equal(got, naive_compose(a, f, t), err_msg=f"{w}x{h} t{t}")


def test_edge_mask_corner_cases():
    one = np.full((1, 1, 3), 200, dtype=np.uint8)
    assert not rc.edge_mask(one, 1).any()          # a 1 x 1 image has contrast 0
    flat = np.full((5, 6, 3), 17, dtype=np.uint8)
    assert not rc.edge_mask(flat, 1).any()
    # one channel of one pixel differs by exactly t: its 3 x 3 neighbourhood is flagged at t and
    # nothing is at t + 1; the extremes 0 / 255 reach t = 255
    for t, lo, hi in ((16, 17, 33), (255, 0, 255)):
        img = np.full((7, 8, 3), lo, dtype=np.uint8)
        img[3, 4, 1] = hi
        want = np.zeros((7, 8), dtype=bool)
        want[2:5, 3:6] = True
        np.testing.assert_array_equal(rc.edge_mask(img, t), want)
        if t < 255:
            assert not rc.edge_mask(img, t + 1).any()
    with pytest.raises(ValueError):
        rc.edge_mask(np.zeros((4, 4, 3), dtype=np.float32), 1)
    with pytest.raises(ValueError):
        rc.adaptive_compose(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 5, 3), np.uint8), 1)


def test_encoding_helpers_and_options():
    assert rc.ssaa_adaptive(4, 16) == 4 | (16 << 8) == 0x1004
    assert rc.ssaa_adaptive(8, 255) == 0xff08 and rc.ssaa_adaptive(2, 0) == 2
    for s in (2, 4, 8):
        for t in (0, 1, 16, 255):
            v = rc.ssaa_adaptive(s, t)
            assert rc.ssaa_factor(v) == s and rc.ssaa_threshold(v) == t
    assert ctypes.sizeof(rc.RcOptions) == 20
    assert rc.options(ssaa=4, adaptive=16).ssaa == 4 | (16 << 8)
    assert rc.options(ssaa=4).ssaa == 4 and rc.options(ssaa=4, adaptive=0).ssaa == 4
    assert ctypes.sizeof(rc.RcAdaptiveStats) == 16
    assert rc.get_tuning(default=True)["adaptive_blocks"] == 0
    assert rc.TUNING_FIELDS[-1] == "adaptive_blocks"
    assert rc.version().startswith("raycast-mi355x 0.3")


def test_tuning_adaptive_blocks_validated():
    for bad in (-1, 4097):
        with pytest.raises(ValueError):
            rc.set_tuning(adaptive_blocks=bad)
    with rc.tuned(adaptive_blocks=4096):
        assert rc.get_tuning()["adaptive_blocks"] == 4096
    assert rc.get_tuning()["adaptive_blocks"] == 0


@pytest.mark.parametrize("factor,value,want_s,want_t,warns", [
    ("4", None, 4, 0, False),
    ("4", "16", 4, 16, False),
    ("2", "1", 2, 1, False),
    ("8", "255", 8, 255, False),
    ("4", "0", 4, 0, True),
    ("4", "256", 4, 0, True),
    ("4", "x", 4, 0, True),
    ("4", "-3", 4, 0, True),
    ("4", "16x", 4, 0, True),
    ("1", "16", 1, 0, True),      # set while the factor is 1: ignored
    (None, "16", 1, 0, True),
])
def test_default_options_adaptive_env(factor, value, want_s, want_t, warns, monkeypatch, capfd):
    for name, v in (("RAYCAST_SSAA", factor), ("RAYCAST_SSAA_ADAPTIVE", value)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    capfd.readouterr()
    opt = rc.default_options(use_env=True)
    assert (opt["ssaa"], opt["adaptive"]) == (want_s, want_t)
    err = capfd.readouterr().err
    if warns:
        assert "Warning" in err and "RAYCAST_SSAA_ADAPTIVE" in err and value in err
    else:
        assert "RAYCAST_SSAA_ADAPTIVE" not in err
    off = rc.default_options(use_env=False)
    assert (off["ssaa"], off["adaptive"]) == (1, 0)
    # the raw field is the encoded value
    raw = rc.RcOptions()
    rc.hip_lib().rc_default_options(ctypes.byref(raw), 1)
    assert raw.ssaa == (rc.ssaa_adaptive(want_s, want_t) if want_t else want_s)
    capfd.readouterr()


@pytest.mark.parametrize("s", [2, 4, 8])
def test_refine_lane_map(s):
    """k_aa_refine's wave restated on the host: lane l serves listed pixel l // (s*s) of the
    step with subsample (i, j) = ((l % (s*s)) % s, (l % (s*s)) // s); the xor butterfly over the
    lane bits 1 .. s*s/2 leaves in every lane the sum of its own group and of no other lane, a
    group covers every subsample once, and one lane per group stores."""
    n = s * s
    rng = np.random.default_rng(s)
    v = rng.integers(0, 256, size=64).astype(np.int64)
    acc = v.copy()
    lanes = np.arange(64)
    m = 1
    while m < n:
        acc = acc + acc[lanes ^ m]
        m <<= 1
    for lane in range(64):
        group = [l for l in range(64) if l // n == lane // n]
        assert acc[lane] == v[group].sum()
    for g in range(64 // n):
        subs = {((l % n) % s, (l % n) // s) for l in range(64) if l // n == g}
        assert subs == {(i, j) for i in range(s) for j in range(s)}
    firsts = [l for l in range(64) if l % n == 0]
    assert len(firsts) == 64 // n == {2: 16, 4: 4, 8: 1}[s]
    # lanes past the list's end hold zeros: a partly filled step still sums the live groups
    live = 64 // n - 1 if n < 64 else 1
    w = np.where(lanes // n < live, v, 0)
    acc = w.copy()
    m = 1
    while m < n:
        acc = acc + acc[lanes ^ m]
        m <<= 1
    for g in range(live):
        assert acc[g * n] == v[g * n:(g + 1) * n].sum()
