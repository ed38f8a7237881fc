"""Supersampled anti-aliasing (rc_options.ssaa), the parts that need no GPU: the numpy statement
of the contract, the option's default and environment, and the struct's layout."""
import ctypes

import numpy as np
import pytest

from helpers import rc


def naive_box(img, s):
    """include/raycast_hip.h's definition, one output sample at a time."""
    h, w = img.shape[0] // s, img.shape[1] // s
    out = np.zeros((h, w, 3), dtype=np.uint8)
    for y in range(h):
        for x in range(w):
            for c in range(3):
                total = 0
                for j in range(s):
                    for i in range(s):
                        total += int(img[s * y + j, s * x + i, c])
                out[y, x, c] = (total + s * s // 2) // (s * s)
    return out


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_box_downsample_matches_definition(s):
    rng = np.random.default_rng(100 + s)
    for w, h in ((1, 1), (7, 3), (5, 6)):
        img = rng.integers(0, 256, size=(s * h, s * w, 3), dtype=np.uint8)
        got = rc.box_downsample(img, s)
        assert got.dtype == np.uint8 and got.shape == (h, w, 3)
        np.testing.assert_array_equal(got, naive_box(img, s))


@pytest.mark.parametrize("s", [2, 4, 8])
def test_box_downsample_rounding(s):
    """Constant images stay what they are (255 must not wrap, 0 must not round up), and the
    0 / 255 checkerboard, whose mean is 127.5, rounds up to 128."""
    for v in (0, 255):
        img = np.full((2 * s, 3 * s, 3), v, dtype=np.uint8)
        np.testing.assert_array_equal(rc.box_downsample(img, s), np.full((2, 3, 3), v, np.uint8))
    yy, xx = np.mgrid[0:2 * s, 0:3 * s]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    got = rc.box_downsample(board, s)
    np.testing.assert_array_equal(got, np.full((2, 3, 3), 128, np.uint8))
    np.testing.assert_array_equal(got, naive_box(board, s))
    # one 255 among s*s - 1 zeros: (255 + s*s/2) / (s*s)
    one = np.zeros((s, s, 3), dtype=np.uint8)
    one[s - 1, s - 1] = 255
    assert rc.box_downsample(one, s)[0, 0, 0] == (255 + s * s // 2) // (s * s)


@pytest.mark.parametrize("s", [2, 4, 8])
def test_lane_butterfly_sums_each_group(s):
    """k_render_ssaa's reduction restated on the host: lane = 8*row + col of an 8x8 wave tile,
    xor butterflies over the column masks 1 .. s/2 and the row masks 8 .. 4s leave in every lane
    the sum of its own s x s group and of no other lane."""
    rng = np.random.default_rng(s)
    v = rng.integers(0, 256, size=64).astype(np.int64)
    acc = v.copy()
    lanes = np.arange(64)
    masks = [m for m in (1, 2, 4) if m < s] + [m for m in (8, 16, 32) if m < 8 * s]
    for m in masks:
        acc = acc + acc[lanes ^ m]
    for lane in range(64):
        row, col = lane >> 3, lane & 7
        group = [8 * r + c for r in range(8) for c in range(8)
                 if r // s == row // s and c // s == col // s]
        assert acc[lane] == v[group].sum()
    firsts = [l for l in range(64) if (l & (s - 1)) == 0 and ((l >> 3) & (s - 1)) == 0]
    assert len(firsts) == 64 // (s * s)   # one storing lane per output pixel


def test_box_downsample_rejects_bad_input():
    with pytest.raises(ValueError):
        rc.box_downsample(np.zeros((3, 4, 3), dtype=np.uint8), 2)
    with pytest.raises(ValueError):
        rc.box_downsample(np.zeros((4, 4, 3), dtype=np.float32), 2)


@pytest.mark.parametrize("value,want", [(None, 1), ("2", 2), ("8", 8), ("3", 1), ("x", 1)])
def test_default_options_ssaa_env(value, want, monkeypatch, capfd):
    """rc_default_options: ssaa is 1 unless RAYCAST_SSAA names 1, 2, 4 or 8; anything else
    warns on stderr and leaves 1.  Without use_env the environment is not read."""
    if value is None:
        monkeypatch.delenv("RAYCAST_SSAA", raising=False)
    else:
        monkeypatch.setenv("RAYCAST_SSAA", value)
    capfd.readouterr()
    assert rc.default_options(use_env=True)["ssaa"] == want
    err = capfd.readouterr().err
    if value in ("3", "x"):
        assert "Warning" in err and "RAYCAST_SSAA" in err and value in err
    else:
        assert "RAYCAST_SSAA" not in err
    assert rc.default_options(use_env=False)["ssaa"] == 1


def test_options_layout_and_binding():
    assert ctypes.sizeof(rc.RcOptions) == 20
    assert [n for n, _ in rc.RcOptions._fields_][-1] == "ssaa"
    assert rc.options().ssaa == 1 and rc.options(ssaa=4).ssaa == 4
    assert rc.RcOptions().ssaa == 0   # zero-initialised options: off
    assert rc.get_tuning(default=True)["ssaa_fused"] == 1
