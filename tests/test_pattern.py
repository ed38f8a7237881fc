"""Sparse sample patterns (rc_pattern), the parts that need no GPU: the contract in numpy against
a per-pixel double loop, the built-in tables, the pattern rules in Python and in the library, the
refusals, RAYCAST_PATTERN, and the kernels' lane maps restated on the host."""
import ctypes

import numpy as np
import pytest

from helpers import rc, scene_path

SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 3), (12, 10)]   # (W, H), test_adaptive.py's

TABLE = {   # the issue's table, written out
    "diag2": (2, [(0, 0), (1, 1)]),
    "rgss4": (4, [(1, 0), (3, 1), (0, 2), (2, 3)]),
    "checker8": (4, [(0, 0), (2, 0), (1, 1), (3, 1), (0, 2), (2, 2), (1, 3), (3, 3)]),
    "queens8": (8, [(3, 0), (6, 1), (2, 2), (7, 3), (1, 4), (4, 5), (0, 6), (5, 7)]),
}
ASYM2 = (8, [(7, 0), (1, 3)])
CUST16 = (8, [((5 * k + 3) % 8, k // 2) for k in range(16)])


def loop_pattern(big, g, points):
    """include/raycast_hip.h's pattern contract, one output pixel at a time."""
    h, w, ch = big.shape[0] // g, big.shape[1] // g, big.shape[2]
    n = len(points)
    out = np.zeros((h, w, ch), dtype=np.uint8)
    for y in range(h):
        for x in range(w):
            for c in range(ch):
                acc = 0
                for px, py in points:
                    acc += int(big[g * y + py, g * x + px, c])
                out[y, x, c] = (acc + n // 2) // n
    return out


@pytest.mark.parametrize("name", sorted(TABLE) + ["asym2", "cust16"])
def test_numpy_contract_equals_the_loop(name):
    g, pts = {"asym2": ASYM2, "cust16": CUST16}.get(name) or TABLE[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    for w, h in SHAPES:
        big = rng.integers(0, 256, size=(g * h, g * w, 3), dtype=np.uint8)
        got = rc.pattern_downsample(big, g, pts)
        assert got.dtype == np.uint8 and got.shape == (h, w, 3)
        np.testing.assert_array_equal(got, loop_pattern(big, g, pts), err_msg=f"{name} {w}x{h}")


@pytest.mark.parametrize("g", [2, 4])
def test_full_patterns_are_the_box_filter(g):
    pts = [(i, j) for j in range(g) for i in range(g)]
    rng = np.random.default_rng(70 + g)
    for w, h in SHAPES:
        big = rng.integers(0, 256, size=(g * h, g * w, 3), dtype=np.uint8)
        np.testing.assert_array_equal(rc.pattern_downsample(big, g, pts),
                                      rc.box_downsample(big, g))
        # the order of the samples does not matter
        np.testing.assert_array_equal(rc.pattern_downsample(big, g, pts[::-1]),
                                      rc.box_downsample(big, g))


def test_builtin_tables():
    assert set(rc.PATTERNS) == set(TABLE)
    lib = rc.hip_lib()
    for name, (g, pts) in TABLE.items():
        assert rc.PATTERNS[name] == (g, pts), name
        assert rc.pattern(name) == (g, pts)
        p = rc.RcPattern()
        assert lib.rc_pattern_builtin(name.encode(), ctypes.byref(p)) == 0
        assert (p.grid, p.nsamples) == (g, len(pts))
        assert [(p.x[k], p.y[k]) for k in range(p.nsamples)] == pts, name
        assert all(p.x[k] == 0 and p.y[k] == 0 for k in range(p.nsamples, 16))
        assert lib.rc_pattern_check(ctypes.byref(p)) == 0
    # N-rooks: rgss4 and queens8 have no two samples in a row or a column; queens8 none on a
    # diagonal either
    for name in ("rgss4", "queens8"):
        g, pts = TABLE[name]
        assert sorted(x for x, _ in pts) == sorted(y for _, y in pts) == list(range(g))
    g, pts = TABLE["queens8"]
    assert len({x + y for x, y in pts}) == len({x - y for x, y in pts}) == 8
    p = rc.RcPattern()
    for bad in (b"", b"rgss", b"RGSS4", b"rgss4 ", b"queens"):
        assert lib.rc_pattern_builtin(bad, ctypes.byref(p)) == -1
    assert lib.rc_pattern_builtin(None, ctypes.byref(p)) == -1
    assert lib.rc_pattern_builtin(b"rgss4", None) == -1
    with pytest.raises(ValueError):
        rc.pattern("rgss")


def make(g, pts, n=None):
    p = rc.RcPattern()
    p.grid = g
    p.nsamples = len(pts) if n is None else n
    for k, (x, y) in enumerate(pts[:16]):
        p.x[k], p.y[k] = x, y
    return p


def rooks(n, g):
    return [(k % g, k // g) for k in range(n)]


BAD = {"n = 1": (2, rooks(1, 2)),
       "n = 3": (2, rooks(3, 2)),
       "n = 32": (8, rooks(32, 8)),
       "n > g*g": (2, rooks(8, 4)),
       "g = 1": (1, [(0, 0), (0, 0)]),
       "g = 3": (3, rooks(4, 3)),
       "g = 16": (16, rooks(4, 16)),
       "x >= g": (4, [(1, 0), (4, 1), (0, 2), (2, 3)]),
       "y >= g": (4, [(1, 0), (3, 1), (0, 4), (2, 3)]),
       "duplicate": (4, [(1, 0), (3, 1), (1, 0), (2, 3)])}


@pytest.mark.parametrize("rule", sorted(BAD))
def test_check_refuses(rule, capfd):
    g, pts = BAD[rule]
    with pytest.raises(ValueError):
        rc.pattern_check(g, pts)
    with pytest.raises(ValueError):
        rc.pattern((g, pts))
    capfd.readouterr()
    assert rc.hip_lib().rc_pattern_check(ctypes.byref(make(g, pts))) == -1
    assert "rc_pattern_check" in capfd.readouterr().err   # a message names the rule


def test_check_null_and_accepts(capfd):
    assert rc.hip_lib().rc_pattern_check(None) == -1
    assert "rc_pattern_check" in capfd.readouterr().err
    for g, pts in list(TABLE.values()) + [ASYM2, CUST16, (2, rooks(4, 2)), (4, rooks(16, 4)),
                                          (8, rooks(16, 8)), (2, [(1, 0), (0, 1)])]:
        assert rc.pattern_check(g, pts) == len(pts)
        assert rc.hip_lib().rc_pattern_check(ctypes.byref(make(g, pts))) == 0
    assert len(set(CUST16[1])) == 16
    assert capfd.readouterr().err == ""


def test_downsample_refuses_bad_images():
    big = np.zeros((8, 8, 3), dtype=np.uint8)
    g, pts = TABLE["rgss4"]
    for bad in (big.astype(np.int32), big[:7], big[:, :7], big[0]):
        with pytest.raises(ValueError):
            rc.pattern_downsample(bad, g, pts)
    with pytest.raises(ValueError):
        rc.pattern_downsample(big, 4, pts[:3])


def test_layout_and_exports():
    assert ctypes.sizeof(rc.RcPattern) == 40
    assert [n for n, _ in rc.RcPattern._fields_] == ["grid", "nsamples", "x", "y"]
    assert (rc.RcPattern.grid.offset, rc.RcPattern.nsamples.offset, rc.RcPattern.x.offset,
            rc.RcPattern.y.offset) == (0, 4, 8, 24)
    assert ctypes.sizeof(rc.RcPatternStats) == 16
    assert rc.PATTERN_MAX_SAMPLES == 16
    lib = rc.hip_lib()
    for name in ("rc_pattern_builtin", "rc_pattern_check", "rc_pattern_env", "rc_render_pattern",
                 "rc_render_pattern_device", "rc_pattern_stats_get", "rc_pattern_phase_ms"):
        assert name in rc.HIP_EXPORTS, name
        assert hasattr(lib, name), name
    # the pinned layouts are untouched
    assert ctypes.sizeof(rc.RcOptions) == 20
    assert rc.TUNING_FIELDS[-1] == "adaptive_blocks"
    assert rc.version().startswith("raycast-mi355x 0.3")


def test_refusals_come_before_any_device_work(capfd):
    """Everything the pattern entry points refuse is refused from the arguments alone, before the
    first HIP call: the refusals hold on a machine without a GPU, each with a message, and the
    pixmap is untouched."""
    sc = rc.Scene.from_file(scene_path("simple"))
    lib = rc.hip_lib()
    fake = 4096   # a non-null "device pointer" that a refused call never follows
    base = np.random.default_rng(5).integers(0, 256, size=(8, 8, 3), dtype=np.uint8)
    out = base.copy()
    host = out.ctypes.data_as(ctypes.c_void_p)
    good = make(*TABLE["rgss4"])

    def both(opt, p, t=0, w=8, h=8):
        pp = ctypes.byref(p) if p is not None else None
        po = ctypes.byref(opt) if opt is not None else None
        capfd.readouterr()
        assert lib.rc_render_pattern(sc.packed(), w, h, po, pp, t, host, None) == -1
        assert "Error: rc_" in capfd.readouterr().err
        assert lib.rc_render_pattern_device(sc.packed(), w, h, po, pp, t, fake, None, None) == -1
        assert "Error: rc_" in capfd.readouterr().err

    # parity mode, with and without a threshold
    both(rc.options(6, "parity"), good)
    both(rc.options(6, "parity"), good, 32)
    for mode in ("fast", "cuda"):
        # a factor above 1 or a threshold in the options; more than one GPU
        for bad in (dict(ssaa=2), dict(ssaa=4), dict(ssaa=8), dict(ssaa=3), dict(ssaa=-1),
                    dict(ssaa=4, adaptive=16), dict(ssaa=1, adaptive=16), dict(gpus=2)):
            both(rc.options(6, mode, **bad), good)
        # a pattern that fails the check, a null pattern
        for g, pts in BAD.values():
            both(rc.options(6, mode), make(g, pts))
        both(rc.options(6, mode), None)
        # the threshold
        for t in (-1, 256, 1 << 16):
            both(rc.options(6, mode), good, t)
        # the size limits: W, H <= 2^28 / g; nothing below 1
        for w, h in (((1 << 26) + 1, 1), (1, (1 << 26) + 1), (0, 8), (8, 0), (-1, 8)):
            both(rc.options(6, mode), good, 0, w, h)
        both(rc.options(6, mode), make(*TABLE["queens8"]), 0, (1 << 25) + 1, 1)
        both(rc.options(6, mode), make(*TABLE["diag2"]), 0, 1, (1 << 27) + 1)
        # with a threshold, W * H < 2^32 (both sides within 2^28 / g)
        both(rc.options(6, mode), good, 16, 1 << 16, 1 << 16)
        both(rc.options(6, mode), good, 1, 1 << 26, 64)
    # ssaa = 0 and 1 both mean "off" and pass the options' check: only the null scene refuses
    opt = rc.options(6, "fast", ssaa=0)
    g = ctypes.byref(good)
    assert lib.rc_render_pattern(None, 8, 8, ctypes.byref(opt), g, 0, host, None) == -1
    assert lib.rc_render_pattern_device(None, 8, 8, ctypes.byref(opt), g, 0, fake, None, None) == -1
    # the other null pointers
    assert lib.rc_render_pattern(sc.packed(), 8, 8, ctypes.byref(opt), g, 0, None, None) == -1
    assert lib.rc_render_pattern_device(sc.packed(), 8, 8, ctypes.byref(opt), g, 0, None, None,
                                        None) == -1
    both(None, good)
    assert lib.rc_pattern_stats_get(None) == -1 and lib.rc_pattern_phase_ms(None) == -1
    # the Python wrappers raise
    with pytest.raises(RuntimeError):
        rc.render_pattern(sc, 8, 8, "rgss4", mode="parity", out=out)
    with pytest.raises(RuntimeError):
        rc.render_pattern_device(sc, 1 << 27, 8, "rgss4", fake)
    with pytest.raises(RuntimeError):
        rc.render_pattern(sc, 8, 8, "rgss4", threshold=256, out=out)
    with pytest.raises(ValueError):
        rc.render_pattern(sc, 8, 8, BAD["duplicate"], out=out)
    with pytest.raises(ValueError):
        rc.render_pattern_device(sc, 8, 8, "rgss", fake)
    np.testing.assert_array_equal(out, base)
    capfd.readouterr()


def test_env_decision(monkeypatch, capfd):
    """RAYCAST_PATTERN as raycast() reads it (rc_pattern_env): a built-in name, alone or with a
    threshold, goes through the pattern path in fast and cuda mode with no ssaa factor;
    everything else warns and keeps today's path."""
    monkeypatch.delenv("RAYCAST_PATTERN", raising=False)
    for mode in ("fast", "cuda", "parity"):
        assert rc.pattern_from_env(mode) is None
    assert capfd.readouterr().err == ""          # unset: silent, today's behaviour
    for name, (g, pts) in TABLE.items():
        monkeypatch.setenv("RAYCAST_PATTERN", name)
        for mode in ("fast", "cuda"):
            assert rc.pattern_from_env(mode) == (g, pts, 0)
            assert rc.pattern_from_env(mode, ssaa=0) == (g, pts, 0)
        for t in (0, 1, 32, 255):
            monkeypatch.setenv("RAYCAST_PATTERN", f"{name}:{t}")
            assert rc.pattern_from_env("fast") == (g, pts, t)
    assert capfd.readouterr().err == ""
    for bad in ("rgss", "", "RGSS4", "rgss4 ", ":16", "box"):          # a bad name
        monkeypatch.setenv("RAYCAST_PATTERN", bad)
        assert rc.pattern_from_env("fast") is None
        err = capfd.readouterr().err
        assert err.startswith("Warning: RAYCAST_PATTERN") and "ignored" in err
    for bad in ("rgss4:", "rgss4:256", "rgss4:-1", "rgss4:x", "rgss4:16x", "rgss4:1:2",
                "rgss4: 16"):                                           # a bad threshold
        monkeypatch.setenv("RAYCAST_PATTERN", bad)
        assert rc.pattern_from_env("fast") is None
        err = capfd.readouterr().err
        assert err.startswith("Warning: RAYCAST_PATTERN") and "threshold" in err
    monkeypatch.setenv("RAYCAST_PATTERN", "rgss4:32")
    assert rc.pattern_from_env("parity") is None                        # parity mode
    err = capfd.readouterr().err
    assert err.startswith("Warning: RAYCAST_PATTERN") and "parity" in err
    for s in (2, 4, 8):                                                 # RAYCAST_SSAA set as well
        assert rc.pattern_from_env("fast", ssaa=s) is None
        err = capfd.readouterr().err
        assert err.startswith("Warning: RAYCAST_PATTERN") and "RAYCAST_SSAA" in err
    assert rc.pattern_from_env("fast", ssaa=4, adaptive=16) is None
    assert "RAYCAST_SSAA" in capfd.readouterr().err
    # through the environment as raycast() sees it: rc_default_options, then rc_pattern_env
    monkeypatch.setenv("RAYCAST_MODE", "fast")
    monkeypatch.setenv("RAYCAST_SSAA", "2")
    raw = rc.RcOptions()
    rc.hip_lib().rc_default_options(ctypes.byref(raw), 1)
    p, t = rc.RcPattern(), ctypes.c_int(-7)
    assert rc.hip_lib().rc_pattern_env(ctypes.byref(raw), ctypes.byref(p), ctypes.byref(t)) == 0
    assert t.value == -7 and "RAYCAST_SSAA 2" in capfd.readouterr().err
    monkeypatch.setenv("RAYCAST_SSAA", "1")
    rc.hip_lib().rc_default_options(ctypes.byref(raw), 1)
    assert rc.hip_lib().rc_pattern_env(ctypes.byref(raw), ctypes.byref(p), ctypes.byref(t)) == 1
    assert (p.grid, p.nsamples, t.value) == (4, 4, 32)
    assert rc.hip_lib().rc_pattern_env(None, ctypes.byref(p), ctypes.byref(t)) == 0
    assert capfd.readouterr().err == ""


@pytest.mark.parametrize("n", [2, 4, 8, 16])
def test_lane_maps(n):
    """The pattern kernels' waves restated on the host.  Lane l serves pixel group l // n with
    sample l % n, taken out of a 64-bit word of 4-bit entries; the xor butterfly over the lane
    bits 1 .. n/2 leaves in every lane the sum of its own group; one lane a group stores.  Dense
    form: a wave's 64 / n groups are a compact block, the workgroup's four waves a tile of
    256 / n pixels, each pixel once."""
    ln = n.bit_length() - 1
    lanes = np.arange(64)
    rng = np.random.default_rng(n)
    v = rng.integers(0, 256, size=64).astype(np.int64)
    live = np.where(lanes // n < max(64 // n - 1, 1), v, 0)   # the last group past the list
    for w in (v, live):
        acc = w.copy()
        m = 1
        while m < n:
            acc = acc + acc[lanes ^ m]
            m <<= 1
        for lane in range(64):
            g0 = (lane // n) * n
            assert acc[lane] == w[g0:g0 + n].sum()
    assert [l for l in range(64) if l % n == 0] == list(range(0, 64, n))
    # the packed words give every lane its own entry
    pts = CUST16[1][:n]
    wx = sum(x << (4 * k) for k, (x, _) in enumerate(pts))
    wy = sum(y << (4 * k) for k, (_, y) in enumerate(pts))
    assert wx < 1 << 64 and wy < 1 << 64
    for lane in range(64):
        k = lane & (n - 1)
        assert ((wx >> (4 * k)) & 15, (wy >> (4 * k)) & 15) == pts[k]
    # the dense form's tile (rc_sample_kernels.hip pat_lbw / pat_lbh)
    lbw, lbh = (7 - ln) // 2, (6 - ln) // 2
    assert (1 << lbw) * (1 << lbh) == 64 // n and lbw >= lbh
    assert (2 << lbw, 2 << lbh) == {2: (16, 8), 4: (8, 8), 8: (8, 4), 16: (4, 4)}[n]
    seen = {}
    for tid in range(256):
        lane, wave = tid & 63, tid >> 6
        grp = lane >> ln
        x = ((wave & 1) << lbw) + (grp & ((1 << lbw) - 1))
        y = ((wave >> 1) << lbh) + (grp >> lbw)
        seen.setdefault((x, y), []).append(lane & (n - 1))
    assert set(seen) == {(x, y) for x in range(2 << lbw) for y in range(2 << lbh)}
    assert all(sorted(s) == list(range(n)) for s in seen.values())
