"""Progressive supersampling without a GPU: the numpy contract against a plain loop, the built-in
sample sequences, the sequence rules, the layouts, and every refusal of the entry points."""
import ctypes

import numpy as np
import pytest

from helpers import oracle_render, oracle_render_cuda, rc, scene_path

SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 3), (12, 10)]   # (W, H), test_pattern.py's

HIER_PREFIX = {   # the first points of each, written out
    "hier2": (2, [(0, 0), (0, 1), (1, 0), (1, 1)]),
    "hier4": (4, [(0, 0), (0, 2), (2, 0), (2, 2), (0, 1), (0, 3), (2, 1), (2, 3)]),
    "hier8": (8, [(0, 0), (0, 4), (4, 0), (4, 4), (0, 2), (0, 6), (4, 2), (4, 6)]),
}


def loop_resolve(acc):
    h, w = acc.shape[:2]
    out = np.zeros((h, w, 3), dtype=np.uint8)
    for y in range(h):
        for x in range(w):
            n = int(acc[y, x, 3])
            for c in range(3):
                out[y, x, c] = (int(acc[y, x, c]) + n // 2) // n if n else 0
    return out


def loop_contrast(img, x, y):
    """The adaptive contract's contrast, one pixel at a time."""
    h, w = img.shape[:2]
    win = img[max(y - 1, 0):min(y + 2, h), max(x - 1, 0):min(x + 2, w)].astype(int)
    return max(int(win[:, :, c].max() - win[:, :, c].min()) for c in range(3))


def loop_step(acc, out, big, g, points, t, reset):
    """include/raycast_hip.h's pass, one pixel at a time."""
    h, w = out.shape[:2]
    count = len(points)
    acc2, out2 = acc.copy(), out.copy()
    active = saturated = 0
    for y in range(h):
        for x in range(w):
            if not reset and t > 0 and loop_contrast(out, x, y) < t:
                continue
            active += 1
            s = [0, 0, 0, 0] if reset else [int(v) for v in acc[y, x]]
            if s[3] + count > 256:
                saturated += 1
                continue
            for px, py in points:
                for c in range(3):
                    s[c] += int(big[g * y + py, g * x + px, c])
            s[3] += count
            acc2[y, x] = s
            out2[y, x] = [(s[c] + s[3] // 2) // s[3] for c in range(3)]
    return acc2, out2, active, saturated


def random_state(rng, h, w, nmax=256):
    """A valid accumulator: n in 0..nmax, each sum in 0..255 * n."""
    n = rng.integers(0, nmax + 1, size=(h, w), dtype=np.int64)
    acc = np.zeros((h, w, 4), dtype=np.uint16)
    acc[:, :, :3] = (rng.random((h, w, 3)) * (255 * n[:, :, None] + 1)).astype(np.int64).clip(
        0, 255 * n[:, :, None])
    acc[:, :, 3] = n
    return acc


def test_resolve_equals_the_loop():
    rng = np.random.default_rng(11)
    acc = random_state(rng, 9, 13)
    acc[0, 0] = (0, 0, 0, 0)
    acc[0, 1] = (255, 0, 128, 1)
    acc[0, 2] = (65280, 0, 32640, 256)
    acc[0, 3] = (7, 8, 9, 5)       # halves round up: (7 + 2) // 5, (8 + 2) // 5
    got = rc.accum_resolve(acc)
    assert got.dtype == np.uint8 and got.shape == (9, 13, 3)
    np.testing.assert_array_equal(got, loop_resolve(acc))
    assert got[0, 0].tolist() == [0, 0, 0] and got[0, 1].tolist() == [255, 0, 128]
    assert got[0, 2].tolist() == [255, 0, 128] and got[0, 3].tolist() == [1, 2, 2]
    for bad in (acc.astype(np.int32), acc[:, :, :3], acc[0]):
        with pytest.raises(ValueError):
            rc.accum_resolve(bad)


@pytest.mark.parametrize("name", ["hier2", "hier4", "hier8", "rgss4", "queens8"])
def test_numpy_contract_equals_the_loop(name):
    g, pts = rc.SAMPLE_SEQS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    for w, h in SHAPES:
        big = rng.integers(0, 256, size=(g * h, g * w, 3), dtype=np.uint8)
        out = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        acc = random_state(rng, h, w)
        acc[0, 0, 3] = 256     # a saturated pixel in every state
        cases = [(pts[:1], 0, True), (pts[:3], 0, False), (pts[1:2], 40, False),
                 (pts[:min(len(pts), 16)], 0, False), (pts[-1:], 1, False), (pts[:2], 255, False)]
        for points, t, reset in cases:
            want = loop_step(acc, out, big, g, points, t, reset)
            got = rc.accum_step(acc, out, big, g, points, t, reset)
            tag = f"{name} {w}x{h} {len(points)} t{t} reset{reset}"
            assert got[0].dtype == np.uint16 and got[1].dtype == np.uint8, tag
            np.testing.assert_array_equal(got[0], want[0], err_msg=tag)
            np.testing.assert_array_equal(got[1], want[1], err_msg=tag)
            assert got[2:] == want[2:], tag
            if not reset:
                assert got[3] >= 1 or t > 0, tag   # the n = 256 pixel is counted when active


def test_step_leaves_its_arguments_alone_and_refuses():
    rng = np.random.default_rng(3)
    big = rng.integers(0, 256, size=(12, 16, 3), dtype=np.uint8)
    out = rng.integers(0, 256, size=(3, 4, 3), dtype=np.uint8)
    acc = random_state(rng, 3, 4, 8)
    keep = acc.copy(), out.copy()
    rc.accum_step(acc, out, big, 4, [(1, 2)], 16)
    np.testing.assert_array_equal(acc, keep[0])
    np.testing.assert_array_equal(out, keep[1])
    for kw in (dict(points=[]), dict(points=[(0, 0)] * 17), dict(points=[(4, 0)]), dict(g=3),
               dict(t=256), dict(t=-1), dict(t=5, reset=True), dict(big=big[:11]),
               dict(out=out[:2]), dict(acc=acc.astype(np.uint32))):
        a = dict(acc=acc, out=out, big=big, g=4, points=[(1, 2)], t=0, reset=False)
        a.update(kw)
        with pytest.raises(ValueError):
            rc.accum_step(**a)
    for dense in (0, 5):
        with pytest.raises(ValueError):
            rc.accum_run(big, 4, rc.SAMPLE_SEQS["rgss4"][1], dense)


def test_run_in_any_split_is_the_mean():
    """A reset pass and t = 0 passes that cover seq[0..k) give the k-sample mean whatever the
    split, for every k, powers of two or not."""
    g, pts = rc.SAMPLE_SEQS["hier4"]
    rng = np.random.default_rng(8)
    big = rng.integers(0, 256, size=(4 * 5, 4 * 6, 3), dtype=np.uint8)
    zero_acc, zero_out = np.zeros((5, 6, 4), np.uint16), np.zeros((5, 6, 3), np.uint8)
    for k in range(1, 17):
        total = sum(big[y::4, x::4].astype(np.uint32) for x, y in pts[:k])
        mean = ((total + k // 2) // k).astype(np.uint8)
        np.testing.assert_array_equal(rc.accum_run(big, g, pts[:k], k), mean)
        np.testing.assert_array_equal(rc.accum_run(big, g, pts[:k], 1), mean)
        acc, out, active, sat = rc.accum_step(zero_acc, zero_out, big, g, pts[:k], 0, True)
        np.testing.assert_array_equal(out, mean)
        assert (acc[:, :, 3] == k).all() and (active, sat) == (30, 0)


def make(g, pts, n=None):
    s = rc.RcSampleSeq()
    s.grid = g
    s.nsamples = len(pts) if n is None else n
    for k, (x, y) in enumerate(pts[:64]):
        s.x[k], s.y[k] = x, y
    return s


def test_builtin_sequences():
    lib = rc.hip_lib()
    assert set(rc.SAMPLE_SEQS) == set(rc.PATTERNS) | set(HIER_PREFIX)
    for name, (g, pts) in rc.PATTERNS.items():     # the patterns' points in their order
        assert rc.SAMPLE_SEQS[name] == (g, pts), name
    for name, (g, first) in HIER_PREFIX.items():
        sg, pts = rc.SAMPLE_SEQS[name]
        assert sg == g and pts[:len(first)] == first, name
        # a bijection onto the lattice
        assert len(pts) == g * g and set(pts) == {(x, y) for x in range(g) for y in range(g)}
        # coarse to fine: the first 4^j points are the lattice of stride g / 2^j
        for j in range(g.bit_length()):
            step = g >> j
            assert set(pts[:4 ** j]) == {(x, y) for x in range(0, g, step)
                                         for y in range(0, g, step)}, (name, j)
    for name, (g, pts) in rc.SAMPLE_SEQS.items():
        s = rc.RcSampleSeq()
        assert lib.rc_sample_seq_builtin(name.encode(), ctypes.byref(s)) == 0
        assert (s.grid, s.nsamples) == (g, len(pts)), name
        assert [(s.x[k], s.y[k]) for k in range(s.nsamples)] == pts, name
        assert all(s.x[k] == 0 and s.y[k] == 0 for k in range(s.nsamples, 64))
        assert lib.rc_sample_seq_check(ctypes.byref(s)) == 0
        assert rc.sample_seq(name) == (g, pts)
        assert rc.sample_seq_check(g, pts) == len(pts)
    s = rc.RcSampleSeq()
    for bad in (b"", b"hier", b"hier3", b"hier16", b"HIER4", b"rgss", b"hier4 "):
        assert lib.rc_sample_seq_builtin(bad, ctypes.byref(s)) == -1
    assert lib.rc_sample_seq_builtin(None, ctypes.byref(s)) == -1
    assert lib.rc_sample_seq_builtin(b"hier4", None) == -1
    with pytest.raises(ValueError):
        rc.sample_seq("hier3")


def rooks(n, g):
    return [(k % g, (k // g) % g) for k in range(n)]


BAD = {"n = 0": ((2, []), "samples"),
       "n > g*g": ((2, rooks(4, 2) + [(0, 0)]), "samples"),
       "n = 65": ((8, rooks(64, 8) + [(0, 0)]), "samples"),
       "g = 1": ((1, [(0, 0)]), "grid"),
       "g = 3": ((3, rooks(4, 3)), "grid"),
       "g = 16": ((16, rooks(4, 16)), "grid"),
       "x >= g": ((4, [(1, 0), (4, 1), (0, 2)]), "off the"),
       "y >= g": ((4, [(1, 0), (3, 1), (0, 4)]), "off the"),
       "duplicate": ((4, [(1, 0), (3, 1), (1, 0)]), "(1, 0)")}


@pytest.mark.parametrize("rule", sorted(BAD))
def test_check_refuses(rule, capfd):
    (g, pts), word = BAD[rule]
    with pytest.raises(ValueError, match=word.replace("(", r"\(").replace(")", r"\)")):
        rc.sample_seq_check(g, pts)
    with pytest.raises(ValueError):
        rc.sample_seq((g, pts))
    capfd.readouterr()
    assert rc.hip_lib().rc_sample_seq_check(ctypes.byref(make(g, pts, len(pts)))) == -1
    err = capfd.readouterr().err
    assert "rc_sample_seq_check" in err and word in err   # the message names the rule


def test_check_null_and_accepts(capfd):
    assert rc.hip_lib().rc_sample_seq_check(None) == -1
    assert "rc_sample_seq_check" in capfd.readouterr().err
    for g, pts in ((2, [(1, 1)]), (4, rooks(3, 4)), (8, rooks(11, 8)), (2, rooks(4, 2)),
                   (4, rooks(16, 4)), (8, rooks(64, 8))):
        assert rc.sample_seq_check(g, pts) == len(pts)
        assert rc.hip_lib().rc_sample_seq_check(ctypes.byref(make(g, pts))) == 0
    assert capfd.readouterr().err == ""


def test_layout_and_exports():
    assert ctypes.sizeof(rc.RcAccumPx) == 8
    assert (rc.RcAccumPx.sum.offset, rc.RcAccumPx.n.offset) == (0, 6)
    assert ctypes.sizeof(rc.RcSampleSeq) == 136
    assert (rc.RcSampleSeq.grid.offset, rc.RcSampleSeq.nsamples.offset, rc.RcSampleSeq.x.offset,
            rc.RcSampleSeq.y.offset) == (0, 4, 8, 72)
    assert ctypes.sizeof(rc.RcAccumStats) == 32
    assert [n for n, _ in rc.RcAccumStats._fields_] == ["passes", "active_pixels", "saturated",
                                                        "rays"]
    assert rc.ACCUM_MAX_SAMPLES == 64
    lib = rc.hip_lib()
    for name in ("rc_sample_seq_builtin", "rc_sample_seq_check", "rc_accum_pass_device",
                 "rc_accum_resolve_device", "rc_render_accum", "rc_accum_stats_get",
                 "rc_accum_phase_ms"):
        assert name in rc.HIP_EXPORTS, name
        assert hasattr(lib, name), name
    # the pinned layouts are untouched
    assert ctypes.sizeof(rc.RcOptions) == 20
    assert rc.TUNING_FIELDS[-1] == "adaptive_blocks"
    assert rc.version().startswith("raycast-mi355x 0.3")
    assert set(rc.PATTERNS) == {"diag2", "rgss4", "checker8", "queens8"}


def test_refusals_come_before_any_device_work(capfd):
    """Everything the accumulation entry points refuse is refused from the arguments alone, before
    the first HIP call: the refusals hold on a machine without a GPU, each with a message that
    says why, and the pixmap is untouched."""
    sc = rc.Scene.from_file(scene_path("simple"))
    lib = rc.hip_lib()
    fake = 4096   # a non-null, 8-byte aligned "device pointer" that a refused call never follows
    base = np.random.default_rng(5).integers(0, 256, size=(8, 8, 3), dtype=np.uint8)
    out = base.copy()
    host = out.ctypes.data_as(ctypes.c_void_p)
    good = make(*rc.SAMPLE_SEQS["rgss4"])

    def both(word, opt, s, t=0, w=8, h=8, first=0, count=1, reset=0, dense=1):
        ps = ctypes.byref(s) if s is not None else None
        po = ctypes.byref(opt) if opt is not None else None
        capfd.readouterr()
        assert lib.rc_render_accum(sc.packed(), w, h, po, ps, dense, t, host, None) == -1
        err = capfd.readouterr().err
        assert "Error: rc_" in err and word in err, err
        assert lib.rc_accum_pass_device(sc.packed(), w, h, po, ps, first, count, t, reset, fake,
                                        fake, None, None) == -1
        err = capfd.readouterr().err
        assert "Error: rc_" in err and word in err, err

    def pass_only(word, **kw):
        a = dict(w=8, h=8, s=good, first=0, count=1, t=0, reset=0, acc=fake, out=fake)
        a.update(kw)
        opt = rc.options(6, "fast")
        capfd.readouterr()
        assert lib.rc_accum_pass_device(
            sc.packed(), a["w"], a["h"], ctypes.byref(opt), ctypes.byref(a["s"]), a["first"],
            a["count"], a["t"], a["reset"], a["acc"], a["out"], None, None) == -1, kw
        err = capfd.readouterr().err
        assert "Error: rc_accum_pass_device" in err and word in err, err

    # parity mode, with the family's sentence about the scan-order carry
    both("scan-order carry", rc.options(6, "parity"), good)
    both("scan-order carry", rc.options(6, "parity"), good, 32)
    for mode in ("fast", "cuda"):
        # a factor above 1 or a threshold in the options; more than one GPU
        for bad in (dict(ssaa=2), dict(ssaa=4), dict(ssaa=8), dict(ssaa=4, adaptive=16)):
            both("ssaa", rc.options(6, mode, **bad), good)
        for bad in (dict(ssaa=3), dict(ssaa=-1), dict(ssaa=1, adaptive=16)):
            both("ssaa", rc.options(6, mode, **bad), good)
        both("num_gpus", rc.options(6, mode, gpus=2), good)
        # a sequence that fails the check, a null sequence
        for (g, pts), word in BAD.values():
            both(word, rc.options(6, mode), make(g, pts, len(pts)))
        both("null pointer", rc.options(6, mode), None)
        # the threshold
        for t in (-1, 256, 1 << 16):
            both("threshold", rc.options(6, mode), good, t)
        # the size limits: W, H in 1 .. 2^28 / g
        for w, h in (((1 << 26) + 1, 1), (1, (1 << 26) + 1), (0, 8), (8, 0), (-1, 8)):
            both("2^28", rc.options(6, mode), good, 0, w, h)
        both("2^28", rc.options(6, mode), make(*rc.SAMPLE_SEQS["hier8"]), 0, (1 << 25) + 1, 1)
        both("2^28", rc.options(6, mode), make(*rc.SAMPLE_SEQS["hier2"]), 0, 1, (1 << 27) + 1)
        # with a threshold, W * H < 2^32 (both sides within 2^28 / g)
        both("32-bit", rc.options(6, mode), good, 16, 1 << 16, 1 << 16)
        both("32-bit", rc.options(6, mode), good, 1, 1 << 26, 64)
        # the tile-row limit of the dense kernel's grid: 65535 rows of 16-row tiles
        both("rows of tiles", rc.options(6, mode), good, 0, 1, 65535 * 16 + 1)
    # first and count: 1 <= count <= 16, first + count <= nsamples
    for first, count in ((0, 0), (0, -1), (0, 17), (-1, 1), (4, 1), (3, 2), (0, 5),
                         (1 << 30, 1 << 30)):
        pass_only("inside the sequence", first=first, count=count)
    pass_only("inside the sequence", s=make(*rc.SAMPLE_SEQS["hier8"]), first=0, count=17)
    # reset with a threshold
    pass_only("reset", reset=1, t=16)
    # dense: 1 <= dense <= nsamples
    opt = rc.options(6, "fast")
    for dense in (0, -1, 5, 1 << 30):
        capfd.readouterr()
        assert lib.rc_render_accum(sc.packed(), 8, 8, ctypes.byref(opt), ctypes.byref(good), dense,
                                   0, host, None) == -1
        assert "dense" in capfd.readouterr().err
    # null pointers, a misaligned accumulator
    g = ctypes.byref(good)
    assert lib.rc_render_accum(None, 8, 8, ctypes.byref(opt), g, 1, 0, host, None) == -1
    assert lib.rc_render_accum(sc.packed(), 8, 8, ctypes.byref(opt), g, 1, 0, None, None) == -1
    assert lib.rc_render_accum(sc.packed(), 8, 8, None, g, 1, 0, host, None) == -1
    assert lib.rc_accum_pass_device(None, 8, 8, ctypes.byref(opt), g, 0, 1, 0, 1, fake, fake, None,
                                    None) == -1
    assert "null pointer" in capfd.readouterr().err
    pass_only("null pointer", acc=None)
    pass_only("null pointer", out=None)
    pass_only("aligned", acc=fake + 4)
    for acc, img, w, h, word in ((None, fake, 8, 8, "null pointer"), (fake, None, 8, 8, "null"),
                                 (fake + 2, fake, 8, 8, "aligned"), (fake, fake, 0, 8, "sides"),
                                 (fake, fake, 8, -1, "sides"),
                                 (fake, fake, 1 << 28, 1 << 28, "sides")):
        capfd.readouterr()
        assert lib.rc_accum_resolve_device(acc, w, h, img, None) == -1
        err = capfd.readouterr().err
        assert "Error: rc_accum_resolve_device" in err and word in err, err
    assert lib.rc_accum_stats_get(None) == -1 and lib.rc_accum_phase_ms(None) == -1
    # the Python wrappers raise
    with pytest.raises(RuntimeError):
        rc.render_accum(sc, 8, 8, "rgss4", mode="parity", out=out)
    with pytest.raises(RuntimeError):
        rc.accum_pass_device(sc, 1 << 27, 8, "rgss4", 0, 1, fake, fake)
    with pytest.raises(RuntimeError):
        rc.render_accum(sc, 8, 8, "rgss4", threshold=256, out=out)
    with pytest.raises(RuntimeError):
        rc.accum_resolve_device(fake, 0, 8, fake)
    with pytest.raises(ValueError):
        rc.render_accum(sc, 8, 8, BAD["duplicate"][0], out=out)
    with pytest.raises(ValueError):
        rc.accum_pass_device(sc, 8, 8, "hier", 0, 1, fake, fake)
    np.testing.assert_array_equal(out, base)
    capfd.readouterr()


@pytest.mark.parametrize("scene", ["simple", "quadric"])
def test_run_identities_on_the_oracle(scene):
    """On the oracle's own g*W x g*H images: every sample for every pixel is the pattern image,
    and the whole lattice is the box filter."""
    sc = rc.Scene.from_file(scene_path(scene))
    w, h = 12, 10
    big = {g: oracle_render(sc, g * w, g * h, 6, "fast")[0] for g in (2, 4, 8)}
    for name, (g, pts) in rc.PATTERNS.items():
        want = rc.pattern_downsample(big[g], g, pts)
        np.testing.assert_array_equal(rc.accum_run(big[g], g, pts, len(pts), 0), want, err_msg=name)
        np.testing.assert_array_equal(rc.accum_run(big[g], g, pts, 1, 0), want, err_msg=name)
    for g in (2, 4, 8):
        pts = rc.SAMPLE_SEQS[f"hier{g}"][1]
        want = rc.box_downsample(big[g], g)
        assert (want != big[g][::g, ::g]).any()     # not the one-ray image of the first point
        np.testing.assert_array_equal(rc.accum_run(big[g], g, pts, g * g, 0), want)
        np.testing.assert_array_equal(rc.accum_run(big[g], g, pts, 3, 0), want)
    cuda = oracle_render_cuda(sc, 4 * w, 4 * h, 50)
    np.testing.assert_array_equal(rc.accum_run(cuda, 4, rc.SAMPLE_SEQS["hier4"][1], 16, 0),
                                  rc.box_downsample(cuda, 4))
