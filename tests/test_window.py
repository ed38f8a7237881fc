"""Windows of a virtual image without a GPU: the numpy contract and the tile and zoom helpers
against plain loops, the layout, every rule of rc_window_check, every refusal of the three entry
points, RAYCAST_WINDOW's reading, and the oracle's two checkers held against each other."""
import ctypes
import os

import numpy as np
import pytest

from helpers import oracle_lib, oracle_render, rc, scene_path

SHAPES = [(1, 1), (1, 9), (9, 1), (7, 3), (12, 10)]   # (W, H)
FACTORS = [1, 2, 4, 8]
INT_MAX = 2 ** 31 - 1


def oracle_pixels(scene, W, H, depth, mode, pix):
    """Oracle per-pixel shade (rco_pixels) of the pixels y*W + x of the W x H image: rgb and
    zero-normalize events."""
    lib = oracle_lib()
    lib.rco_pixels.argtypes = [ctypes.POINTER(rc.JsonDataT)] + [ctypes.c_int] * 4 + [
        ctypes.c_int64] + [ctypes.c_void_p] * 6
    pix = np.ascontiguousarray(pix, dtype=np.int64)
    n = len(pix)
    rgb = np.zeros((n, 3), np.uint8)
    cout = np.zeros((n, 3), np.float32)
    cls = np.zeros(n, np.uint8)
    z = np.zeros(n, np.int64)
    assert lib.rco_pixels(ctypes.byref(scene.js), W, H, depth + 1, rc.MODES[mode], n,
                          pix.ctypes.data, None, rgb.ctypes.data, cout.ctypes.data,
                          cls.ctypes.data, z.ctypes.data) == 0
    return rgb, z


def loop_crop(img, s, window, w, h):
    fw, fh, x0, y0 = window
    out = np.zeros((s * h, s * w, img.shape[2]), dtype=img.dtype)
    for y in range(s * h):
        for x in range(s * w):
            out[y, x] = img[s * y0 + y, s * x0 + x]
    return out


@pytest.mark.parametrize("s", FACTORS)
def test_crop_equals_the_loop(s):
    rng = np.random.default_rng(s)
    for w, h in SHAPES:
        for fw, fh, x0, y0 in ((w, h, 0, 0), (w + 5, h + 3, 5, 3), (w + 5, h + 3, 2, 1),
                               (2 * w + 1, 3 * h, w + 1, 2 * h)):
            img = rng.integers(0, 256, size=(s * fh, s * fw, 3), dtype=np.uint8)
            got = rc.window_crop(img, s, (fw, fh, x0, y0), w, h)
            assert got.shape == (s * h, s * w, 3) and got.dtype == np.uint8
            np.testing.assert_array_equal(got, loop_crop(img, s, (fw, fh, x0, y0), w, h))
    img = np.zeros((s * 6, s * 8, 3), np.uint8)
    np.testing.assert_array_equal(rc.window_crop(img, s, (8, 6, 0, 0), 8, 6), img)   # identity
    for bad in (dict(window=(8, 6, 1, 0)), dict(window=(8, 6, 0, 1)), dict(window=(8, 6, -1, 0)),
                dict(window=(8, 6, 0, 0), w=0), dict(window=(9, 6, 0, 0)), dict(s=3),
                dict(img=img[0])):
        a = dict(img=img, s=s, window=(8, 6, 0, 0), w=8, h=6)
        a.update(bad)
        with pytest.raises(ValueError):
            rc.window_crop(a["img"], a["s"], a["window"], a["w"], a["h"])


def loop_tiles(fw, fh, tw, th):
    tiles = []
    y0 = 0
    while y0 < fh:
        x0 = 0
        while x0 < fw:
            w = tw if x0 + tw <= fw else fw - x0
            h = th if y0 + th <= fh else fh - y0
            tiles.append(((fw, fh, x0, y0), w, h))
            x0 += tw
        y0 += th
    return tiles


def test_tiles_equal_the_loop_and_partition_the_image():
    sizes = SHAPES + [(64, 48), (97, 61)]
    for fw, fh in sizes:
        for tw, th in ((1, 1), (3, 2), (4, 5), (8, 8), (24, 20), (fw, fh), (fw + 3, fh + 1)):
            tiles = rc.window_tiles(fw, fh, tw, th)
            assert tiles == loop_tiles(fw, fh, tw, th)
            count = np.zeros((fh, fw), dtype=np.int64)
            for (tfw, tfh, x0, y0), w, h in tiles:
                assert (tfw, tfh) == (fw, fh) and 1 <= w <= tw and 1 <= h <= th
                count[y0:y0 + h, x0:x0 + w] += 1
            assert (count == 1).all(), (fw, fh, tw, th)
    # 64 x 48 in 24 x 20: the last column 16 wide, the last row 8 tall
    tiles = rc.window_tiles(64, 48, 24, 20)
    assert len(tiles) == 9 and tiles[2] == ((64, 48, 48, 0), 16, 20)
    assert tiles[8] == ((64, 48, 48, 40), 16, 8)
    for bad in ((0, 4, 2, 2), (4, 0, 2, 2), (4, 4, 0, 2), (4, 4, 2, -1)):
        with pytest.raises(ValueError):
            rc.window_tiles(*bad)


def loop_zoom(w, h, z, cx, cy):
    """The window whose pixel (w // 2, h // 2) is the middle virtual pixel of (cx, cy), moved
    pixel by pixel back inside the zoomed frame."""
    x0, y0 = z * cx + z // 2 - w // 2, z * cy + z // 2 - h // 2
    while x0 < 0:
        x0 += 1
    while x0 + w > z * w:
        x0 -= 1
    while y0 < 0:
        y0 += 1
    while y0 + h > z * h:
        y0 -= 1
    return z * w, z * h, x0, y0


def test_zoom_equals_the_loop():
    lib = rc.hip_lib()
    for w, h in SHAPES:
        for z in (1, 2, 3, 7, 16):
            for cx in sorted({0, w // 2, w - 1}):
                for cy in sorted({0, h // 2, h - 1}):
                    win = rc.window_for_zoom(w, h, z, cx, cy)
                    assert win == loop_zoom(w, h, z, cx, cy), (w, h, z, cx, cy)
                    rw = rc.RcWindow(*win)
                    assert lib.rc_window_check(ctypes.byref(rw), w, h, 8) == 0
    assert rc.window_for_zoom(12, 10, 1, 3, 4) == (12, 10, 0, 0)   # zoom 1: the identity window
    assert rc.window_for_zoom(12, 10, 7, 6, 5) == (84, 70, 39, 33)
    for bad in ((12, 10, 0, 0, 0), (12, 10, 2, 12, 0), (12, 10, 2, 0, -1), (0, 10, 2, 0, 0)):
        with pytest.raises(ValueError):
            rc.window_for_zoom(*bad)


def test_layout_and_exports():
    assert ctypes.sizeof(rc.RcWindow) == 16
    assert [n for n, _ in rc.RcWindow._fields_] == ["full_w", "full_h", "x0", "y0"]
    assert (rc.RcWindow.full_w.offset, rc.RcWindow.full_h.offset, rc.RcWindow.x0.offset,
            rc.RcWindow.y0.offset) == (0, 4, 8, 12)
    lib = rc.hip_lib()
    for name in ("rc_window_check", "rc_window_env", "rc_render_window",
                 "rc_render_window_device", "rc_accum_pass_window_device"):
        assert name in rc.HIP_EXPORTS, name
        assert hasattr(lib, name), name
    assert ctypes.sizeof(rc.RcOptions) == 20   # rc_options keeps its 20 bytes


# rule -> ((full_w, full_h, x0, y0), W, H, s, a word of the message)
BAD = {
    "factor 3": ((97, 61, 0, 0), 8, 8, 3, "factor"),
    "factor 16": ((97, 61, 0, 0), 8, 8, 16, "factor"),
    "factor -1": ((97, 61, 0, 0), 8, 8, -1, "factor"),
    "full_w 0": ((0, 61, 0, 0), 8, 8, 1, "at least 1"),
    "full_h -1": ((97, -1, 0, 0), 8, 8, 1, "at least 1"),
    "W 0": ((97, 61, 0, 0), 0, 8, 1, "at least 1"),
    "H 0": ((97, 61, 0, 0), 8, 0, 1, "at least 1"),
    "x0 negative": ((97, 61, -1, 0), 8, 8, 1, "origin"),
    "y0 negative": ((97, 61, 0, -5), 8, 8, 1, "origin"),
    "x0 + W > full_w": ((97, 61, 90, 0), 8, 8, 1, "outside"),
    "y0 + H > full_h": ((97, 61, 0, 54), 8, 8, 1, "outside"),
    "x0 + W past 2^31": ((INT_MAX, 61, INT_MAX - 1, 0), INT_MAX, 8, 1, "outside"),
    "y0 + H past 2^31": ((97, INT_MAX, 0, INT_MAX), 8, INT_MAX, 1, "outside"),
    "s * full_w past 2^31 - 1": ((INT_MAX // 2 + 1, 61, 0, 0), 8, 8, 2, "2^31 - 1"),
    "s * full_h past 2^31 - 1": ((97, INT_MAX // 8 + 1, 0, 0), 8, 8, 8, "2^31 - 1"),
    "rows of tiles": ((97, 65535 * 16 + 1, 0, 0), 8, 65535 * 16 + 1, 1, "rows of"),
    "rows of tiles at 8": ((97, 65535 * 2 + 1, 0, 0), 8, 65535 * 2 + 1, 8, "rows of"),
}


@pytest.mark.parametrize("rule", sorted(BAD))
def test_check_refuses(rule, capfd):
    win, w, h, s, word = BAD[rule]
    capfd.readouterr()
    assert rc.hip_lib().rc_window_check(ctypes.byref(rc.RcWindow(*win)), w, h, s) == -1
    err = capfd.readouterr().err
    assert "Error: rc_window_check" in err and word in err, err   # the message names the rule
    assert not rc.window_check(win, w, h, s)
    capfd.readouterr()


def test_check_null_and_accepts(capfd):
    lib = rc.hip_lib()
    assert lib.rc_window_check(None, 8, 8, 1) == -1
    assert "rc_window_check" in capfd.readouterr().err
    good = [((97, 61, 0, 0), 97, 61, 1), ((97, 61, 5, 3), 33, 17, 8), ((97, 61, 96, 60), 1, 1, 4),
            ((97, 61, 64, 44), 33, 17, 2), ((8, 8, 0, 0), 8, 8, 0),
            ((1000003, 700001, 999970, 699984), 33, 17, 8),
            ((33554433, 33554431, 33554400, 33554414), 33, 17, 8),
            ((INT_MAX, INT_MAX, INT_MAX - 33, INT_MAX - 17), 33, 17, 1),
            ((INT_MAX // 8, 61, 0, 0), 8, 8, 8), ((97, 65535 * 16, 0, 0), 8, 65535 * 16, 1),
            ((97, 65535 * 2, 0, 0), 8, 65535 * 2, 8)]
    for win, w, h, s in good:
        assert lib.rc_window_check(ctypes.byref(rc.RcWindow(*win)), w, h, s) == 0, (win, w, h, s)
        assert rc.window_check(win, w, h, s)
    assert capfd.readouterr().err == ""


def test_refusals_come_before_any_device_work(capfd):
    """Everything the window entry points refuse is refused from the arguments alone, before the
    first HIP call: the refusals hold on a machine without a GPU, each with a message that says
    why, and the pixmap is untouched."""
    sc = rc.Scene.from_file(scene_path("simple"))
    lib = rc.hip_lib()
    fake = 4096   # a non-null, 8-byte aligned "device pointer" that a refused call never follows
    base = np.random.default_rng(5).integers(0, 256, size=(8, 8, 3), dtype=np.uint8)
    out = base.copy()
    host = out.ctypes.data_as(ctypes.c_void_p)
    seq = rc._rc_sample_seq("rgss4")
    ident = (8, 8, 0, 0)

    def render(word, opt, win=ident, w=8, h=8):
        pw = ctypes.byref(rc.RcWindow(*win)) if win is not None else None
        po = ctypes.byref(opt) if opt is not None else None
        capfd.readouterr()
        assert lib.rc_render_window(sc.packed(), pw, w, h, po, host, None) == -1
        err = capfd.readouterr().err
        assert "Error: rc_" in err and word in err, err
        assert lib.rc_render_window_device(sc.packed(), pw, w, h, po, fake, None, None) == -1
        err = capfd.readouterr().err
        assert "Error: rc_" in err and word in err, err

    def accum(word, opt, win=ident, w=8, h=8, s=seq, first=0, count=1, t=0, reset=0, acc=fake,
              img=fake):
        pw = ctypes.byref(rc.RcWindow(*win)) if win is not None else None
        po = ctypes.byref(opt) if opt is not None else None
        ps = ctypes.byref(s) if s is not None else None
        capfd.readouterr()
        assert lib.rc_accum_pass_window_device(sc.packed(), pw, w, h, po, ps, first, count, t,
                                               reset, acc, img, None, None) == -1
        err = capfd.readouterr().err
        assert "Error: rc_" in err and word in err, err

    def all_three(word, opt, **kw):
        render(word, opt, **kw)
        accum(word, opt, **kw)

    # parity mode, with the family's sentence about the scan-order carry
    all_three("scan-order carry", rc.options(6, "parity"))
    render("scan-order carry", rc.options(6, "parity", ssaa=4))
    for mode in ("fast", "cuda"):
        # a threshold in the options, a factor outside 0, 1, 2, 4, 8
        render("accumulation pass", rc.options(6, mode, ssaa=4, adaptive=16))
        for bad in (dict(ssaa=3), dict(ssaa=16), dict(ssaa=-1), dict(ssaa=1, adaptive=16)):
            all_three("ssaa", rc.options(6, mode, **bad))
        for bad in (dict(ssaa=2), dict(ssaa=8), dict(ssaa=4, adaptive=16)):
            accum("ssaa", rc.options(6, mode, **bad))   # the sequence carries the grid
        all_three("num_gpus", rc.options(6, mode, gpus=2))
        all_three("null pointer", rc.options(6, mode), win=None)
        all_three("null pointer", None)
        # the window's own rules, through every entry (the accumulation entry checks W and H by
        # its family's rules first)
        for rule, (win, w, h, s, word) in BAD.items():
            if s not in (1, 2, 4, 8):
                continue
            render(word, rc.options(6, mode, ssaa=s), win=win, w=w, h=h)
        for win, w, h, word in (((97, 61, -1, 0), 8, 8, "origin"), ((97, 61, 0, -1), 8, 8, "origin"),
                                ((97, 61, 90, 0), 8, 8, "outside"),
                                ((97, 61, 0, 54), 8, 8, "outside"),
                                ((0, 61, 0, 0), 8, 8, "at least 1"),
                                ((INT_MAX // 4 + 1, 61, 0, 0), 8, 8, "2^31 - 1"),
                                ((97, INT_MAX // 4 + 1, 0, 0), 8, 8, "2^31 - 1"),
                                ((97, 61, 0, 0), 0, 8, "2^28"), ((97, 61, 0, 0), 8, -1, "2^28")):
            accum(word, rc.options(6, mode), win=win, w=w, h=h)
        # the accumulation family's own refusals apply as they do there
        accum("null pointer", rc.options(6, mode), s=None)
        accum("null pointer", rc.options(6, mode), acc=None)
        accum("null pointer", rc.options(6, mode), img=None)
        accum("aligned", rc.options(6, mode), acc=fake + 4)
        accum("threshold", rc.options(6, mode), t=256)
        accum("reset", rc.options(6, mode), t=16, reset=1)
        accum("inside the sequence", rc.options(6, mode), first=3, count=2)
        accum("inside the sequence", rc.options(6, mode), count=17)
        accum("32-bit", rc.options(6, mode), win=(1 << 16, 1 << 16, 0, 0), w=1 << 16, h=1 << 16,
              t=16)
    opt = rc.options(6, "fast")
    win = ctypes.byref(rc.RcWindow(*ident))
    assert lib.rc_render_window(None, win, 8, 8, ctypes.byref(opt), host, None) == -1
    assert lib.rc_render_window(sc.packed(), win, 8, 8, ctypes.byref(opt), None, None) == -1
    assert lib.rc_render_window_device(None, win, 8, 8, ctypes.byref(opt), fake, None, None) == -1
    assert lib.rc_render_window_device(sc.packed(), win, 8, 8, ctypes.byref(opt), None, None,
                                       None) == -1
    assert lib.rc_accum_pass_window_device(None, win, 8, 8, ctypes.byref(opt), ctypes.byref(seq),
                                           0, 1, 0, 1, fake, fake, None, None) == -1
    assert capfd.readouterr().err.count("null pointer") == 5
    # the Python wrappers raise
    with pytest.raises(RuntimeError):
        rc.render_window(sc, ident, 8, 8, mode="parity", out=out)
    with pytest.raises(RuntimeError):
        rc.render_window(sc, (8, 8, 1, 0), 8, 8, out=out)
    with pytest.raises(RuntimeError):
        rc.render_window_device(sc, ident, 8, 8, fake, ssaa=3)
    with pytest.raises(RuntimeError):
        rc.accum_pass_window_device(sc, (8, 8, 0, 1), 8, 8, "rgss4", 0, 1, fake, fake)
    np.testing.assert_array_equal(out, base)
    capfd.readouterr()


ENV = ("RAYCAST_WINDOW", "RAYCAST_PATTERN", "RAYCAST_FILTER")


@pytest.fixture
def clean_env():
    saved = {k: os.environ.pop(k, None) for k in ENV}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def test_env(clean_env, capfd):
    # unset: nothing, and no message
    assert rc.window_from_env(33, 17) is None
    assert capfd.readouterr().err == ""
    os.environ["RAYCAST_WINDOW"] = "97x61+5+3"
    for mode in ("fast", "cuda"):
        for s in FACTORS:
            assert rc.window_from_env(33, 17, mode, s) == (97, 61, 5, 3)
    os.environ["RAYCAST_WINDOW"] = "33554433x33554431+33554400+0"
    assert rc.window_from_env(33, 17, "fast", 8) == (33554433, 33554431, 33554400, 0)
    os.environ["RAYCAST_WINDOW"] = "33x17+0+0"
    assert rc.window_from_env(33, 17) == (33, 17, 0, 0)
    assert capfd.readouterr().err == ""
    # null arguments
    lib = rc.hip_lib()
    opt = rc.options(6, "fast")
    assert lib.rc_window_env(None, 33, 17, ctypes.byref(rc.RcWindow())) == 0
    assert lib.rc_window_env(ctypes.byref(opt), 33, 17, None) == 0
    # each malformed form: a warning, ignored
    for bad in ("", "97x61", "97x61+5", "97x61+5+", "97x61+5+3+1", "97x61+5+3 ", " 97x61+5+3",
                "x61+5+3", "97x+5+3", "97X61+5+3", "97x61-5+3", "97x61+-5+3", "-97x61+5+3",
                "97.0x61+5+3", "97x61,5,3", "97x61+5+3junk", "0x61x61+5+3", "99999999999x61+5+3",
                "97x61+4294967301+3", "window"):
        os.environ["RAYCAST_WINDOW"] = bad
        assert rc.window_from_env(33, 17) is None, bad
        err = capfd.readouterr().err
        assert "Warning: RAYCAST_WINDOW" in err and "FWxFH+X0+Y0" in err, (bad, err)
    # each combination that is ignored with a warning
    os.environ["RAYCAST_WINDOW"] = "97x61+5+3"
    assert rc.window_from_env(33, 17, "parity") is None
    assert "scan-order carry" in capfd.readouterr().err
    assert rc.window_from_env(33, 17, "fast", 4, adaptive=16) is None
    assert "RAYCAST_SSAA_ADAPTIVE" in capfd.readouterr().err
    assert rc.window_from_env(33, 17, "fast", gpus=2) is None
    assert "RAYCAST_GPUS" in capfd.readouterr().err
    os.environ["RAYCAST_PATTERN"] = "rgss4"
    assert rc.window_from_env(33, 17) is None
    assert "RAYCAST_PATTERN" in capfd.readouterr().err
    del os.environ["RAYCAST_PATTERN"]
    os.environ["RAYCAST_FILTER"] = "tent"
    assert rc.window_from_env(33, 17, "fast", 2) is None
    assert "RAYCAST_FILTER" in capfd.readouterr().err
    os.environ["RAYCAST_FILTER"] = "box"
    assert rc.window_from_env(33, 17, "fast", 2) == (97, 61, 5, 3)
    del os.environ["RAYCAST_FILTER"]
    assert capfd.readouterr().err == ""
    # a window that fails rc_window_check: its message, then the warning
    for bad, w, h in (("97x61+65+3", 33, 17), ("97x61+5+45", 33, 17), ("0x61+0+0", 33, 17),
                      ("97x61+5+3", 0, 17), ("2147483647x61+0+0", 33, 17)):
        os.environ["RAYCAST_WINDOW"] = bad
        s = 2 if bad.startswith("2147483647") else 1
        assert rc.window_from_env(w, h, "fast", s) is None, bad
        err = capfd.readouterr().err
        assert "Error: rc_window_check" in err and "Warning: RAYCAST_WINDOW" in err, (bad, err)


def test_the_two_checkers_agree():
    """The reference held to its own bound: the crop the GPU tests take from rco_pixels at
    full = (97, 61) is the crop of oracle_render's 97 x 61 image, pixels and zero-normalize
    events."""
    sc = rc.Scene.from_file(scene_path("quadric"))
    fw, fh = 97, 61
    full, stats = oracle_render(sc, fw, fh, 6, "fast")
    for (x0, y0), (w, h) in (((0, 0), (97, 61)), ((5, 3), (33, 17)), ((64, 44), (33, 17))):
        ys, xs = np.mgrid[y0:y0 + h, x0:x0 + w]
        rgb, z = oracle_pixels(sc, fw, fh, 6, "fast", (ys * fw + xs).ravel())
        np.testing.assert_array_equal(rgb.reshape(h, w, 3),
                                      rc.window_crop(full, 1, (fw, fh, x0, y0), w, h))
        if (w, h) == (fw, fh):
            assert int(z.sum()) == stats["zero_normalize"]
    crop = rc.window_crop(full, 1, (fw, fh, 5, 3), 33, 17)
    assert len(np.unique(crop.reshape(-1, 3), axis=0)) > 1   # not a flat patch
