"""Variable-rate supersampling from a per-pixel rate map on the GPU (rc_render_rates,
rc_render_rates_device): every output byte is rc.rates_compose over images of the CPU oracle, its
W x H image F_1 and the box filters F_s of its s*W x s*H images, and the caller's own bytes where
the rate is 0: no tolerance anywhere.  The caller's buffer is always pre-filled with seeded random
bytes, so "not stored to" is visible and a black pixel cannot hide in it."""
import ctypes

import numpy as np
import pytest

from helpers import oracle_render, oracle_render_cuda, rc, scene_path

pytestmark = pytest.mark.gpu

SCENES = ["simple", "reflection", "quadric"]
SIZES = [(1, 1), (7, 3), (33, 17), (64, 48)]   # one pixel; partial tiles; a partly filled wave
ALL = rc.RATE_VALUES


@pytest.fixture(scope="module")
def scenes():
    return {n: rc.Scene.from_file(scene_path(n)) for n in SCENES}


_oracle = {}


def oracle_image(sc, name, w, h, s, depth, mode):
    """(F_s, zero-normalize events of the s*W x s*H image; None in cuda mode, whose oracle keeps
    none) from the CPU oracle: computed once per key, read-only."""
    key = (name, w, h, s, depth, mode)
    if key not in _oracle:
        if mode == "cuda":
            img, zn = oracle_render_cuda(sc, s * w, s * h, depth), None
        else:
            img, stats = oracle_render(sc, s * w, s * h, depth, mode)
            assert stats["parity_defined"] == 1, key   # the example scenes are all defined
            zn = stats["zero_normalize"]
        if s > 1:
            img = rc.box_downsample(img, s)
        img.setflags(write=False)
        _oracle[key] = (img, zn)
    return _oracle[key]


def oracle_images(scenes, name, w, h, rates, depth, mode):
    """{s: F_s} for the non-zero rates that occur in the map."""
    return {s: oracle_image(scenes[name], name, w, h, s, depth, mode)[0]
            for s in np.unique(rates).tolist() if s in ALL and s != 0}


def random_base(w, h):
    return np.random.default_rng(77000 + w * 10 + h).integers(0, 256, size=(h, w, 3),
                                                               dtype=np.uint8)


def random_map(w, h, values=ALL):
    return np.random.default_rng(9000 + w * 10 + h).choice(np.array(values, dtype=np.uint8),
                                                           size=(h, w))


def check_stats(rates, tag):
    st = rc.rate_stats()
    counts = {s: int((rates == s).sum()) for s in (1, 2, 4, 8)}
    assert st["pixels"] == counts, tag
    assert st["invalid"] == 0, tag
    assert st["rays"] == counts[1] + 4 * counts[2] + 16 * counts[4] + 64 * counts[8], tag
    return st


def check(scenes, name, w, h, rates, depth=6, mode="fast", timing=None, tag=""):
    """render_rates over a random base against rates_compose of the oracle's images; the
    statistics against the map's own counts.  Returns (expected, images)."""
    base = random_base(w, h)
    images = oracle_images(scenes, name, w, h, rates, depth, mode)
    want = rc.rates_compose(base, images, rates)
    out = base.copy()
    got = rc.render_rates(scenes[name], w, h, rates, depth=depth, mode=mode, out=out,
                          timing=timing)
    assert got is out
    tag = f"{name} {w}x{h} {mode} d{depth} {tag}"
    np.testing.assert_array_equal(out, want, err_msg=tag)
    check_stats(rates, tag)
    return want, images


@pytest.mark.parametrize("scene", SCENES)
def test_random_maps_vs_oracle(scene, scenes):
    for w, h in SIZES:
        rates = random_map(w, h)
        if (w, h) in ((33, 17), (64, 48)):
            assert set(np.unique(rates).tolist()) == set(ALL)
        if (w, h) == (64, 48):
            # a partly filled last wave step of the rate-2 (16 pixels a step) and the rate-4
            # list (4 a step): a condition on the input
            assert int((rates == 2).sum()) % 16 != 0 and int((rates == 4).sum()) % 4 != 0
        check(scenes, scene, w, h, rates, tag="random")


@pytest.mark.parametrize("scene", SCENES)
def test_uniform_maps_vs_oracle(scene, scenes):
    for w, h in SIZES:
        base = random_base(w, h)
        out = base.copy()
        rc.render_rates(scenes[scene], w, h, np.zeros((h, w), dtype=np.uint8), out=out)
        np.testing.assert_array_equal(out, base, err_msg=f"{scene} {w}x{h} all 0")
        check_stats(np.zeros((h, w), dtype=np.uint8), "all 0")
        for s in (1, 2, 4, 8):
            tim = {}
            want, images = check(scenes, scene, w, h, np.full((h, w), s, dtype=np.uint8),
                                 timing=tim, tag=f"all {s}")
            np.testing.assert_array_equal(want, images[s])   # the plain / the ssaa = s image
            zn = oracle_image(scenes[scene], scene, w, h, s, 6, "fast")[1]
            assert tim["zero_normalize"] == zn, (scene, w, h, s)


@pytest.mark.parametrize("scene", SCENES)
def test_checkerboards_vs_oracle(scene, scenes):
    """By pixel: a store wider than a pixel, or a whole-row store, writes into a rate-0
    neighbour."""
    w, h = 33, 17
    yy, xx = np.mgrid[0:h, 0:w]
    for s in (1, 2):
        for phase in (0, 1):
            rates = np.where((xx + yy) % 2 == phase, s, 0).astype(np.uint8)
            check(scenes, scene, w, h, rates, tag=f"checker {s}/{phase}")


@pytest.mark.parametrize("scene", SCENES)
def test_region_of_interest_vs_oracle(scene, scenes):
    w, h = 64, 48
    rates = np.zeros((h, w), dtype=np.uint8)
    rates[7:17, 13:33] = 4   # 20 x 10 at an odd origin
    assert int((rates == 4).sum()) == 200
    check(scenes, scene, w, h, rates, tag="roi")


def fovea_map(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    d2 = (xx - w // 2) ** 2 + (yy - h // 2) ** 2
    rates = np.ones((h, w), dtype=np.uint8)
    rates[d2 < (h // 2) ** 2] = 2
    rates[d2 < (h // 4) ** 2] = 4
    rates[d2 < (h // 8) ** 2] = 8
    return rates


@pytest.mark.parametrize("scene", SCENES)
def test_fovea_vs_oracle(scene, scenes):
    w, h = 64, 48
    rates = fovea_map(w, h)
    assert set(np.unique(rates).tolist()) == {1, 2, 4, 8}
    want, images = check(scenes, scene, w, h, rates, tag="fovea")
    for s in (1, 2, 4, 8):   # a build that returns any single image fails
        assert (want != images[s]).any(), (scene, s)


@pytest.mark.parametrize("scene", SCENES)
def test_cuda_vs_oracle(scene, scenes):
    for w, h in ((7, 3), (64, 48)):
        rates = random_map(w, h, values=(0, 1, 2, 4))
        if (w, h) == (64, 48):
            assert set(np.unique(rates).tolist()) == {0, 1, 2, 4}
        check(scenes, scene, w, h, rates, depth=50, mode="cuda", tag="random")


def device_render(torch, sc, w, h, rates, base, stream=None, **kw):
    """render_rates_device over device copies of the map and the base; the image back on the
    host."""
    d_rates = torch.from_numpy(np.ascontiguousarray(rates)).cuda()
    d_out = torch.from_numpy(base.copy()).cuda()
    torch.cuda.synchronize()
    rc.render_rates_device(sc, w, h, d_rates.data_ptr(), d_out.data_ptr(), stream, **kw)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def test_invalid_bytes(scenes):
    torch = pytest.importorskip("torch")
    w, h = 33, 17
    rates = random_map(w, h)
    bad = rates.copy()
    spots = [((2, 5), 3), ((16, 32), 5), ((0, 0), 16), ((9, 20), 255), ((9, 21), 7)]
    for (y, x), v in spots:
        bad[y, x] = v
    cleaned = bad.copy()
    for (y, x), _ in spots:
        cleaned[y, x] = 0   # an invalid byte is treated as rate 0
    base = random_base(w, h)
    images = oracle_images(scenes, "quadric", w, h, cleaned, 6, "fast")
    got = device_render(torch, scenes["quadric"], w, h, bad, base)
    np.testing.assert_array_equal(got, rc.rates_compose(base, images, cleaned))
    st = rc.rate_stats()
    assert st["invalid"] == len(spots)
    assert st["pixels"] == {s: int((cleaned == s).sum()) for s in (1, 2, 4, 8)}
    # the host-map call checks the map before anything is enqueued
    out = base.copy()
    with pytest.raises(RuntimeError):
        rc.render_rates(scenes["quadric"], w, h, bad, out=out)
    np.testing.assert_array_equal(out, base)
    # and the device is as usable as before
    check(scenes, "quadric", w, h, rates, tag="after invalid")


@pytest.mark.parametrize("mode,depth", [("fast", 6), ("cuda", 50)])
def test_larger_image_on_the_gpu_alone(mode, depth, scenes):
    """Many tiles and lists longer than a small grid, against rates_compose of the GPU's own
    ssaa = s images; the lists' order differs from run to run, the bytes do not."""
    sc, w, h = scenes["quadric"], 257, 129
    rates = random_map(w, h)
    assert set(np.unique(rates).tolist()) == set(ALL)
    images = {s: rc.render(sc, w, h, depth=depth, mode=mode, ssaa=s) for s in (1, 2, 4, 8)}
    base = random_base(w, h)
    want = rc.rates_compose(base, images, rates)
    one = rc.render_rates(sc, w, h, rates, depth=depth, mode=mode, out=base.copy())
    np.testing.assert_array_equal(one, want)
    check_stats(rates, mode)
    two = rc.render_rates(sc, w, h, rates, depth=depth, mode=mode, out=base.copy())
    np.testing.assert_array_equal(two, one)
    for blocks in (1, 2):   # the stride loops walk lists longer than the grid
        with rc.tuned(adaptive_blocks=blocks):
            got = rc.render_rates(sc, w, h, rates, depth=depth, mode=mode, out=base.copy())
            check_stats(rates, f"{mode} blocks {blocks}")
        np.testing.assert_array_equal(got, want, err_msg=f"{mode} blocks {blocks}")


@pytest.mark.parametrize("mode,depth", [("fast", 6), ("cuda", 50)])
def test_against_adaptive(mode, depth, scenes):
    """Adaptive supersampling is the rate map its own edge test makes."""
    sc, w, h = scenes["reflection"], 64, 48
    a = rc.render(sc, w, h, depth=depth, mode=mode)
    for s, t in ((2, 16), (4, 1)):
        m = np.where(rc.edge_mask(a, t), s, 0).astype(np.uint8)
        assert 0 < int((m == s).sum()) < w * h
        want = rc.render(sc, w, h, depth=depth, mode=mode, ssaa=s, adaptive=t)
        refined = rc.adaptive_stats()["refined_pixels"]
        got = rc.render_rates(sc, w, h, m, depth=depth, mode=mode, out=a.copy())
        np.testing.assert_array_equal(got, want, err_msg=f"{mode} s{s} t{t}")
        assert rc.rate_stats()["pixels"][s] == refined


def test_stream_order_and_phase_spans(scenes):
    """The map is written by a torch operation on the caller's stream immediately before the
    call, with no synchronisation in between and one afterwards."""
    torch = pytest.importorskip("torch")
    sc, w, h = scenes["quadric"], 64, 48
    rates = fovea_map(w, h)
    rates[0:5, :] = 0
    base = random_base(w, h)
    images = oracle_images(scenes, "quadric", w, h, rates, 6, "fast")
    want = rc.rates_compose(base, images, rates)
    src = torch.from_numpy(rates).cuda()
    d_rates = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    d_out = torch.from_numpy(base.copy()).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_rates.copy_(src)
        rc.render_rates_device(sc, w, h, d_rates.data_ptr(), d_out.data_ptr(),
                               stream.cuda_stream)
    stream.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy(), want)
    check_stats(rates, "stream")
    # timed: synchronous, and the two spans make up the kernel time
    d_out.copy_(torch.from_numpy(base))
    torch.cuda.synchronize()
    tim = {}
    rc.render_rates_device(sc, w, h, d_rates.data_ptr(), d_out.data_ptr(), stream.cuda_stream,
                           timing=tim)
    np.testing.assert_array_equal(d_out.cpu().numpy(), want)
    ms = rc.rate_phase_ms()
    assert ms["render"] > 0.0 and ms["refine"] > 0.0
    assert ms["render"] + ms["refine"] == pytest.approx(tim["kernel_ms"], rel=1e-3)


def raw_render_rates(sc, w, h, opt, rates, out):
    """rc_render_rates with options the Python call does not offer; raises like it."""
    r = rc.hip_lib().rc_render_rates(sc.packed(), w, h, ctypes.byref(opt),
                                     rates.ctypes.data_as(ctypes.c_void_p),
                                     out.ctypes.data_as(ctypes.c_void_p), None)
    if r != 0:
        raise RuntimeError("rc_render_rates failed")


def test_refusals(scenes):
    torch = pytest.importorskip("torch")
    sc, w, h = scenes["simple"], 8, 8
    rates = random_map(w, h)
    base = random_base(w, h)
    out = base.copy()
    d_rates = torch.from_numpy(rates).cuda()
    d_out = torch.from_numpy(base.copy()).cuda()
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):   # parity mode
        rc.render_rates(sc, w, h, rates, mode="parity", out=out)
    with pytest.raises(RuntimeError):
        rc.render_rates_device(sc, w, h, d_rates.data_ptr(), d_out.data_ptr(), mode="parity")
    for bad in (dict(ssaa=2), dict(ssaa=2, adaptive=16), dict(ssaa=1, adaptive=16),
                dict(ssaa=3), dict(gpus=2)):
        with pytest.raises(RuntimeError):   # the map carries the factor; one GPU
            raw_render_rates(sc, w, h, rc.options(6, "fast", **bad), rates, out)
    with rc.tuned(share_device=1):   # two ranks on this device: still refused
        with pytest.raises(RuntimeError):
            raw_render_rates(sc, w, h, rc.options(6, "fast", gpus=2), rates, out)
    with pytest.raises(RuntimeError):   # null pointers
        rc.render_rates_device(sc, w, h, 0, d_out.data_ptr())
    with pytest.raises(RuntimeError):
        rc.render_rates_device(sc, w, h, d_rates.data_ptr(), 0)
    # sizes the 32-bit pixel indices or the tile grid cannot address: W*H = 2^32, 8*W past
    # INT_MAX, more than 65535 rows of tiles (refused from the sizes alone, before any launch)
    for bw, bh in ((1 << 16, 1 << 16), (1 << 28, 1), (1, 1 << 28), (1, 16 * 65535 + 1)):
        with pytest.raises(RuntimeError):
            rc.render_rates_device(sc, bw, bh, d_rates.data_ptr(), d_out.data_ptr())
    # nothing was written
    np.testing.assert_array_equal(out, base)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy(), base)
    # a refusal leaves the device usable
    check(scenes, "simple", w, h, rates, tag="after refusals")
