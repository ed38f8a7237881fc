"""The primary-visibility G-buffer on the GPU (rc_render_gbuffer*, rc_pick*, rc_id_edge_rates_device;
DESIGN.md §22): every plane is the CPU oracle's own scan of the same primary ray, bit for bit (floats
are compared as uint32), for windows of virtual images of 97 x 61 and of 33 554 433 x 33 554 431
pixels; the geometric-edge recipe is the rate-map contract of the oracle's images.  No tolerance
anywhere.  The expectation is built here from the ray-level suite's helpers: the direction in
numpy's IEEE arithmetic (shade_cases.primary_dir_ref; the CUDA port's float sum as
shade_cases.camera_dirs_cuda forms it) and the oracle's rco_prim_nearest / rco_prim_nearest_cuda
(prim_cases.ref_nearest)."""
import ctypes
import itertools

import numpy as np
import pytest

import prim_cases as pc
import shade_cases as shc
from helpers import oracle_render, oracle_render_cuda, rc, scene_path

pytestmark = pytest.mark.gpu

F32, F64, I32, U32 = np.float32, np.float64, np.int32, np.uint32
FULL = (97, 61)
HUGE = (33554433, 33554431)
SIZES = [(1, 1), (7, 3), (33, 17), (64, 48), FULL]
SCENES = pc.GOLDEN_SCENES + ["random14x", "random65"]
MODES = ["fast", "parity", "cuda"]
ALL4 = ("id", "t", "P", "N")
SUBSETS = [("id",), ("t",), ("id", "t"), ("P",), ("N",), ALL4]
SENTINEL = 0x5a5a5a5a
TAIL = 64            # elements behind every plane that must come back untouched
DEPTH = 6


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def origins(w, h, full=FULL):
    """(0, 0); (5, 3), odd: no multiple of the 8 x 8 wave block; flush right and bottom."""
    return sorted({(0, 0), (min(5, full[0] - w), min(3, full[1] - h)), (full[0] - w, full[1] - h)})


# ------------------------------------------------------------------- the reference --
def primary_dirs(js, full, xy, cuda):
    """The primary rays of the virtual pixels xy [n, 2] of the full_w x full_h image, as the
    launchers form the camera (make_cam): the C port's normalize (a double sum) or, cuda, the CUDA
    port's (a float sum)."""
    cw, ch = F32(js.camera_width), F32(js.camera_height)
    n = len(xy)
    cam = np.tile([0.0 - F64(cw) / 2.0, 0.0 + F64(ch) / 2.0], (n, 1))
    pix = np.zeros((n, 4), F32)
    pix[:, 0], pix[:, 1] = cw / F32(full[0]), ch / F32(full[1])
    if not cuda:
        d, zero = shc.primary_dir_ref(cam, pix, xy)
        assert not zero.any()
        return d
    dx = (cam[:, 0] + pix[:, 0].astype(F64) * (xy[:, 0].astype(F64) + 0.5)).astype(F32)
    dy = (cam[:, 1] - pix[:, 1].astype(F64) * (xy[:, 1].astype(F64) + 0.5)).astype(F32)
    dz = np.full(n, -1.0, F32)
    s = dx * dx
    s = s + dy * dy
    s = s + dz * dz
    ln = np.sqrt(s.astype(F64)).astype(F32)
    return np.stack([dx / ln, dy / ln, dz / ln], 1).astype(F32)


def ref_points(name, cuda, full, xy):
    """The oracle's records of the virtual pixels xy: a dict of id [n], t [n], P, N [n, 3] (the C
    port) and the zero-normalize events; a miss is id -1 and +0 everywhere (the export's own)."""
    js = pc.list_scenes()[name].js
    xy = np.ascontiguousarray(xy, I32).reshape(-1, 2)
    D = np.ascontiguousarray(primary_dirs(js, full, xy, cuda))
    O, skip = np.zeros_like(D), np.full(len(D), -1, I32)
    if cuda:
        idx, t = pc.ref_nearest(js, O, D, skip, cuda=True)
        return {"id": idx, "t": t, "zero": 0}
    idx, t, P, N, z = pc.ref_nearest(js, O, D, skip)
    return {"id": idx, "t": t, "P": P, "N": N, "zero": int(z.sum())}


_REF = {}


def ref_planes(name, cuda, window, w, h):
    """ref_points over the w x h window at window = (full_w, full_h, x0, y0), as planes [h, w] and
    [h, w, 3]; computed once per key, read-only."""
    key = (name, cuda, tuple(window), w, h)
    if key not in _REF:
        fw, fh, x0, y0 = window
        ys, xs = np.mgrid[y0:y0 + h, x0:x0 + w]
        r = ref_points(name, cuda, (fw, fh), np.stack([xs.ravel(), ys.ravel()], 1))
        out = {"zero": r.pop("zero")}
        for k, a in r.items():
            out[k] = a.reshape((h, w) + a.shape[1:])
            out[k].setflags(write=False)
        miss = out["id"] < 0
        assert np.all(out["id"][miss] == -1) and not out["t"][miss].view(U32).any()
        _REF[key] = out
    return _REF[key]


def crop(planes, x0, y0, w, h):
    return {k: (a[y0:y0 + h, x0:x0 + w] if k != "zero" else a) for k, a in planes.items()}


def bits(a):
    return np.ascontiguousarray(a).view(U32)


# ----------------------------------------------------------------------- the device --
def gpu_planes(torch, scene, mode, window, w, h, names, stream=None, timing=None):
    """The planes `names` of the window through rc_render_gbuffer_device into buffers that are TAIL
    elements longer than the plane and pre-filled: the tails must come back untouched."""
    comps = {p: rc.GBUFFER_PLANES[p][1] for p in names}
    bufs = {p: torch.full((w * h * c + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
            for p, c in comps.items()}
    torch.cuda.synchronize()
    ptr = {"d_" + p.lower() + "_ptr": b.data_ptr() for p, b in bufs.items()}
    rc.render_gbuffer_device(scene, w, h, window=window, mode=mode, timing=timing,
                             stream_ptr=stream.cuda_stream if stream else None, **ptr)
    torch.cuda.synchronize()
    out = {}
    for p, b in bufs.items():
        a = b.cpu().numpy()
        assert np.all(a[-TAIL:] == SENTINEL), f"{p}: the kernel stored behind its plane"
        a = a[:-TAIL].reshape((h, w) + ((3,) if comps[p] == 3 else ()))
        out[p] = a if p == "id" else a.view(F32)
    return out


def assert_planes(got, want, names, tag):
    for p in names:
        assert got[p].shape == want[p].shape, (tag, p)
        bad = np.argwhere(bits(got[p]) != bits(want[p]))
        assert len(bad) == 0, (f"{tag} plane {p}: {len(bad)} words differ, first at {bad[0]}: "
                               f"{got[p][tuple(bad[0])]!r} != {want[p][tuple(bad[0])]!r}")


# ------------------------------------------------ 1. planes against the oracle --
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SCENES)
def test_planes_bit_for_bit(name, mode, torch):
    scene = pc.list_scenes()[name]
    cuda = mode == "cuda"
    names = ("id", "t") if cuda else ALL4
    full = ref_planes(name, cuda, (*FULL, 0, 0), *FULL)
    assert 0 < np.count_nonzero(full["id"] >= 0), name          # the image is not empty
    for w, h in SIZES:
        for x0, y0 in origins(w, h):
            got = gpu_planes(torch, scene, mode, (*FULL, x0, y0), w, h, names)
            assert_planes(got, crop(full, x0, y0, w, h), names, f"{name} {mode} {w}x{h}+{x0}+{y0}")
    # every subset of the planes, on the odd window
    w, h, x0, y0 = 33, 17, 5, 3
    want = crop(full, x0, y0, w, h)
    for sub in SUBSETS:
        if cuda and ("P" in sub or "N" in sub):
            continue
        assert_planes(gpu_planes(torch, scene, mode, (*FULL, x0, y0), w, h, sub), want, sub,
                      f"{name} {mode} subset {sub}")
    # win = NULL is the identity window
    assert_planes(gpu_planes(torch, scene, mode, None, *FULL, names), full, names,
                  f"{name} {mode} win=NULL")


def test_the_two_arithmetics_differ():
    """The references are two contracts: with each port's own primary ray the CUDA port's t differs
    in bits from the C port's on 589 .. 4197 of the 5917 pixels of every scene (its direction is
    normalised with a float sum), and the ids agree everywhere.  The generalised direction used
    here is shade_cases.camera_dirs_cuda's on that helper's own 64 x 48 image."""
    for name in SCENES:
        c = ref_planes(name, False, (*FULL, 0, 0), *FULL)
        u = ref_planes(name, True, (*FULL, 0, 0), *FULL)
        np.testing.assert_array_equal(c["id"], u["id"], err_msg=name)
        assert np.count_nonzero(bits(c["t"]) != bits(u["t"])) >= 100, name
    js = pc.list_scenes()["quadric"].js
    ys, xs = np.mgrid[0:48, 0:64]
    xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(I32)
    assert primary_dirs(js, (64, 48), xy, True).tobytes() == shc.camera_dirs_cuda(js).tobytes()
    assert primary_dirs(js, (64, 48), xy, False).tobytes() == shc.camera_dirs(js).tobytes()


def test_host_entry_and_parity_bytes():
    """rc_render_gbuffer (host planes): the oracle's bits in the three modes, parity's bytes being
    fast's; the timing record of a parity call has nothing parity-specific in it."""
    w, h, win = 33, 17, (*FULL, 5, 3)
    for name in ("quadric", "random65"):
        scene = pc.list_scenes()[name]
        want = crop(ref_planes(name, False, (*FULL, 0, 0), *FULL), 5, 3, w, h)
        out = {}
        for mode in ("fast", "parity"):
            tim = {}
            out[mode] = rc.render_gbuffer(scene, w, h, planes=ALL4, window=win, mode=mode,
                                          timing=tim)
            assert_planes(out[mode], want, ALL4, f"{name} {mode} host")
            assert tim["kernel_ms"] > 0.0 and tim["total_ms"] >= tim["d2h_ms"] >= 0.0
            assert tim["resolve_ms"] == 0.0 and tim["dep_pixels"] == 0
            assert tim["zero_normalize"] == want["zero"]
        for p in ALL4:
            assert out["fast"][p].tobytes() == out["parity"][p].tobytes(), (name, p)
        got = rc.render_gbuffer(scene, w, h, window=win, mode="cuda")
        assert sorted(got) == ["id", "t"]
        assert_planes(got, crop(ref_planes(name, True, (*FULL, 0, 0), *FULL), 5, 3, w, h),
                      ("id", "t"), f"{name} cuda host")


# -------------------------------------------- 2. a virtual image nobody could render --
# 64 x 48 windows of the 33 554 433 x 33 554 431 image of quadric.scene.  The origins were chosen on
# the CPU on the oracle's planes.  A window is 64 pixels of 33 million wide, so t moves by a few ulps
# across it unless the surface is seen at a grazing angle: the origins lie on silhouettes, found by
# bisecting a row of the huge image between two pixels of the 97 x 61 image with different ids.
# Distinct bit patterns of t (C port / CUDA port) and ids per window:
#   (6087648, 5775741)    81 / 77   {-1, 1}      the cylinder's left edge against the background
#   (23767685, 16777194)  187 / 215 {-1, 2, 4}   the sphere's edge, the floor's horizon behind it
#   (13485665, 18977485)  84 / 112  {1}          both odd, just inside the cylinder's right edge
#   (29360069, 16777194)  63 / 38   {-1, 2, 4}   the sphere's right edge
# The conditions are re-checked below on the oracle's planes.
HUGE_SCENE = "quadric"
HUGE_ORIGINS = [(6087648, 5775741), (23767685, 16777194), (13485665, 18977485),
                (29360069, 16777194)]


def _check_huge_inputs(cuda):
    mixed = False
    for x0, y0 in HUGE_ORIGINS:
        r = ref_planes(HUGE_SCENE, cuda, (*HUGE, x0, y0), 64, 48)
        assert len(np.unique(bits(r["t"]))) >= 32, (x0, y0)
        hits = np.count_nonzero(r["id"] >= 0)
        mixed = mixed or 0 < hits < 64 * 48
    assert mixed


@pytest.mark.parametrize("mode", ["fast", "cuda"])
def test_huge_virtual_image(mode, torch):
    cuda = mode == "cuda"
    names = ("id", "t") if cuda else ALL4
    _check_huge_inputs(cuda)
    scene = pc.list_scenes()[HUGE_SCENE]
    for x0, y0 in HUGE_ORIGINS:
        win = (*HUGE, x0, y0)
        assert_planes(gpu_planes(torch, scene, mode, win, 64, 48, names),
                      ref_planes(HUGE_SCENE, cuda, win, 64, 48), names, f"{mode} huge +{x0}+{y0}")
    # a 7x zoom of the 97 x 61 frame, odd origin
    win = (7 * FULL[0], 7 * FULL[1], 301, 187)
    want = ref_planes(HUGE_SCENE, cuda, win, 64, 48)
    assert 0 < np.count_nonzero(want["id"] >= 0) and len(np.unique(want["id"])) >= 2
    assert_planes(gpu_planes(torch, scene, mode, win, 64, 48, names), want, names, f"{mode} zoom")


# --------------------------------------------------- 3. consistency with the renderer --
@pytest.mark.parametrize("name", SCENES)
def test_misses_are_black_and_hit_share(name, torch):
    scene = pc.list_scenes()[name]
    w, h = FULL
    got = gpu_planes(torch, scene, "fast", (*FULL, 0, 0), w, h, ("id",))["id"]
    d_img = torch.full((h, w, 3), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc.render_window_device(scene, (*FULL, 0, 0), w, h, d_img.data_ptr(), depth=DEPTH, mode="fast")
    torch.cuda.synchronize()
    img = d_img.cpu().numpy()
    assert not img[got == -1].any()
    want = ref_planes(name, False, (*FULL, 0, 0), w, h)["id"]
    assert np.count_nonzero(got >= 0) == np.count_nonzero(want >= 0)
    assert got.min() >= -1 and got.max() < scene.num_shapes


# ------------------------------------------------------------------------- 4. pick --
PICK_NS = [1, 63, 64, 65, 1000]


def pick_points(n):
    """n points of the 97 x 61 image: the four corners first, duplicates of them and of random
    points among the rest."""
    rng = np.random.default_rng(4400 + n)
    corners = [(0, 0), (FULL[0] - 1, 0), (0, FULL[1] - 1), (FULL[0] - 1, FULL[1] - 1)]
    pts = np.stack([rng.integers(0, FULL[0], n), rng.integers(0, FULL[1], n)], 1)
    pts[:min(n, 4)] = corners[:min(n, 4)]
    if n >= 63:
        pts[10:14] = corners                   # duplicates of the corners
        pts[20:30] = pts[40:50]                # and of ten other points
    return pts.astype(I32)


def hit_records(full, pts, frame):
    """The records rc_pick* must give for pts, read off the window planes `full`."""
    x, y = pts[:, 0], pts[:, 1]
    rec = np.zeros(len(pts), rc.HIT_DTYPE)
    rec["id"], rec["t"] = full["id"][y, x], full["t"][y, x]
    if frame:
        rec["P"], rec["N"] = full["P"][y, x], full["N"][y, x]
    return rec


@pytest.mark.parametrize("mode,frame", [("fast", 0), ("fast", 1), ("parity", 1), ("cuda", 0)])
def test_pick_equals_the_planes(mode, frame, torch):
    name = "quadric"
    scene = pc.list_scenes()[name]
    full = ref_planes(name, mode == "cuda", (*FULL, 0, 0), *FULL)
    for n in PICK_NS:
        pts = pick_points(n)
        want = hit_records(full, pts, frame)
        got = rc.pick(scene, *FULL, pts, frame=bool(frame), mode=mode)
        assert got.tobytes() == want.tobytes(), f"{mode} frame {frame} n {n} (host)"
        # the device entry, records with a tail
        d_xy = torch.from_numpy(pts).cuda()
        d_hits = torch.full(((n + 2) * 8,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc.pick_device(scene, *FULL, n, d_xy.data_ptr(), d_hits.data_ptr(), frame=bool(frame),
                       mode=mode)
        torch.cuda.synchronize()
        raw = d_hits.cpu().numpy()
        assert np.all(raw[-16:] == SENTINEL)
        assert raw[:-16].tobytes() == want.tobytes(), f"{mode} frame {frame} n {n} (device)"


def test_pick_points_outside(torch):
    name, n = "quadric", 65
    scene = pc.list_scenes()[name]
    full = ref_planes(name, False, (*FULL, 0, 0), *FULL)
    pts = pick_points(n)
    outside = {0: (-1, 5), 31: (FULL[0], 7), 64: (3, FULL[1])}        # first, mid-wave, last
    for k, p in outside.items():
        pts[k] = p
    inside = np.array([k not in outside for k in range(n)])
    want = np.zeros(n, rc.HIT_DTYPE)
    want[inside] = hit_records(full, pts[inside], 1)
    want["id"][~inside] = -2
    d_xy = torch.from_numpy(pts).cuda()
    d_hits = torch.full((n * 8,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc.pick_device(scene, *FULL, n, d_xy.data_ptr(), d_hits.data_ptr(), frame=True)
    torch.cuda.synchronize()
    assert d_hits.cpu().numpy().tobytes() == want.tobytes()
    # the host entry sees the points: -1, hits untouched
    hits = np.full(n * 32, 7, np.uint8)
    opt = rc.options(0, "fast")
    r = rc.hip_lib().rc_pick(scene.packed(), *FULL, ctypes.byref(opt), 1, n,
                             pts.ctypes.data_as(ctypes.c_void_p),
                             hits.ctypes.data_as(ctypes.c_void_p))
    assert r == -1 and np.all(hits == 7)


# --------------------------------------------------------------------- 5. edge map --
EDGE_SCENES = ["simple", "reflection", "quadric"]
EDGE_SIZES = [(64, 48), (33, 17)]


def gpu_edge_rates(torch, ids, s, base):
    h, w = ids.shape
    d_id = torch.from_numpy(np.array(ids, dtype=I32)).cuda()      # a writable copy
    d_rates = torch.full((w * h + TAIL,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc.id_edge_rates_device(d_id.data_ptr(), w, h, s, d_rates.data_ptr(), base=base)
    torch.cuda.synchronize()
    a = d_rates.cpu().numpy()
    assert np.all(a[-TAIL:] == 0x5a)
    return a[:-TAIL].reshape(h, w)


def test_edge_map(torch):
    rng = np.random.default_rng(5500)
    planes = []
    for name, (w, h) in itertools.product(EDGE_SCENES, EDGE_SIZES):
        ids = ref_planes(name, False, (w, h, 0, 0), w, h)["id"]
        share = np.count_nonzero(rc.id_edge_rates(ids, 4, 1) == 4) / ids.size
        assert 0.01 <= share <= 0.60, (name, w, h, share)      # the input has edges and interiors
        planes.append(ids)
    for shape in ((1, 1), (1, 9), (9, 1), (17, 33)):
        planes.append(rng.integers(-1, 4, shape).astype(I32))
    for ids in planes:
        for s, base in itertools.product((2, 4, 8), (0, 1)):
            np.testing.assert_array_equal(gpu_edge_rates(torch, ids, s, base),
                                          rc.id_edge_rates(ids, s, base),
                                          err_msg=f"{ids.shape} s{s} base{base}")


# ------------------------------------------------------------ 6. the recipe end to end --
_IMG = {}


def oracle_ssaa(name, w, h, s, mode):
    """The oracle's ssaa = s image of that mode at DEPTH: computed once per key, read-only."""
    key = (name, w, h, s, mode)
    if key not in _IMG:
        scene = pc.list_scenes()[name]
        if mode == "cuda":
            big = oracle_render_cuda(scene, s * w, s * h, DEPTH)
        else:
            big, _ = oracle_render(scene, s * w, s * h, DEPTH, mode)
        _IMG[key] = rc.box_downsample(big, s)
        _IMG[key].setflags(write=False)
    return _IMG[key]


@pytest.mark.parametrize("mode", ["fast", "cuda"])
@pytest.mark.parametrize("name", ["simple", "quadric"])
def test_geometric_edge_recipe(name, mode, torch):
    """G-buffer, edge map, rate-map frame: three enqueues on one non-default stream with no host
    synchronisation in between."""
    scene = pc.list_scenes()[name]
    stream = torch.cuda.Stream()
    for (w, h), base in itertools.product(EDGE_SIZES, (1, 0)):
        ids = ref_planes(name, mode == "cuda", (w, h, 0, 0), w, h)["id"]
        rates = rc.id_edge_rates(ids, 4, base)
        assert 0 < np.count_nonzero(rates == 4) < rates.size
        rng = np.random.default_rng(6600 + w)
        prefill = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        want = rc.rates_compose(prefill, {1: oracle_ssaa(name, w, h, 1, mode),
                                          4: oracle_ssaa(name, w, h, 4, mode)}, rates)
        d_id = torch.full((w * h,), SENTINEL, dtype=torch.int32, device="cuda")
        d_rates = torch.full((w * h,), 0x5a, dtype=torch.uint8, device="cuda")
        d_out = torch.from_numpy(prefill).cuda()
        torch.cuda.synchronize()
        sp = stream.cuda_stream
        rc.render_gbuffer_device(scene, w, h, d_id_ptr=d_id.data_ptr(), stream_ptr=sp, mode=mode)
        rc.id_edge_rates_device(d_id.data_ptr(), w, h, 4, d_rates.data_ptr(), base=base,
                                stream_ptr=sp)
        rc.render_rates_device(scene, w, h, d_rates.data_ptr(), d_out.data_ptr(), stream_ptr=sp,
                               depth=DEPTH, mode=mode)
        stream.synchronize()
        tag = f"{name} {mode} {w}x{h} base {base}"
        np.testing.assert_array_equal(d_rates.cpu().numpy().reshape(h, w), rates, err_msg=tag)
        np.testing.assert_array_equal(d_out.cpu().numpy(), want, err_msg=tag)
        if base == 0:          # rate-0 pixels keep their bytes
            keep = rates == 0
            assert keep.any() and np.array_equal(d_out.cpu().numpy()[keep], prefill[keep])


# ------------------------------------------------------------------------ 7. state --
def test_state(torch):
    name, (w, h) = "quadric", (64, 48)
    scene = pc.list_scenes()[name]
    rates = np.array(rc.RATE_VALUES, np.uint8)[np.arange(w * h) % len(rc.RATE_VALUES)].reshape(h, w)
    d_rates = torch.from_numpy(rates).cuda()
    d_out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    # a rate-map frame takes the event set: no G-buffer frame owns spans (before any, too)
    rc.render_rates_device(scene, w, h, d_rates.data_ptr(), d_out.data_ptr(), depth=DEPTH)
    with pytest.raises(RuntimeError):
        rc.gbuffer_phase_ms()
    # a G-buffer frame between the rate-map frame and its stats
    tim = {}
    win = (*FULL, 5, 3)
    got = gpu_planes(torch, scene, "fast", win, w, h, ALL4, timing=tim)
    stats = rc.rate_stats()
    assert stats["invalid"] == 0 and all(n > 0 for n in stats["pixels"].values())
    assert stats["pixels"] == {s: int(np.count_nonzero(rates == s)) for s in (1, 2, 4, 8)}
    ms = rc.gbuffer_phase_ms()
    assert sorted(ms) == ["kernel"] and ms["kernel"] > 0.0
    assert tim["kernel_ms"] == pytest.approx(ms["kernel"]) and tim["resolve_ms"] == 0.0
    with pytest.raises(RuntimeError):
        rc.rate_phase_ms()                      # the G-buffer frame recorded the set anew
    want = crop(ref_planes(name, False, (*FULL, 0, 0), *FULL), 5, 3, w, h)
    assert_planes(got, want, ALL4, "state")
    # the oracle's event sum for the window: 0 on these scenes (no zero-length direction, d.z = -1,
    # and no hit with a zero-length normal), so the counter is checked at 0
    assert want["zero"] == 0 and tim["zero_normalize"] == 0
    # a pick frame is a G-buffer frame: it owns the spans after it
    rc.render_rates_device(scene, w, h, d_rates.data_ptr(), d_out.data_ptr(), depth=DEPTH)
    rc.pick(scene, *FULL, pick_points(65))
    assert rc.gbuffer_phase_ms()["kernel"] > 0.0
    assert rc.rate_stats() == stats
