"""A free camera and rays with origins on the GPU (rc_render_camera*, rc_trace_rays_from*, DESIGN.md
§24).  Every comparison is exact: image bytes, and float bit patterns through assert_same_floats /
assert_same_hits.  The expectation is tests/ray_cases.py's ref_trace_from: the oracle's scan and
shade exports with the fast-mode loop between them, itself held against the oracle's own loop in
tests/test_camera.py."""
import numpy as np
import pytest

import prim_cases as pc
import ray_cases as rcs
import shade_cases as shc
import view_cases as vc
from helpers import rc
from test_gpu_rays import assert_same_floats, assert_same_hits, random_units

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = rcs.SIZE
DEPTH = rcs.DEPTH


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def tiled(eye, n):
    return np.tile(np.asarray(eye, F32), (n, 1))


def check_camera(name, eye, m, min_hits=0.30, bounce=True):
    """k_camera against the oracle, and against k_rays_from on the same rays (which has no eye
    table): two device paths and one oracle."""
    sc = rcs.scene(name)
    ids = rcs.camera_samples(name, eye, m)[2]
    assert (ids >= 0).mean() >= min_hits, (name, eye)                 # not a black image
    if bounce:
        assert rcs.bounce_changes(name, eye, m) > 0.0, (name, eye)
    want = rcs.camera_image(name, eye, m)
    got = rc.render_camera(sc, eye, m, W, H, depth=DEPTH)
    np.testing.assert_array_equal(got, want, err_msg=f"{name} {eye}")
    d = rcs.camera_dirs(sc, m, (W, H), rc.view_grid(W, H))
    rays = rc.trace_rays_from(sc, tiled(eye, len(d)), d, ("rgb8",), depth=DEPTH)["rgb8"]
    np.testing.assert_array_equal(rays.reshape(H, W, 3), got, err_msg=f"rays {name} {eye}")


# ------------------------------------------------------------- 1. cameras and the oracle --
@pytest.mark.parametrize("k", range(len(rcs.CAMERAS)),
                         ids=[f"{c[0]}-{k}" for k, c in enumerate(rcs.CAMERAS)])
def test_camera_follows_the_oracle(k):
    name, eye, m = rcs.CAMERAS[k]
    check_camera(name, eye, m, bounce=k not in rcs.NO_BOUNCE)


def first_sphere_centre(js):
    ty, pos, _ = pc.shape_table(js)
    return tuple(float(v) for v in pos[np.flatnonzero(ty == pc.SPHERE)[0]].astype(F32))


@pytest.mark.parametrize("name", ["random65", "random64"])
def test_scenes_too_large_to_stage(name):
    """More shapes than the LDS copy of the scene holds: k_camera's general path.  The eye is the
    centre of the scene's first sphere, so the oracle's scan hits in every direction."""
    sc = rcs.scene(name)
    assert sc.num_shapes + 1 > 32
    check_camera(name, first_sphere_centre(sc.js), rc.view_euler(0.2, 0.1), bounce=False)


def test_cross_terms():
    """Quadrics with d, e, f: the table's entries and the scan without the cross-term-free form."""
    sc = rcs.scene("random14x")
    assert (pc.shape_table(sc.js)[2][:, 3:6] != 0).any()
    check_camera("random14x", first_sphere_centre(sc.js), rc.view_euler(0.2, 0.1), bounce=False)
    check_camera("random14x", (1.0, 0.5, 2.0), rcs.IDENT, min_hits=0.0, bounce=False)


# ----------------------------------------------------------- 2. supersampling and windows --
@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_supersampling(s, torch):
    """37 x 29: no multiple of the 8 x 8 wave block."""
    eye, m, size = (0.5, 0.25, 1.0), rc.view_euler(0.1, -0.05), (37, 29)
    want = rcs.camera_image("quadric", eye, m, s, size)
    assert want.any(axis=2).mean() >= 0.30
    d_out = torch.full((size[1], size[0], 3), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc.render_camera_device(rcs.scene("quadric"), eye, m, *size, d_out.data_ptr(), ssaa=s,
                            depth=DEPTH)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy(), want)
    np.testing.assert_array_equal(
        rc.render_camera(rcs.scene("quadric"), eye, m, *size, ssaa=s, depth=DEPTH), want)


def eye_with_an_edge(name, window, size, a, b):
    """An eye on the segment a .. b for which the window looks at an edge between two shapes.  The
    window spans a few millionths of a radian, so from a and from b it sees one shape each (two
    different ones); the eye is bisected in float32, on the oracle's side, until both are in it."""
    def ids(eye):
        return rcs.camera_samples(name, eye, rcs.IDENT, 1, size, window)[2]
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ia, ib = np.unique(ids(tuple(a))), np.unique(ids(tuple(b)))
    assert len(ia) == len(ib) == 1 and ia[0] != ib[0] and ia[0] >= 0
    lo, hi = 0.0, 1.0
    for _ in range(60):
        mid = (lo + hi) / 2
        eye = tuple(float(v) for v in (a + mid * (b - a)).astype(F32))
        got = np.unique(ids(eye))
        if len(got) > 1:
            return eye
        lo, hi = (mid, hi) if got[0] == ia[0] else (lo, mid)
    raise AssertionError("no eye of the segment puts an edge into the window")


def test_window_of_a_huge_virtual_image():
    full, at, size = (33554433, 33554431), (33554000, 1000003), (40, 24)
    win = (*full, *at)
    eye = eye_with_an_edge("quadric", win, size, (-2.0, -2.0, 1.0), (-6.0, -5.0, 0.0))
    for s in (1, 2):
        want = rcs.camera_image("quadric", eye, rcs.IDENT, s, size, win)
        # conditions on the input: the window looks at an edge, which the eye at the origin
        # does not see there
        assert len(np.unique(want.reshape(-1, 3), axis=0)) >= 2, eye
        got = rc.render_camera(rcs.scene("quadric"), eye, rcs.IDENT, *size, window=win, ssaa=s,
                               depth=DEPTH)
        np.testing.assert_array_equal(got, want, err_msg=f"s{s} {eye}")
    plain = rc.render_view(rcs.scene("quadric"), rcs.IDENT, *size, window=win, depth=DEPTH)
    assert (plain != rcs.camera_image("quadric", eye, rcs.IDENT, 1, size, win)).any()


# --------------------------------------------------------------------------- 3. identities --
@pytest.mark.parametrize("view", list(vc.VIEWS))
def test_eye_at_the_origin_is_the_view(view):
    sc = vc.scene("quadric")
    want = rc.render_view(sc, vc.VIEWS[view], *vc.FULL, ssaa=2, depth=DEPTH)
    for eye in ((0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (0.0, -0.0, 0.0)):
        got = rc.render_camera(sc, eye, vc.VIEWS[view], *vc.FULL, ssaa=2, depth=DEPTH)
        np.testing.assert_array_equal(got, want, err_msg=f"{view} {eye}")


def test_eye_at_the_origin_with_the_identity_is_the_plain_render():
    for name in ("simple", "reflection", "quadric"):
        sc = vc.scene(name)
        want = rc.render(sc, W, H, depth=DEPTH, mode="fast")
        for eye in ((0.0, 0.0, 0.0), (-0.0, -0.0, -0.0)):
            np.testing.assert_array_equal(rc.render_camera(sc, eye, None, W, H, depth=DEPTH), want,
                                          err_msg=f"{name} {eye}")


# -------------------------------------------------------------------------- 4. ray batches --
def gather_rays(name="quadric", n=None):
    """The rays an occlusion or gather pass shoots: origins are the primary hit points of the 64 x 48
    frame, directions seeded random unit vectors."""
    sc = rcs.scene(name)
    d0 = rcs.camera_dirs(sc, rcs.IDENT, (W, H), rc.view_grid(W, H))
    _, ids, _, P, _ = rcs.ref_trace_from(sc.js, np.zeros_like(d0), d0, 1)
    P = P[ids >= 0]
    assert len(P) >= 1000
    n = n or len(P)
    O = P[np.arange(n) % len(P)]
    return np.ascontiguousarray(O, F32), random_units(777, n)


def expect(name, O, D, frame):
    rgb, ids, t, P, N = rcs.ref_trace_from(rcs.scene(name).js, O, D, DEPTH + 1)
    return {"rgb": rgb, "rgb8": vc.oracle_quant(rgb), "hits": rcs.hits_records(ids, t, P, N, frame)}


def check_batch(name, O, D, frame, tag):
    want = expect(name, O, D, frame)
    got = rc.trace_rays_from(rcs.scene(name), O, D, ("rgb8", "rgb", "hits"), frame=frame,
                             depth=DEPTH)
    assert_same_floats(got["rgb"], want["rgb"], f"rgb {tag}")
    np.testing.assert_array_equal(got["rgb8"], want["rgb8"], err_msg=f"rgb8 {tag}")
    assert_same_hits(got["hits"], want["hits"], tag)
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_batch_sizes(n):
    O, D = gather_rays(n=n)
    for frame in (True, False):
        want = check_batch("quadric", O, D, frame, f"n {n} frame {frame}")
    if n >= 257:
        hit = want["hits"]["id"] >= 0
        assert 0.2 <= hit.mean() <= 0.99 and want["rgb8"].any()      # hits and misses both


@pytest.mark.parametrize("name", ["reflection", "random14x", "random65"])
def test_batches_on_other_scenes(name):
    O, D = gather_rays("quadric", 2000)        # any points will do as origins
    want = check_batch(name, O, D, True, name)
    assert (want["hits"]["id"] >= 0).mean() >= 0.05


def test_nonfinite_origins_are_misses_as_in_the_oracle():
    O, D = gather_rays(n=640)
    O = O.copy()
    bad = [np.nan, np.inf, -np.inf]
    for k in range(0, 640, 5):                 # every fifth ray, components in turn
        O[k, (k // 5) % 3] = bad[(k // 15) % 3]
    O[3::40] = F32(3e38)
    O[7::40, 1] = F32(-3e38)
    want = check_batch("quadric", O, D, True, "nonfinite")
    nonfinite = ~np.isfinite(O).all(axis=1)
    assert nonfinite.sum() == 128 and (want["hits"]["id"][nonfinite] == -1).all()
    assert (want["hits"]["id"][~nonfinite] >= 0).any()
    check_batch("random14x", O, D, True, "nonfinite, cross terms")


def test_scaled_directions_are_used_as_given():
    O, D = gather_rays(n=2000)
    unit = expect("quadric", O, D, False)["hits"]
    for k in (3.0, 1e-3):
        Dk = (D * F32(k)).astype(F32)
        want = check_batch("quadric", O, Dk, True, f"scale {k}")["hits"]
        hit = (unit["id"] >= 0) & (want["id"] >= 0)
        assert hit.sum() >= 100 and (unit["t"][hit] != want["t"][hit]).mean() > 0.9


@pytest.mark.parametrize("only", ["rgb8", "rgb", "hits"])
def test_only_the_requested_output_is_written(only, torch):
    """Guard bytes: one buffer per output with 64 bytes of 0x5a on either side; the one asked for
    is written between its guards and the others stay untouched."""
    O, D = gather_rays(n=1000)
    n, G = len(D), 64
    want = expect("quadric", O, D, True)
    d_o, d_d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    size = {"rgb8": 3 * n, "rgb": 12 * n, "hits": 32 * n}
    bufs = {k: torch.full((G + v + G,), 0x5a, dtype=torch.uint8, device="cuda")
            for k, v in size.items()}
    assert all((b.data_ptr() + G) % 16 == 0 for b in bufs.values())
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    rc.trace_rays_from_device(rcs.scene("quadric"), n, d_o.data_ptr(), d_d.data_ptr(), frame=True,
                              depth=DEPTH, stream_ptr=stream.cuda_stream,
                              **{f"d_{only}_ptr": bufs[only].data_ptr() + G})
    torch.cuda.synchronize()
    for name, buf in bufs.items():
        raw = buf.cpu().numpy()
        assert (raw[:G] == 0x5a).all() and (raw[-G:] == 0x5a).all(), name
        body = raw[G:-G]
        if name != only:
            assert (body == 0x5a).all(), name
        elif name == "rgb8":
            np.testing.assert_array_equal(body.reshape(n, 3), want["rgb8"])
        elif name == "rgb":
            assert_same_floats(body.view(F32).reshape(n, 3), want["rgb"], "rgb")
        else:
            assert_same_hits(body.view(rc.HIT_DTYPE).reshape(-1), want["hits"], "hits")


# ------------------------------------------------------------------------------ 5. streams --
def test_two_cameras_on_two_streams(torch):
    """Two frames with different eyes enqueued back to back on two streams, each its own oracle
    image: the eye's table is the workgroup's own, nothing is shared between frames in flight."""
    cams = [rcs.CAMERAS[8], rcs.CAMERAS[11], rcs.CAMERAS[9], rcs.CAMERAS[12]]      # all quadric
    assert {c[0] for c in cams} == {"quadric"}
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in cams]
    want = [rcs.camera_image(n, e, m, 2) for n, e, m in cams]
    assert len({w.tobytes() for w in want}) == len(want)
    torch.cuda.synchronize()
    for k, (name, eye, m) in enumerate(cams):
        rc.render_camera_device(rcs.scene(name), eye, m, W, H, bufs[k].data_ptr(), ssaa=2,
                                depth=DEPTH, stream_ptr=streams[k % 2].cuda_stream)
    torch.cuda.synchronize()
    for k, buf in enumerate(bufs):
        np.testing.assert_array_equal(buf.cpu().numpy(), want[k], err_msg=str(cams[k][1]))


# ---------------------------------------------------------------------------- 6. refusals --
def test_refusals_leave_device_buffers_untouched(torch):
    """The messages are pinned in tests/golden/camera_refusals.json (tests/test_camera.py, which
    runs without a GPU); here every kind of refusal meets real device buffers."""
    sc = rcs.scene("simple")
    eye = (0.5, 0.25, 1.0)
    d_img = torch.full((H, W, 3), 0x5a, dtype=torch.uint8, device="cuda")
    O, D = gather_rays(n=8)
    d_o, d_d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    d_hits = torch.full((8, 32), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for kw in ({"mode": "cuda"}, {"mode": "parity"}, {"ssaa": 3}, {"window": (64, 48, 60, 40)}):
        with pytest.raises(RuntimeError):
            rc.render_camera_device(sc, eye, None, W, H, d_img.data_ptr(), **kw)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(RuntimeError):
            rc.render_camera_device(sc, (0.0, bad, 0.0), None, W, H, d_img.data_ptr())
        with pytest.raises(RuntimeError):
            rc.render_camera_device(sc, eye, np.diag([1.0, bad, 1.0]), W, H, d_img.data_ptr())
    hits = {"d_hits_ptr": d_hits.data_ptr()}
    for mode in ("cuda", "parity"):
        with pytest.raises(RuntimeError):
            rc.trace_rays_from_device(sc, 8, d_o.data_ptr(), d_d.data_ptr(), mode=mode, **hits)
        with pytest.raises(RuntimeError):
            rc.trace_rays_from(sc, O, D, mode=mode)
    with pytest.raises(RuntimeError):          # a null origins pointer
        rc.trace_rays_from_device(sc, 8, 0, d_d.data_ptr(), **hits)
    with pytest.raises(RuntimeError):          # all three outputs null
        rc.trace_rays_from_device(sc, 8, d_o.data_ptr(), d_d.data_ptr())
    with pytest.raises(RuntimeError):          # records not 16-byte aligned
        rc.trace_rays_from_device(sc, 7, d_o.data_ptr(), d_d.data_ptr(),
                                  d_hits_ptr=d_hits.data_ptr() + 4)
    for n in (0, (1 << 24) + 1):
        with pytest.raises(RuntimeError):
            rc.trace_rays_from_device(sc, n, d_o.data_ptr(), d_d.data_ptr(), **hits)
    torch.cuda.synchronize()
    assert (d_img.cpu().numpy() == 0x5a).all() and (d_hits.cpu().numpy() == 0x5a).all()


# ------------------------------------------- 7. state of the other families (§15) --
def test_other_families_keep_their_state(torch):
    """An accumulation pass, a G-buffer call and a view call give the same bytes after a camera
    frame and a batch of rays with origins as before them."""
    sc = rcs.scene("quadric")
    d_out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    d_acc = torch.zeros((H, W, 4), dtype=torch.int16, device="cuda")
    O, D = gather_rays(n=500)

    def others():
        rc.accum_pass_device(sc, W, H, "hier4", 0, 3, d_acc.data_ptr(), d_out.data_ptr(),
                             reset=True, depth=DEPTH)
        torch.cuda.synchronize()
        acc, px, stats = d_acc.cpu().numpy().copy(), d_out.cpu().numpy().copy(), rc.accum_stats()
        planes = rc.render_gbuffer(sc, W, H, ("id", "t", "P", "N"))
        view = rc.render_view(sc, vc.VIEWS["ypr"], W, H, ssaa=2, depth=DEPTH)
        return acc, px, stats, planes, view

    before = others()
    accum = rc.accum_stats()
    rc.render_camera(sc, (0.5, 0.25, 1.0), vc.VIEWS["yaw10"], W, H, ssaa=2, depth=DEPTH)
    ms = rc.view_phase_ms()                    # a camera frame is a view frame to the spans
    assert sorted(ms) == ["kernel"] and ms["kernel"] > 0.0
    assert rc.accum_stats() == accum
    rc.render_camera_device(sc, (2.0, 3.0, -8.0), None, W, H, d_out.data_ptr(), depth=DEPTH)
    rc.trace_rays_from(sc, O, D, ("rgb", "hits"), frame=True, depth=DEPTH)
    assert rc.view_phase_ms()["kernel"] > 0.0 and rc.accum_stats() == accum
    d_o, d_d = torch.from_numpy(O).cuda(), torch.from_numpy(D).cuda()
    d_rgb = torch.zeros((len(D), 3), dtype=torch.float32, device="cuda")
    rc.trace_rays_from_device(sc, len(D), d_o.data_ptr(), d_d.data_ptr(),
                              d_rgb_ptr=d_rgb.data_ptr(), depth=DEPTH)
    assert rc.view_phase_ms()["kernel"] > 0.0 and rc.accum_stats() == accum
    after = others()
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    assert after[2] == before[2]
    for k in before[3]:
        np.testing.assert_array_equal(after[3][k].view(np.uint32), before[3][k].view(np.uint32),
                                      err_msg=k)
    np.testing.assert_array_equal(after[4], before[4])
