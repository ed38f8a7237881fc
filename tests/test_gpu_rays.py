"""Caller-supplied ray batches on the GPU (rc_trace_rays*): every output is the CPU
oracle's own routine for that direction, used as given — rgb is rco_prim_shoot /
rco_prim_shoot_cuda bit for bit (one NaN equal to another, tests/test_gpu_shading.py's rule), rgb8
is rco_prim_quant of it and a record is rco_prim_nearest(O = 0, D, skip = -1)."""
import numpy as np
import pytest

import prim_cases as pc
import view_cases as vc
from helpers import rc
from test_gpu_prims import same_bits32

pytestmark = pytest.mark.gpu

F32 = np.float32
FULL = vc.FULL
DEPTH = vc.DEPTH
SIZES = [1, 63, 64, 65, 5917]            # one lane; around one wave; 97 * 61, 24 workgroups


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def axes():
    """The six signed axes with +0 and -0 in the zero components."""
    out = []
    for k in range(3):
        for sign in (1.0, -1.0):
            for zero in (0.0, -0.0):
                d = np.full(3, zero, F32)
                d[k] = sign
                out.append(d)
    return np.array(out, F32)


def random_units(seed, n):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def direction_lists(name, mode):
    """label -> [n, 3] float32: view_dirs of the 97 x 61 grid under two views, seeded random unit
    vectors, the same scaled by 3 and by 1e-3 (used as given: the result follows the oracle, it is
    not renormalised) and the signed axes."""
    units = random_units(4242, 5917)
    return {"grid/yaw30": vc.grid_dirs(name, "yaw30", 1, mode),
            "grid/ypr": vc.grid_dirs(name, "ypr", 1, mode),
            "units": units, "units*3": (units * F32(3.0)).astype(F32),
            "units*1e-3": (units * F32(1e-3)).astype(F32), "axes": axes()}


def assert_same_floats(got, want, tag):
    ok = same_bits32(got, want)
    if not ok.all():
        i = int(np.argwhere(~ok)[0][0])
        pytest.fail(f"{tag}: {int((~ok).sum())} floats differ, first in ray {i}: device "
                    f"{pc.bits32(got[i])} oracle {pc.bits32(want[i])}")


def assert_same_hits(got, want, tag):
    np.testing.assert_array_equal(got["id"], want["id"], err_msg=f"id {tag}")
    for f in ("t", "P", "N"):
        assert_same_floats(got[f], want[f], f"{f} {tag}")


def expect(name, d, mode, frame):
    rgb, zero, _ = vc.oracle_shoot(name, d, mode)
    if mode == "cuda":
        hits, hz = vc.oracle_hits_cuda(name, d), 0
    else:
        hits, hz = vc.oracle_hits(name, d, frame)
    return {"rgb": rgb, "rgb8": vc.oracle_quant(rgb), "hits": hits}, zero + hz


def check_batch(name, d, mode, frame, tag):
    want, _ = expect(name, d, mode, frame)
    got = rc.trace_rays(vc.scene(name), d, ("rgb8", "rgb", "hits"), frame=frame, depth=DEPTH,
                        mode=mode)
    assert_same_floats(got["rgb"], want["rgb"], f"rgb {tag}")
    np.testing.assert_array_equal(got["rgb8"], want["rgb8"], err_msg=f"rgb8 {tag}")
    assert_same_hits(got["hits"], want["hits"], tag)
    return want


# --------------------------------------------------------------------- 1. the outputs --
@pytest.mark.parametrize("mode", ["fast", "cuda"])
@pytest.mark.parametrize("name", ["simple", "reflection", "quadric", "mirror_behind"])
def test_rays_follow_the_oracle(name, mode):
    hit_some = False
    for label, d in direction_lists(name, mode).items():
        want = check_batch(name, d, mode, mode == "fast", f"{name} {mode} {label}")
        hit_some = hit_some or (want["hits"]["id"] >= 0).any()
    assert hit_some


@pytest.mark.parametrize("n", SIZES)
def test_sizes(n):
    d = vc.grid_dirs("quadric", "yaw30", 1, "fast")
    d = d[np.linspace(0, len(d) - 1, n).astype(np.int64)]       # spread over the whole image
    for frame in (False, True):
        check_batch("quadric", d, "fast", frame, f"n {n} frame {frame}")
    check_batch("quadric", d, "cuda", False, f"n {n} cuda")


def test_scaled_directions_are_not_renormalised():
    """A condition on the inputs: used as given, a scaled direction's record differs from the unit
    direction's (t scales with 1 / |d|), so a kernel that normalised could not pass."""
    u = random_units(4242, 5917)
    a = vc.oracle_hits("quadric", u, False)[0]
    b = vc.oracle_hits("quadric", (u * F32(3.0)).astype(F32), False)[0]
    hit = (a["id"] >= 0) & (b["id"] >= 0)
    assert hit.sum() >= 100 and (a["t"][hit] != b["t"][hit]).mean() > 0.9


# ------------------------------------------------------------ 2. rays against a frame --
@pytest.mark.parametrize("mode", ["fast", "cuda"])
def test_rays_of_a_view_are_the_views_image(mode, torch):
    sc = vc.scene("quadric")
    d = vc.grid_dirs("quadric", "ypr", 1, mode)
    d_dirs = torch.from_numpy(d).cuda()
    d_rgb8 = torch.zeros((len(d), 3), dtype=torch.uint8, device="cuda")
    d_img = torch.zeros((FULL[1], FULL[0], 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc.trace_rays_device(sc, len(d), d_dirs.data_ptr(), d_rgb8_ptr=d_rgb8.data_ptr(), depth=DEPTH,
                         mode=mode)
    rc.render_view_device(sc, vc.VIEWS["ypr"], *FULL, d_img.data_ptr(), depth=DEPTH, mode=mode)
    torch.cuda.synchronize()
    img = d_img.cpu().numpy()
    np.testing.assert_array_equal(d_rgb8.cpu().numpy().reshape(img.shape), img)
    np.testing.assert_array_equal(img, vc.view_image("quadric", "ypr", 1, mode)[0])


def test_picking_in_a_turned_view():
    """What is under pixel (x, y) of a turned view: trace_rays(view_dirs of that pixel), the id
    plane of the oracle's scan along the view's directions."""
    d = vc.grid_dirs("quadric", "yaw30", 1, "fast")
    ids = vc.oracle_hits("quadric", d, False)[0]["id"].reshape(FULL[1], FULL[0])
    assert len(np.unique(ids)) >= 3
    js = vc.scene("quadric").js
    xy = np.array([[48, 30], [0, 0], [96, 60], [20, 45], [70, 12]])
    one = rc.view_dirs(js.camera_width, js.camera_height, FULL, xy, vc.VIEWS["yaw30"])
    got = rc.trace_rays(vc.scene("quadric"), one, ("hits",), frame=True)["hits"]
    assert got["id"].tolist() == [int(ids[y, x]) for x, y in xy]


# ------------------------------------------------------------ 3. null outputs, streams --
@pytest.mark.parametrize("only", ["rgb8", "rgb", "hits"])
def test_only_the_requested_output_is_written(only, torch):
    sc = vc.scene("quadric")
    d = vc.grid_dirs("quadric", "yaw10", 1, "fast")[:1000]
    want, _ = expect("quadric", d, "fast", True)
    d_dirs = torch.from_numpy(d).cuda()
    bufs = {"rgb8": torch.full((len(d), 3), 0x5a, dtype=torch.uint8, device="cuda"),
            "rgb": torch.full((len(d), 12), 0x5a, dtype=torch.uint8, device="cuda"),
            "hits": torch.full((len(d), 32), 0x5a, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    rc.trace_rays_device(sc, len(d), d_dirs.data_ptr(), frame=True, depth=DEPTH,
                         stream_ptr=stream.cuda_stream,
                         **{f"d_{only}_ptr": bufs[only].data_ptr()})
    torch.cuda.synchronize()
    for name, buf in bufs.items():
        raw = buf.cpu().numpy()
        if name != only:
            assert (raw == 0x5a).all(), name
        elif name == "rgb8":
            np.testing.assert_array_equal(raw, want["rgb8"])
        elif name == "rgb":
            assert_same_floats(raw.view(F32), want["rgb"], "rgb")
        else:
            assert_same_hits(raw.view(rc.HIT_DTYPE).reshape(-1), want["hits"], "hits")


def test_rays_through_a_zero_length_normalisation():
    """The rays of test_gpu_view.py's light-on-the-hit-point scene as a batch: the centre ray's
    light vector has length zero, the C port's normalize leaves it as it is, and the colour and the
    record are the oracle's all the same (the ray entries take no rc_timing; the count itself is
    checked through the view frame there)."""
    d = vc.grid_dirs("light_on_plane_behind", "back", 1, "fast", (5, 3))
    want, events = expect("light_on_plane_behind", d, "fast", True)
    assert events > 0
    got = rc.trace_rays(vc.scene("light_on_plane_behind"), d, ("rgb", "hits"), frame=True,
                        depth=DEPTH)
    assert_same_floats(got["rgb"], want["rgb"], "rgb")
    assert_same_hits(got["hits"], want["hits"], "hits")


# ---------------------------------------------------------------------------- 4. refusals --
def test_refusals(torch):
    sc = vc.scene("simple")
    d = random_units(1, 8)
    d_dirs = torch.from_numpy(d).cuda()
    d_hits = torch.full((8, 32), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):      # frame in cuda mode
        rc.trace_rays(sc, d, ("hits",), frame=True, mode="cuda")
    with pytest.raises(RuntimeError):
        rc.trace_rays_device(sc, 8, d_dirs.data_ptr(), d_hits_ptr=d_hits.data_ptr(), frame=True,
                             mode="cuda")
    with pytest.raises(RuntimeError):      # all three pointers null
        rc.trace_rays_device(sc, 8, d_dirs.data_ptr())
    with pytest.raises(RuntimeError):
        rc.trace_rays(sc, d, ())
    for n in (0, (1 << 24) + 1):           # the device entry cannot see the arrays: n alone
        with pytest.raises(RuntimeError):
            rc.trace_rays_device(sc, n, d_dirs.data_ptr(), d_hits_ptr=d_hits.data_ptr())
    with pytest.raises(RuntimeError):      # parity mode
        rc.trace_rays(sc, d, mode="parity")
    torch.cuda.synchronize()
    assert (d_hits.cpu().numpy() == 0x5a).all()
    # frame without hits is no request for a frame: cuda mode takes it
    rc.trace_rays(sc, d, ("rgb8",), frame=True, mode="cuda")


# ------------------------------------------- 5. state of the other families (§15) --
def test_other_families_keep_their_state(torch):
    sc = vc.scene("simple")
    w, h = 64, 48
    rates = np.ones((h, w), np.uint8)
    rates[8:24, 8:40], rates[30:40, 20:50], rates[40:, :10] = 2, 4, 8
    d_rates = torch.from_numpy(rates).cuda()
    d_out = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    d_acc = torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        rc.render_rates_device(sc, w, h, d_rates.data_ptr(), d_out.data_ptr(), depth=DEPTH)
        rc.view_phase_ms()                     # the rate-map frame took the event set
    rate = rc.rate_stats()
    rc.accum_pass_device(sc, w, h, "hier4", 0, 3, d_acc.data_ptr(), d_out.data_ptr(), reset=True,
                         depth=DEPTH)
    accum = rc.accum_stats()
    assert accum == {"passes": 1, "active_pixels": w * h, "saturated": 0, "rays": 3 * w * h}
    planes = rc.render_gbuffer(sc, w, h, ("id", "t"))
    assert rc.gbuffer_phase_ms()["kernel"] > 0.0
    d = vc.grid_dirs("simple", "yaw10", 1, "fast")
    for frame in ("view", "view_host", "rays", "rays_device"):
        if frame == "view":
            rc.render_view_device(sc, vc.VIEWS["yaw10"], w, h, d_out.data_ptr(), ssaa=2, depth=DEPTH)
        elif frame == "view_host":
            rc.render_view(sc, vc.VIEWS["ypr"], w, h, depth=DEPTH)
        elif frame == "rays":
            rc.trace_rays(sc, d, ("rgb8", "hits"), depth=DEPTH)
        else:
            d_dirs = torch.from_numpy(d).cuda()
            d_rgb = torch.zeros((len(d), 3), dtype=torch.float32, device="cuda")
            rc.trace_rays_device(sc, len(d), d_dirs.data_ptr(), d_rgb_ptr=d_rgb.data_ptr(),
                                 depth=DEPTH)
        ms = rc.view_phase_ms()                # readable after each view or ray frame
        assert sorted(ms) == ["kernel"] and ms["kernel"] > 0.0, frame
        assert rc.rate_stats() == rate and rc.accum_stats() == accum, frame
    # one event set, one owner (§15): the view frame recorded the set anew, so the spans of the
    # frames before it are gone, exactly as after a window frame; their records and buffers stay
    with pytest.raises(RuntimeError):
        rc.gbuffer_phase_ms()
    again = rc.render_gbuffer(sc, w, h, ("id", "t"))
    np.testing.assert_array_equal(again["id"], planes["id"])
    assert rc.gbuffer_phase_ms()["kernel"] > 0.0
    with pytest.raises(RuntimeError):
        rc.view_phase_ms()                     # and the other way round
