"""The G-buffer through a camera, the guided filter and the ambient compose on the GPU
(rc_render_camera_gbuffer*, rc_ao_filter_device, rc_ao_compose_device, rc_render_ambient, DESIGN.md
§28).  Every comparison is exact: ids, the floats' bits, bytes.  The expectation is
tests/guided_cases.py's: the oracle's primary hits and occlusion states, rc.ao_filter and
rc.ao_compose (the contract in numpy) and the oracle's quant.  tests/test_guided.py holds the numpy
rule against a pixel-by-pixel restatement and checks that these inputs make the guide matter."""
import numpy as np
import pytest

import guided_cases as gc
import ray_cases as rcs
from helpers import rc

pytestmark = pytest.mark.gpu

F32, I32, U32 = np.float32, np.int32, np.uint32
INF, NAN = np.inf, np.nan
W, H = gc.SIZE
DEPTH = rcs.DEPTH
GUARD = 64
THRESHOLDS = ((0.9, 0.05), (-INF, INF), (2.0, 0.05))


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


class Buf:
    """nbytes of device memory filled with 0x5a between guard bytes; `off` shifts the start off
    its 64-byte boundary."""

    def __init__(self, torch, nbytes, off=0, data=None):
        self.torch, self.n, self.off = torch, nbytes, off
        self.raw = torch.full((GUARD + off + nbytes + GUARD,), 0x5a, dtype=torch.uint8,
                              device="cuda")
        self.ptr = self.raw.data_ptr() + GUARD + off
        assert (self.raw.data_ptr() + GUARD) % 64 == 0
        if data is not None:
            self.put(data)

    def put(self, a):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        assert len(b) == self.n
        lo = GUARD + self.off
        self.raw[lo:lo + self.n] = self.torch.from_numpy(b.copy()).cuda()
        self.torch.cuda.synchronize()

    def get(self, dtype=np.uint8, shape=None):
        self.torch.cuda.synchronize()
        a = self.raw.cpu().numpy()
        lo = GUARD + self.off
        assert (a[:lo] == 0x5a).all() and (a[lo + self.n:] == 0x5a).all(), "guard bytes"
        out = a[lo:lo + self.n].copy().view(dtype)
        return out.reshape(shape) if shape else out


class Planes:
    """The four G-buffer planes in guarded device memory."""
    SIZES = {"id": 4, "t": 4, "P": 12, "N": 12}

    def __init__(self, torch, w, h, names=("id", "t", "P", "N")):
        self.w, self.h = w, h
        self.bufs = {p: Buf(torch, w * h * self.SIZES[p]) for p in names}

    def ptr(self, p):
        return self.bufs[p].ptr if p in self.bufs else None

    def run(self, sc, eye, m, window=None, stream=None, timing=None):
        rc.render_camera_gbuffer_device(sc, eye, m, self.w, self.h, window=window,
                                        d_id_ptr=self.ptr("id"), d_t_ptr=self.ptr("t"),
                                        d_p_ptr=self.ptr("P"), d_n_ptr=self.ptr("N"),
                                        stream_ptr=stream.cuda_stream if stream else None,
                                        timing=timing)

    def read(self):
        out = {}
        for p, b in self.bufs.items():
            dt, c = rc.GBUFFER_PLANES[p]
            out[p] = b.get(dt, (self.h, self.w) + ((3,) if c == 3 else ()))
        return out


def same_bits(got, want, tag):
    """ids equal, floats bit for bit (-0 is not +0)."""
    for p in got:
        g, x = np.ascontiguousarray(got[p]), np.ascontiguousarray(want[p])
        assert g.shape == x.shape and g.dtype == x.dtype, f"{p} {tag}"
        np.testing.assert_array_equal(g.view(U32), x.view(U32), err_msg=f"{p} {tag}")


# ------------------------------------------------------ 1. the G-buffer through a camera --
@pytest.mark.parametrize("k", gc.CAMS)
def test_the_four_planes_against_the_oracle(k, torch):
    name, eye, m = rcs.CAMERAS[k]
    g = Planes(torch, W, H)
    g.run(rcs.scene(name), eye, m)
    got, want = g.read(), gc.planes(name, eye, m)
    same_bits(got, want, f"camera {k}")
    miss = want["id"] < 0
    assert (got["t"].view(U32)[miss] == 0).all() and (got["P"].view(U32)[miss] == 0).all()
    assert (got["N"].view(U32)[miss] == 0).all()
    assert (want["id"] >= 0).sum() > 0.3 * W * H


def test_the_eye_at_zero_is_rc_render_gbuffers_planes(torch):
    sc = rcs.scene("reflection")
    old = Planes(torch, W, H)
    rc.render_gbuffer_device(sc, W, H, d_id_ptr=old.ptr("id"), d_t_ptr=old.ptr("t"),
                             d_p_ptr=old.ptr("P"), d_n_ptr=old.ptr("N"))
    new = Planes(torch, W, H)
    new.run(sc, (0.0, 0.0, 0.0), rcs.IDENT)
    want = old.read()
    same_bits(new.read(), want, "eye +0")
    assert 0 < (want["id"] >= 0).sum() < W * H


def test_windows_are_crops_of_the_whole_image(torch):
    name, eye, m = rcs.CAMERAS[9]
    sc = rcs.scene(name)
    fw, fh = gc.FULL
    whole = Planes(torch, fw, fh)
    whole.run(sc, eye, m)
    full = whole.read()
    for window, (w, h) in ((gc.WINDOW, gc.SIZE), (gc.CORNER, gc.CORNER_SIZE)):
        g = Planes(torch, w, h)
        g.run(sc, eye, m, window=window)
        got = g.read()
        x0, y0 = window[2:]
        same_bits(got, {p: full[p][y0:y0 + h, x0:x0 + w] for p in full}, f"crop {window}")
        same_bits(got, gc.planes(name, eye, m, (w, h), window), f"oracle {window}")


def test_each_plane_alone(torch):
    name, eye, m = rcs.CAMERAS[14]
    want = gc.planes(name, eye, m)
    for p in ("id", "t", "P", "N"):
        g = Planes(torch, W, H, names=(p,))
        g.run(rcs.scene(name), eye, m)
        same_bits(g.read(), {p: want[p]}, f"{p} alone")


def test_a_scene_too_large_to_stage(torch):
    name, eye, m = "random65", (0.0, 0.0, 5.0), rcs.IDENT
    sc = rcs.scene(name)
    assert sc.num_shapes + 1 > 32
    g = Planes(torch, W, H)
    g.run(sc, eye, m)
    want = gc.planes(name, eye, m)
    same_bits(g.read(), want, name)
    assert (want["id"] >= 0).sum() > 0.3 * W * H


def test_the_gbuffers_host_form(torch):
    name, eye, m = rcs.CAMERAS[3]
    sc = rcs.scene(name)
    timing = {}
    got = rc.render_camera_gbuffer(sc, eye, m, W, H, planes=("id", "t", "P", "N"), timing=timing)
    same_bits(got, gc.planes(name, eye, m), "host form")
    assert timing["kernel_ms"] > 0.0 and rc.gbuffer_phase_ms()["kernel"] > 0.0
    w, h = gc.CORNER_SIZE
    got = rc.render_camera_gbuffer(sc, eye, m, w, h, planes=("id", "N"), window=gc.CORNER)
    want = gc.planes(name, eye, m, (w, h), gc.CORNER)
    same_bits(got, {"id": want["id"], "N": want["N"]}, "host corner")


# ----------------------------------------------------------- 2. the filter on real data --
def filters():
    out = []
    for r in (0, 1, 3, 8):
        for taps in ("tent", "box"):
            out.append((r, taps))
    out.append((3, [6, 4, 2, 1]))
    return out


@pytest.mark.parametrize("k", gc.CAMS)
def test_the_filter_on_camera_frames(k, torch):
    """The state from k_ao, the guide from k_camera_gbuffer, every run against rc.ao_filter on
    the oracle's planes."""
    name, eye, m = rcs.CAMERAS[k]
    sc = rcs.scene(name)
    g = Planes(torch, W, H)
    g.run(sc, eye, m)
    want_g = gc.planes(name, eye, m)
    for sets in (gc.two_pass_sets(16), [rc.ao_dirs(1)]):
        ao = Buf(torch, W * H * 4)
        for j, dirs in enumerate(sets):
            rc.ao_pass_device(sc, eye, m, W, H, dirs, ao.ptr, reset=j == 0, depth=DEPTH)
        acc = gc.state(name, eye, m, sets)
        np.testing.assert_array_equal(ao.get(rc.AO_DTYPE, (H, W)), acc)
        plain = Buf(torch, W * H)
        rc.ao_resolve_device(ao.ptr, W, H, plain.ptr)
        resolved = plain.get(shape=(H, W))
        for r, taps in filters():
            for nmin, dplane in THRESHOLDS:
                f = rc.ao_filter_params(r, taps, nmin, dplane)
                out = Buf(torch, W * H)
                rc.ao_filter_device(ao.ptr, g.ptr("id"), g.ptr("P"), g.ptr("N"), W, H, f, out.ptr)
                got = out.get(shape=(H, W))
                tag = f"camera {k} sets {len(sets)} r{r} {taps} nmin {nmin} dplane {dplane}"
                want = rc.ao_filter(acc, want_g["id"], want_g["P"], want_g["N"], f)
                np.testing.assert_array_equal(got, want, err_msg=tag)
                if nmin == 2.0 or r == 0:
                    np.testing.assert_array_equal(got, resolved, err_msg=tag)


# ------------------------------------------------------ 3. the filter on synthetic planes --
def synthetic(w, h, seed):
    """A state and a guide from numpy: ids in {-1, 0, 1, 2}, near-flat surfaces so that the
    thresholds split the neighbours, with NaN, +-inf and -0 sprinkled into P and N and records
    without rays."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(-1, 3, (h, w)).astype(I32)
    ids[rng.random((h, w)) < 0.5] = 1                    # one large surface
    N = np.zeros((h, w, 3), F32)
    N[..., 2] = 1.0
    N += rng.normal(0, 0.25, (h, w, 3)).astype(F32)
    N /= np.linalg.norm(N, axis=2, keepdims=True).astype(F32)
    P = np.zeros((h, w, 3), F32)
    P[..., 0], P[..., 1] = np.arange(w)[None, :] * 0.1, np.arange(h)[:, None] * 0.1
    P[..., 2] = -5.0 + rng.normal(0, 0.04, (h, w))
    for a in (P, N):
        flat = a.reshape(-1)
        pick = rng.random(flat.shape) < 0.03
        flat[pick] = rng.choice(np.array([NAN, INF, -INF, -0.0], F32), int(pick.sum()))
    acc = np.zeros((h, w), rc.AO_DTYPE)
    acc["rays"] = rng.integers(0, 200, (h, w))
    acc["open"] = (acc["rays"] * rng.random((h, w))).astype(np.uint16)
    acc["rays"][rng.random((h, w)) < 0.1] = 0
    acc["open"][acc["rays"] == 0] = 0
    return acc, ids, P, N


def run_filter(torch, acc, ids, P, N, f, off=0):
    h, w = ids.shape
    bufs = [Buf(torch, a.nbytes, data=a) for a in (acc, ids, P, N)]
    out = Buf(torch, w * h, off=off)
    rc.ao_filter_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, w, h, f, out.ptr)
    return out.get(shape=(h, w))


@pytest.mark.parametrize("w,h", [(1, 1), (1, 40), (40, 1), (7, 3), (67, 3), (37, 35)])
def test_the_filter_on_synthetic_planes(w, h, torch):
    acc, ids, P, N = synthetic(w, h, 1000 * w + h)
    seen = set()
    for r, taps in ((0, "box"), (1, [2, 1]), (3, "tent"), (8, "tent"), (8, "box")):
        for nmin, dplane in ((0.9, 0.05), (-INF, INF), (0.5, 0.2)):
            f = rc.ao_filter_params(r, taps, nmin, dplane)
            got = run_filter(torch, acc, ids, P, N, f)
            want = rc.ao_filter(acc, ids, P, N, f)
            np.testing.assert_array_equal(got, want, err_msg=f"{w} x {h} r{r} {taps} {nmin}")
            seen.add(want.tobytes())
    if w * h > 100:
        assert len(seen) > 6                             # radius and thresholds matter here


def test_the_caps_edge(torch):
    """Every record (65535, 65535) under the 181^2 taps at radius 8: the interior sums reach
    32761 * 65535, just below 2^31."""
    w, h = 37, 35
    acc = np.zeros((h, w), rc.AO_DTYPE)
    acc["open"] = acc["rays"] = 65535
    ids = np.zeros((h, w), I32)
    P = np.zeros((h, w, 3), F32)
    N = np.zeros((h, w, 3), F32)
    N[..., 2] = 1.0
    f = rc.ao_filter_params(8, [21] + [10] * 8, -INF, INF)
    got = run_filter(torch, acc, ids, P, N, f)
    assert (got == 255).all()
    acc["open"] = 21845                                   # a third: a wrapped sum would show
    got = run_filter(torch, acc, ids, P, N, f)
    np.testing.assert_array_equal(got, rc.ao_filter(acc, ids, P, N, f))
    assert (got == 85).all()


@pytest.mark.parametrize("off", [1, 2, 3])
def test_an_output_off_its_4_byte_boundary(off, torch):
    acc, ids, P, N = synthetic(37, 35, 77)
    f = rc.ao_filter_params(3, [6, 4, 2, 1])
    got = run_filter(torch, acc, ids, P, N, f, off=off)
    np.testing.assert_array_equal(got, rc.ao_filter(acc, ids, P, N, f))


# ------------------------------------------------------------------------ 4. the compose --
@pytest.mark.parametrize("w", [1, 3, 4, 5, 67])
def test_the_compose(w, torch):
    h = 3
    sc = rcs.scene("quadric")
    n = sc.num_shapes
    rng = np.random.default_rng(w)
    ids = rng.integers(0, n, (h, w)).astype(I32)
    wild = rng.random((h, w))
    ids[wild < 0.1], ids[(wild >= 0.1) & (wild < 0.2)] = -1, n
    ids.flat[-1] = np.iinfo(I32).max
    ao = rng.integers(0, 256, (h, w)).astype(np.uint8)
    ao.flat[0] = 255
    rgb = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    d_id = Buf(torch, ids.nbytes, data=ids)
    for ambient in ((0.2, 0.3, 0.4), (4.0, 4.0, 4.0)):
        table = gc.shape_table(sc.js, ambient)
        want = rc.ao_compose(rgb, ids, ao, table)
        known = (ids >= 0) & (ids < n)
        np.testing.assert_array_equal(want[~known], rgb[~known])
        if w * h > 4:
            assert (want[known] != rgb[known]).any()
        if ambient[0] == 4.0 and w * h > 4:
            assert (want == 255).any()
        for off in range(4):                             # pointers off every alignment
            d_ao = Buf(torch, ao.nbytes, off=off, data=ao)
            d_in = Buf(torch, rgb.nbytes, off=(off + 1) % 4, data=rgb)
            d_out = Buf(torch, rgb.nbytes, off=(off + 2) % 4)
            rc.ao_compose_device(sc, d_id.ptr, d_ao.ptr, ambient, d_in.ptr, d_out.ptr, w, h)
            np.testing.assert_array_equal(d_out.get(shape=(h, w, 3)), want, err_msg=f"off {off}")
            np.testing.assert_array_equal(d_in.get(shape=(h, w, 3)), rgb)
            rc.ao_compose_device(sc, d_id.ptr, d_ao.ptr, ambient, d_in.ptr, d_in.ptr, w, h)
            np.testing.assert_array_equal(d_in.get(shape=(h, w, 3)), want, err_msg=f"in place {off}")


# ------------------------------------------------------------------- 5. the wider system --
def expect_ambient(name, eye, m, sets, f, ambient, size, window):
    sc = rcs.scene(name)
    img = rcs.camera_image(name, eye, m, 1, size, window)
    g = gc.planes(name, eye, m, size, window)
    acc = gc.state(name, eye, m, sets, size, window)
    plane = rc.ao_filter(acc, g["id"], g["P"], g["N"], f)
    return rc.ao_compose(img, g["id"], plane, gc.shape_table(sc.js, ambient))


def test_render_ambient_is_the_composition_of_the_device_entries(torch):
    name, eye, m = rcs.CAMERAS[9]        # its window holds three shapes and the background
    sc, (w, h), window = rcs.scene(name), gc.SIZE, gc.WINDOW
    sets = [rc.ao_dirs(16, 2.0), rc.ao_dirs(5, INF, gc.ROT), rc.ao_dirs(64, 2.0, gc.ROT)]
    f, ambient = rc.ao_filter_params(3, [6, 4, 2, 1]), (0.2, 0.3, 0.4)
    timing = {}
    got = rc.render_ambient(sc, eye, m, w, h, sets, f, ambient, window=window, depth=DEPTH,
                            timing=timing)
    assert timing["kernel_ms"] > 0.0
    # the device entries, one by one
    img, ao, plane = Buf(torch, w * h * 3), Buf(torch, w * h * 4), Buf(torch, w * h)
    g = Planes(torch, w, h, names=("id", "P", "N"))
    rc.render_camera_device(sc, eye, m, w, h, img.ptr, window=window, depth=DEPTH)
    for j, dirs in enumerate(sets):
        rc.ao_pass_device(sc, eye, m, w, h, dirs, ao.ptr, window=window, reset=j == 0,
                          depth=DEPTH)
    g.run(sc, eye, m, window=window)
    rc.ao_filter_device(ao.ptr, g.ptr("id"), g.ptr("P"), g.ptr("N"), w, h, f, plane.ptr)
    rc.ao_compose_device(sc, g.ptr("id"), plane.ptr, ambient, img.ptr, img.ptr, w, h)
    np.testing.assert_array_equal(got, img.get(shape=(h, w, 3)))
    want = expect_ambient(name, eye, m, sets, f, ambient, (w, h), window)
    np.testing.assert_array_equal(got, want)
    assert (want != rcs.camera_image(name, eye, m, 1, (w, h), window)).any()
    one = rc.render_ambient(sc, eye, m, w, h, sets[0], f, ambient, window=window, depth=DEPTH)
    np.testing.assert_array_equal(one, expect_ambient(name, eye, m, sets[:1], f, ambient, (w, h),
                                                      window))


def test_two_filters_on_two_streams(torch):
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = synthetic(67, 35, 5)
    b = synthetic(37, 35, 6)
    fa, fb = rc.ao_filter_params(8, "tent", 0.5, 0.2), rc.ao_filter_params(3, "box")
    da = [Buf(torch, x.nbytes, data=x) for x in a]
    db = [Buf(torch, x.nbytes, data=x) for x in b]
    oa, ob = Buf(torch, 67 * 35), Buf(torch, 37 * 35)
    for _ in range(3):
        rc.ao_filter_device(da[0].ptr, da[1].ptr, da[2].ptr, da[3].ptr, 67, 35, fa, oa.ptr,
                            stream_ptr=s1.cuda_stream)
        rc.ao_filter_device(db[0].ptr, db[1].ptr, db[2].ptr, db[3].ptr, 37, 35, fb, ob.ptr,
                            stream_ptr=s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    np.testing.assert_array_equal(oa.get(shape=(35, 67)), rc.ao_filter(*a, fa))
    np.testing.assert_array_equal(ob.get(shape=(35, 37)), rc.ao_filter(*b, fb))


def test_refusals_leave_live_buffers_alone(torch):
    name, eye, m = rcs.CAMERAS[9]
    sc = rcs.scene(name)
    g = Planes(torch, W, H)
    g.run(sc, eye, m)
    planes = g.read()
    acc, ids, P, N = synthetic(W, H, 9)
    bufs = [Buf(torch, x.nbytes, data=x) for x in (acc, ids, P, N)]
    out, img = Buf(torch, W * H), Buf(torch, W * H * 3)
    good = rc.ao_filter_params(2, "tent")
    bad_f = rc.ao_filter_params(2, "tent")
    bad_f.pad = 1
    with pytest.raises(RuntimeError):
        g.run(sc, (NAN, 0.0, 0.0), m)
    with pytest.raises(RuntimeError):
        g.run(sc, eye, m, window=(64, 48, 60, 0))
    with pytest.raises(RuntimeError):
        rc.render_camera_gbuffer_device(sc, eye, m, W, H, d_id_ptr=g.ptr("id"), mode="cuda")
    for f, ptr, w in ((bad_f, bufs[0].ptr, W), (good, bufs[0].ptr + 2, W), (good, bufs[0].ptr, 0),
                      (rc.ao_filter_params(8, [22] + [10] * 8), bufs[0].ptr, W)):
        with pytest.raises(RuntimeError):
            rc.ao_filter_device(ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, w, H, f, out.ptr)
    with pytest.raises(RuntimeError):
        rc.ao_filter_device(bufs[0].ptr, bufs[1].ptr, None, bufs[3].ptr, W, H, good, out.ptr)
    for ambient, mode in (((0.1, -0.1, 0.1), "fast"), ((NAN, 0.0, 0.0), "fast"),
                          ((0.1, 0.1, 0.1), "parity"), ((0.1, 0.1, 0.1), "cuda")):
        with pytest.raises(RuntimeError):
            rc.ao_compose_device(sc, bufs[1].ptr, out.ptr, ambient, img.ptr, img.ptr, W, H,
                                 mode=mode)
    with pytest.raises(RuntimeError):
        rc.render_ambient(sc, eye, m, W, H, rc.ao_dirs(4), bad_f, (0.1, 0.1, 0.1))
    same_bits(g.read(), planes, "after the refusals")
    assert (out.get() == 0x5a).all() and (img.get() == 0x5a).all()
    np.testing.assert_array_equal(bufs[0].get(rc.AO_DTYPE, (H, W)), acc)


def test_the_other_kernels_bytes_before_and_after(torch):
    """k_camera's image and an occlusion pass's records do not move when the new entries run in
    between."""
    name, eye, m = rcs.CAMERAS[9]
    sc = rcs.scene(name)

    def others():
        img = rc.render_camera(sc, eye, m, W, H, depth=DEPTH)
        ao, out = Buf(torch, W * H * 4), Buf(torch, W * H)
        rc.ao_pass_device(sc, eye, m, W, H, rc.ao_dirs(16, 2.0), ao.ptr, out.ptr, reset=True,
                          depth=DEPTH)
        return img, ao.get(), out.get(), rc.ao_stats()

    before = others()
    np.testing.assert_array_equal(before[0], rcs.camera_image(name, eye, m, 1, gc.SIZE))
    g = Planes(torch, W, H)
    g.run(sc, eye, m)
    acc, ids, P, N = synthetic(W, H, 11)
    run_filter(torch, acc, ids, P, N, rc.ao_filter_params(8, "box"))
    rc.render_ambient(sc, eye, m, W, H, rc.ao_dirs(16), rc.ao_filter_params(3, "tent"),
                      (0.2, 0.3, 0.4), depth=DEPTH)
    rc.render_camera_gbuffer(sc, eye, m, W, H)
    after = others()
    for x, y in zip(before[:3], after[:3]):
        np.testing.assert_array_equal(x, y)
    assert before[3] == after[3]
