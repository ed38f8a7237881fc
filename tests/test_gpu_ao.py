"""Any-hit visibility and ambient occlusion on the GPU (rc_ao_pass_device, rc_ao_resolve_device,
rc_render_ao, rc_occluded_rays*).  Every comparison is exact: records, bytes, counts.
The expectation is tests/ao_cases.py's: the oracle's primary hits and the occlusion rule over the
oracle's shape test, put through the pass's contract in numpy (rc.ao_flip, rc.ao_step, rc.ao_byte).
tests/test_ao.py holds the rule against the oracle's shadow scan and checks that these inputs are
not constant planes."""
import numpy as np
import pytest

import ao_cases as aoc
import ray_cases as rcs
from helpers import rc
from test_gpu_camera import first_sphere_centre

pytestmark = pytest.mark.gpu

F32, I32 = np.float32, np.int32
INF = np.inf
W, H = aoc.SIZE
DEPTH = rcs.DEPTH
GUARD = 64


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


def guarded(torch, nbytes, fill=0x5a):
    raw = torch.full((GUARD + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
    return raw, raw.data_ptr() + GUARD


def unguard(raw):
    a = raw.cpu().numpy()
    assert (a[:GUARD] == 0x5a).all() and (a[-GUARD:] == 0x5a).all(), "guard bytes"
    return a[GUARD:-GUARD].copy()


class State:
    """An occlusion state and its plane in device memory, both filled with 0x5a and with guard
    bytes on either side."""

    def __init__(self, torch, w, h):
        self.torch, self.w, self.h = torch, w, h
        self.raw_ao, self.ao_ptr = guarded(torch, w * h * 4)
        self.raw_out, self.out_ptr = guarded(torch, w * h)
        assert self.ao_ptr % 4 == 0
        torch.cuda.synchronize()

    def preset(self, acc):
        t = self.torch.from_numpy(np.ascontiguousarray(acc).view(np.uint8).reshape(-1).copy())
        self.raw_ao[GUARD:GUARD + self.w * self.h * 4] = t.cuda()
        self.torch.cuda.synchronize()

    def run(self, sc, eye, m, dirs, window=None, reset=False, stream=None, out=True):
        rc.ao_pass_device(sc, eye, m, self.w, self.h, dirs, self.ao_ptr,
                          self.out_ptr if out else None, window=window, reset=reset,
                          stream_ptr=stream.cuda_stream if stream else None, depth=DEPTH)

    def read(self):
        self.torch.cuda.synchronize()
        return (unguard(self.raw_ao).view(rc.AO_DTYPE).reshape(self.h, self.w),
                unguard(self.raw_out).reshape(self.h, self.w))


def check_state(st, acc, tag, out=True):
    got, got_out = st.read()
    np.testing.assert_array_equal(got["rays"], acc["rays"], err_msg=f"rays {tag}")
    np.testing.assert_array_equal(got["open"], acc["open"], err_msg=f"open {tag}")
    if out:
        np.testing.assert_array_equal(got_out, rc.ao_byte(acc), err_msg=f"bytes {tag}")


def expect_pass(acc, name, eye, m, dirs, size=aoc.SIZE, window=None, reset=False):
    """(acc', stats) of one pass by the oracle and the numpy contract."""
    add, hits, blocked = aoc.open_add(name, eye, m, dirs, size, window)
    new, sat = rc.ao_step(acc, add, len(dirs[0]), reset=reset)
    assert sat == 0
    return new, {"hit_pixels": hits, "rays": hits * len(dirs[0]), "blocked": blocked,
                 "saturated": 0}


def zero(w=W, h=H):
    return np.zeros((h, w), rc.AO_DTYPE)


# --------------------------------------------------------- 1. states, stats and bytes --
@pytest.mark.parametrize("tmax", aoc.TMAXES, ids=["inf", "2.0"])
@pytest.mark.parametrize("k", aoc.CAMS)
def test_states_stats_and_bytes(k, tmax, torch):
    name, eye, m = rcs.CAMERAS[k]
    sc = rcs.scene(name)
    for n in (1, 5, 16, 64):
        st = State(torch, W, H)
        first, second = rc.ao_dirs(n, tmax), rc.ao_dirs(n, tmax, aoc.ROT)
        acc, stats = expect_pass(zero(), name, eye, m, first, reset=True)
        st.run(sc, eye, m, first, reset=True)            # over 0x5a records: reset reads nothing
        tag = f"{name} {eye} n{n} tmax {tmax}"
        check_state(st, acc, tag + " pass 1")
        assert rc.ao_stats() == stats, tag
        acc, stats = expect_pass(acc, name, eye, m, second)
        st.run(sc, eye, m, second)
        check_state(st, acc, tag + " pass 2")
        assert rc.ao_stats() == stats, tag
        assert (acc["rays"] == 2 * n).all()
        if n >= 16:
            assert len(np.unique(rc.ao_byte(acc))) > 4, tag    # a plane, not a constant
    assert rc.ao_phase_ms()["ao"] > 0.0


# --------------------------------------------------------------------------- 2. windows --
@pytest.mark.parametrize("tmax", aoc.TMAXES, ids=["inf", "2.0"])
def test_windows(tmax, torch):
    """The window's state is the crop of the whole image's state, device against device and both
    against the oracle."""
    name, eye, m = rcs.CAMERAS[9]
    sc, dirs = rcs.scene(name), rc.ao_dirs(16, tmax)
    fw, fh = aoc.FULL
    whole = State(torch, fw, fh)
    whole.run(sc, eye, m, dirs, reset=True)
    full_acc, full_out = whole.read()
    np.testing.assert_array_equal(full_out, rc.ao_byte(full_acc))
    for window, (w, h) in ((aoc.WINDOW, aoc.SIZE), (aoc.CORNER, aoc.CORNER_SIZE)):
        st = State(torch, w, h)
        st.run(sc, eye, m, dirs, window=window, reset=True)
        want, stats = expect_pass(zero(w, h), name, eye, m, dirs, (w, h), window, reset=True)
        check_state(st, want, f"window {window}")
        assert rc.ao_stats() == stats
        x0, y0 = window[2:]
        np.testing.assert_array_equal(st.read()[0], full_acc[y0:y0 + h, x0:x0 + w])
    assert 0 < (full_acc["open"] < 16).sum() < fw * fh


# ------------------------------------------------------------ 3. device against device --
def test_the_eye_at_zero_and_the_gbuffers_ids(torch):
    """Eye +0 with the identity view and the eye -0 case give the same records; a primary miss
    leaves open = rays = n, on exactly the pixels where rc_render_gbuffer's id is negative."""
    sc, dirs = rcs.scene("reflection"), rc.ao_dirs(16)
    a, b = State(torch, W, H), State(torch, W, H)
    a.run(sc, (0.0, 0.0, 0.0), None, dirs, reset=True)
    stats = rc.ao_stats()
    b.run(sc, (-0.0, -0.0, -0.0), rcs.IDENT, dirs, reset=True)
    assert rc.ao_stats() == stats
    acc = a.read()[0]
    np.testing.assert_array_equal(b.read()[0], acc)
    np.testing.assert_array_equal(b.read()[1], a.read()[1])
    ids = rc.render_gbuffer(sc, W, H, planes=("id",))["id"]
    assert stats["hit_pixels"] == int((ids >= 0).sum()) and 0 < stats["hit_pixels"] < W * H
    assert (acc["open"][ids < 0] == 16).all() and (acc["rays"] == 16).all()
    assert (acc["open"][ids >= 0] < 16).any()
    want, _ = expect_pass(zero(), "reflection", (0.0, 0.0, 0.0), rcs.IDENT, dirs, reset=True)
    np.testing.assert_array_equal(acc, want)


# ------------------------------------------------------------------------ 4. shape counts --
@pytest.mark.parametrize("name", ["random64", "random65"])
def test_scenes_too_large_to_stage(name, torch):
    """More shapes than the LDS copy of the scene holds.  These scenes are enclosed, so nearly
    every unbounded ray is blocked; the bounded ones are mixed on half the pixels (checked on the
    CPU: 0.52 and 0.62)."""
    sc = rcs.scene(name)
    assert sc.num_shapes + 1 > 32
    eye, m = (0.0, 0.0, 5.0), rcs.IDENT
    assert aoc.mixed_share(name, eye, m, rc.ao_dirs(5, 2.0)) > 0.3
    for tmax in aoc.TMAXES:
        dirs = rc.ao_dirs(5, tmax)
        st = State(torch, W, H)
        st.run(sc, eye, m, dirs, reset=True)
        acc, stats = expect_pass(zero(), name, eye, m, dirs, reset=True)
        check_state(st, acc, f"{name} tmax {tmax}")
        assert rc.ao_stats() == stats and stats["hit_pixels"] > 0.3 * W * H


# -------------------------------------------------------------------------- 5. edge inputs --
def test_cross_terms_from_a_shapes_centre(torch):
    name = "random14x"
    sc = rcs.scene(name)
    eye, m = first_sphere_centre(sc.js), rc.view_euler(0.2, 0.1)
    for tmax in aoc.TMAXES:
        dirs = rc.ao_dirs(16, tmax)
        st = State(torch, W, H)
        st.run(sc, eye, m, dirs, reset=True)
        acc, stats = expect_pass(zero(), name, eye, m, dirs, reset=True)
        check_state(st, acc, f"{name} tmax {tmax}")
        assert rc.ao_stats() == stats and stats["blocked"] > 0


def test_tmax_is_in_units_of_the_directions_length(torch):
    name, eye, m = rcs.CAMERAS[9]
    sc = rcs.scene(name)
    u = rc.ao_dirs(16)[0]
    planes = {}
    for scale in (1.0, 3.0, 1e-3):
        dirs = ((u.astype(np.float64) * scale).astype(F32), 2.0)
        st = State(torch, W, H)
        st.run(sc, eye, m, dirs, reset=True)
        acc, stats = expect_pass(zero(), name, eye, m, dirs, reset=True)
        check_state(st, acc, f"scale {scale}")
        assert rc.ao_stats() == stats
        planes[scale] = acc["open"].astype(np.int64)
    # longer directions reach further at the same tmax: never more open rays, somewhere fewer
    assert (planes[3.0] <= planes[1.0]).all() and (planes[3.0] < planes[1.0]).any()
    assert (planes[1e-3] >= planes[1.0]).all() and (planes[1e-3] > planes[1.0]).any()


# --------------------------------------------------------------------------- 6. saturation --
def test_saturation(torch):
    name, eye, m = rcs.CAMERAS[9]
    sc, (w, h) = rcs.scene(name), (9, 5)
    start = zero(w, h)
    start["rays"], start["open"] = rc.AO_MAX_RAYS - 63, 1000
    st = State(torch, w, h)
    st.preset(start)
    d63, d1 = rc.ao_dirs(63), rc.ao_dirs(1)
    add, hits, blocked = aoc.open_add(name, eye, m, d63, (w, h))
    acc, sat = rc.ao_step(start, add, 63)
    assert sat == 0 and (acc["rays"] == rc.AO_MAX_RAYS).all() and 0 < hits
    st.run(sc, eye, m, d63)
    check_state(st, acc, "63 rays to the brim")
    assert rc.ao_stats() == {"hit_pixels": hits, "rays": 63 * hits, "blocked": blocked,
                             "saturated": 0}
    st.raw_out[GUARD:GUARD + w * h] = 0x33          # the refusing pass still stores the bytes
    st.run(sc, eye, m, d1)
    check_state(st, acc, "a saturated state takes no ray")
    assert rc.ao_stats() == {"hit_pixels": 0, "rays": 0, "blocked": 0, "saturated": 45}
    st.run(sc, eye, m, d1, reset=True)              # a reset pass does not read the records
    check_state(st, expect_pass(zero(w, h), name, eye, m, d1, (w, h), reset=True)[0], "reset")


# ------------------------------------------------------------------------------ 7. resolve --
@pytest.mark.parametrize("w", [1, 3, 4, 5, 67])
def test_resolve(w, torch):
    h = 3
    rng = np.random.default_rng(w)
    acc = zero(w, h)
    acc["rays"] = rng.integers(0, 65536, (h, w))
    acc["open"] = (acc["rays"] * rng.random((h, w))).astype(np.uint16)
    acc["rays"][0, 0] = 0
    acc["open"].flat[-1] = acc["rays"].flat[-1] = 65535
    st = State(torch, w, h)
    st.preset(acc)
    rc.ao_resolve_device(st.ao_ptr, w, h, st.out_ptr)
    check_state(st, acc, f"resolve {w} x {h}")
    # an output that starts off a 4-byte boundary, and a state off a 16-byte one
    for off in (1, 2, 3):
        raw, ptr = guarded(torch, w * h + 4)
        rc.ao_resolve_device(st.ao_ptr, w, h, ptr + off)
        torch.cuda.synchronize()
        got = unguard(raw)
        np.testing.assert_array_equal(got[off:off + w * h].reshape(h, w), rc.ao_byte(acc))
        assert (got[:off] == 0x5a).all() and (got[off + w * h:] == 0x5a).all()
    if w * h > 4:
        raw, ptr = guarded(torch, w * h)
        rc.ao_resolve_device(st.ao_ptr + 4, w * h - 1, 1, ptr)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(unguard(raw)[:w * h - 1], rc.ao_byte(acc).ravel()[1:])


# --------------------------------------------------------------------------- 8. ray batches --
def frame_rays(ndirs):
    """k_ao's own rays for camera 9 with ndirs directions."""
    name, eye, m = rcs.CAMERAS[9]
    O, D, skip, px = aoc.hit_rays(name, eye, m, rc.ao_dirs(ndirs)[0])
    return rcs.scene(name), O, D, skip, px


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_ray_batches(n, torch):
    sc, O, D, skip, _ = frame_rays(64)
    first = 1000                                     # past the frame's first rows
    assert len(skip) >= first + 4097
    O, D, skip = O[first:first + n].copy(), D[first:first + n], skip[first:first + n]
    O[n // 2] = (np.nan, 0.0, -5.0)                  # data, not looked at: nothing is blocked
    if n > 3:
        O[1], O[2] = (INF, 0.0, 0.0), (0.0, -INF, 0.0)
    tmax = np.resize(np.array([INF, 2.0, 0.0, -1.0, np.nan, 0.75, -INF], F32), n)
    wild = skip.copy()
    wild[::3] = -1
    wild[1::7] = sc.num_shapes + 5                   # names no shape: skips nothing, z rule on
    wild[5::11] = -7
    rule = lambda s, t: aoc.blocked_rule(sc.js, sc.num_shapes, O, D, s, t).astype(np.uint8)
    none = np.full(n, -1, I32)
    for s, t in ((None, None), (skip, None), (None, tmax), (skip, tmax), (wild, tmax)):
        got = rc.occluded_rays(sc, O, D, skip=s, tmax=t)
        want = rule(none if s is None else s, INF if t is None else t)
        np.testing.assert_array_equal(got, want, err_msg=f"n{n} skip {s is not None} tmax "
                                                         f"{t is not None}")
    assert got[n // 2] == 0
    # the device entry, with guard bytes round the output
    d_o, d_d = torch.from_numpy(O).cuda(), torch.from_numpy(np.ascontiguousarray(D)).cuda()
    d_s, d_t = torch.from_numpy(wild).cuda(), torch.from_numpy(tmax).cuda()
    raw, ptr = guarded(torch, n)
    rc.occluded_rays_device(sc, n, d_o.data_ptr(), d_d.data_ptr(), ptr, d_skip_ptr=d_s.data_ptr(),
                            d_tmax_ptr=d_t.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(unguard(raw), rule(wild, tmax))
    if n == 4097:
        assert 0 < rule(skip, INF).sum() < n and 0 < rule(skip, tmax).sum() < rule(skip, INF).sum()


def test_the_batch_on_the_passes_own_rays_is_its_count(torch):
    sc, O, D, skip, px = frame_rays(16)
    name, eye, m = rcs.CAMERAS[9]
    for tmax in aoc.TMAXES:
        st = State(torch, W, H)
        st.run(sc, eye, m, rc.ao_dirs(16, tmax), reset=True, out=False)
        acc = st.read()[0]
        t = None if tmax == INF else np.full(len(skip), tmax, F32)
        blocked = rc.occluded_rays(sc, O, D, skip=skip, tmax=t)
        want = np.full(W * H, 16, np.int64)
        np.subtract.at(want, px, blocked.astype(np.int64))
        np.testing.assert_array_equal(acc["open"].ravel(), want)
        assert rc.ao_stats()["blocked"] == int(blocked.sum())
        assert (st.read()[1] == 0x5a).all()          # no plane was asked for


# ------------------------------------------------------------------- 9. the wider system --
def test_two_states_on_two_streams(torch):
    (na, ea, ma), (nb, eb, mb) = rcs.CAMERAS[9], rcs.CAMERAS[3]
    da, db = rc.ao_dirs(16), rc.ao_dirs(5, 2.0)
    a, b = State(torch, W, H), State(torch, W, H)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    acc_a, acc_b = zero(), zero()
    for k in range(3):
        rot = None if k == 0 else rc.view_euler(0.3 * k, 0.1 * k)
        da_k, db_k = rc.ao_dirs(16, INF, rot), rc.ao_dirs(5, 2.0, rot)
        a.run(rcs.scene(na), ea, ma, da_k, reset=k == 0, stream=s1)
        b.run(rcs.scene(nb), eb, mb, db_k, reset=k == 0, stream=s2)
        acc_a, _ = expect_pass(acc_a, na, ea, ma, da_k, reset=k == 0)
        acc_b, stats_b = expect_pass(acc_b, nb, eb, mb, db_k, reset=k == 0)
    s1.synchronize()
    s2.synchronize()
    assert rc.ao_stats() == stats_b                   # the last pass enqueued
    check_state(a, acc_a, "stream 1")
    check_state(b, acc_b, "stream 2")
    assert da[0].shape == (16, 3) and db[1] == 2.0


def test_the_host_form_with_three_sets_through_a_window(torch):
    name, eye, m = rcs.CAMERAS[14]
    sc, (w, h) = rcs.scene(name), aoc.SIZE
    sets = [rc.ao_dirs(16, 2.0), rc.ao_dirs(5, INF, aoc.ROT), rc.ao_dirs(64, 2.0, aoc.ROT)]
    acc = zero()
    for k, dirs in enumerate(sets):
        acc, stats = expect_pass(acc, name, eye, m, dirs, (w, h), aoc.WINDOW, reset=k == 0)
    timing = {}
    got = rc.render_ao(sc, eye, m, w, h, sets, window=aoc.WINDOW, depth=DEPTH, timing=timing)
    np.testing.assert_array_equal(got, rc.ao_byte(acc))
    assert rc.ao_stats() == stats and (acc["rays"] == 85).all()
    assert timing["kernel_ms"] > 0.0 and rc.ao_phase_ms()["ao"] > 0.0
    one = rc.render_ao(sc, eye, m, w, h, sets[0], window=aoc.WINDOW, depth=DEPTH)
    first = expect_pass(zero(), name, eye, m, sets[0], (w, h), aoc.WINDOW, reset=True)[0]
    np.testing.assert_array_equal(one, rc.ao_byte(first))


def test_refusals_leave_live_buffers_alone(torch):
    name, eye, m = rcs.CAMERAS[9]
    sc, dirs = rcs.scene(name), rc.ao_dirs(16)
    st = State(torch, W, H)
    st.run(sc, eye, m, dirs, reset=True)
    acc, out = st.read()
    stats = rc.ao_stats()
    bad = [dict(mode="parity"), dict(mode="cuda"), dict(window=(64, 48, 60, 0)),
           dict(dirs=(dirs[0], 0.0)), dict(dirs=(np.zeros((4, 3), F32), INF)),
           dict(eye=(np.nan, 0.0, 0.0))]
    for kw in bad:
        args = dict(eye=eye, dirs=dirs, window=None, mode="fast")
        args.update(kw)
        with pytest.raises(RuntimeError):
            rc.ao_pass_device(sc, args["eye"], m, W, H, args["dirs"], st.ao_ptr, st.out_ptr,
                              window=args["window"], mode=args["mode"], depth=DEPTH)
    with pytest.raises(RuntimeError):
        rc.ao_pass_device(sc, eye, m, W, H, dirs, st.ao_ptr + 2, st.out_ptr, depth=DEPTH)
    with pytest.raises(RuntimeError):
        rc.ao_resolve_device(st.ao_ptr + 1, W, H, st.out_ptr)
    with pytest.raises(RuntimeError):
        rc.occluded_rays(sc, np.zeros((4, 3), F32), np.ones((4, 3), F32), mode="cuda")
    got, got_out = st.read()
    np.testing.assert_array_equal(got, acc)
    np.testing.assert_array_equal(got_out, out)
    assert rc.ao_stats() == stats


def test_the_other_kernels_bytes_before_and_after(torch):
    """k_camera's image and the window accumulation's records and bytes do not move when occlusion
    passes run in between."""
    name, eye, m = rcs.CAMERAS[9]
    sc = rcs.scene(name)

    def others():
        img = rc.render_camera(sc, eye, m, W, H, depth=DEPTH)
        d_acc = torch.zeros((H * W * 8,), dtype=torch.uint8, device="cuda")
        d_out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        rc.accum_pass_window_device(sc, aoc.WINDOW, W, H, "hier4", 0, 5, d_acc.data_ptr(),
                                    d_out.data_ptr(), reset=True, depth=DEPTH)
        torch.cuda.synchronize()
        return img, d_acc.cpu().numpy(), d_out.cpu().numpy(), rc.accum_stats()

    before = others()
    np.testing.assert_array_equal(before[0], rcs.camera_image(name, eye, m, 1, aoc.SIZE))
    st = State(torch, W, H)
    st.run(sc, eye, m, rc.ao_dirs(64, 2.0), reset=True)
    rc.render_ao(sc, eye, m, W, H, rc.ao_dirs(16), depth=DEPTH)
    rc.occluded_rays(sc, np.zeros((65, 3), F32), np.ones((65, 3), F32))
    after = others()
    for x, y in zip(before[:3], after[:3]):
        np.testing.assert_array_equal(x, y)
    assert before[3] == after[3]
