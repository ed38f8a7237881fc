"""The primary-visibility G-buffer without a GPU: the numpy contract of the id-edge
rate map against a plain double loop, every refusal of the new entry points (one line on stderr
that names the entry point, -1, from the arguments alone: none of these calls reaches a HIP call),
the structures' sizes and the Python-side argument errors.  The expected lines are written here;
a call that breaks two rules prints the first clause's."""
import ctypes
import itertools

import numpy as np
import pytest

from helpers import rc, scene_path
from test_refusals import FAKE, O, S, WIN, captured, ref, scene

ODD = FAKE + 4     # a non-null "device pointer" that is not 16-byte aligned


# ------------------------------------------------------------------ the edge map --
def edge_rates_loop(ids, s, base):
    """rc_id_edge_rates_device's contract, pixel by pixel."""
    h, w = ids.shape
    out = np.empty((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            edge = False
            for yy in range(max(y - 1, 0), min(y + 2, h)):
                for xx in range(max(x - 1, 0), min(x + 2, w)):
                    edge = edge or ids[yy, xx] != ids[y, x]
            out[y, x] = s if edge else base
    return out


EDGE_SHAPES = [(1, 1), (1, 9), (9, 1), (17, 33)]


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_id_edge_rates_against_loop(shape):
    rng = np.random.default_rng(2200 + shape[0] * 100 + shape[1])
    noise = rng.integers(-1, 4, shape).astype(np.int32)
    # the same values in blocks of 4 x 4, so that pixels with a constant neighbourhood occur too
    blocks = np.kron(rng.integers(-1, 4, ((shape[0] + 3) // 4, (shape[1] + 3) // 4)),
                     np.ones((4, 4), np.int64))[:shape[0], :shape[1]].astype(np.int32)
    for ids in (noise, blocks):
        for s, base in itertools.product((2, 4, 8), (0, 1)):
            got = rc.id_edge_rates(ids, s, base)
            assert got.dtype == np.uint8 and got.shape == shape
            np.testing.assert_array_equal(got, edge_rates_loop(ids, s, base))
    if shape == (17, 33):                  # the inputs are not vacuous: both values occur
        assert len(np.unique(rc.id_edge_rates(blocks, 4, 1))) == 2


@pytest.mark.parametrize("shape", EDGE_SHAPES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_id_edge_rates_constant_and_checkerboard(shape):
    y, x = np.indices(shape)
    for s, base in itertools.product((2, 4, 8), (0, 1)):
        for v in (-1, 0, 3):
            assert np.all(rc.id_edge_rates(np.full(shape, v, np.int32), s, base) == base)
        assert np.all(rc.id_edge_rates(((x + y) & 1).astype(np.int32), s, base) == s)
    assert np.all(rc.id_edge_rates(np.full((1, 1), 2, np.int32), 8, 0) == 0)


def test_id_edge_rates_argument_errors():
    ids = np.zeros((4, 4), np.int32)
    for bad in (ids.astype(np.int64), ids.ravel(), np.zeros((0, 4), np.int32)):
        with pytest.raises(ValueError, match="id_edge_rates"):
            rc.id_edge_rates(bad, 4)
    for s, base in ((3, 1), (1, 1), (16, 0), (4, 2), (4, -1)):
        with pytest.raises(ValueError, match="id_edge_rates"):
            rc.id_edge_rates(ids, s, base)


# ---------------------------------------------------------------------- refusals --
def G(**planes):
    return rc.RcGbuffer(**planes)


ID_T = G(id=FAKE, t=FAKE)
ALL4 = G(id=FAKE, t=FAKE, P=FAKE, N=FAKE)
W64 = WIN(64, 48, 8, 4)
SSAA_MSG = ("ssaa {v} in the options: a G-buffer of the s x s image is a window of the s*full_w x "
            "s*full_h image, leave ssaa at 0 or 1")
THR_MSG = ("ssaa {v} carries an adaptive threshold: a G-buffer holds one primary hit a pixel; the "
           "planes of the s x s image are a window of the s*full_w x s*full_h image")
CUDA_MSG = ("the hit point and the normal (P, N, frame = 1) are for fast and parity mode: no "
            "reference pins the CUDA port's hit frame; ask for id and t")
ADAPT = rc.ssaa_adaptive(4, 16)

# (id, the arguments behind (scene, ...) of both plane entries, the message behind "Error: <who>: ")
PLANE_REFUSALS = [
    ("null_scene", (None, None, 16, 16, ref(O()), ref(ID_T)), "a null pointer"),
    ("null_options", (S, None, 16, 16, None, ref(ID_T)), "a null pointer"),
    ("null_planes", (S, None, 16, 16, ref(O()), None), "a null pointer"),
    ("no_plane", (S, None, 16, 16, ref(O()), ref(G())),
     "all four planes are null: ask for at least one of id, t, P and N"),
    ("ssaa3", (S, None, 16, 16, ref(O(ssaa=3)), ref(ID_T)), None),      # ssaa_decode's own line
    ("ssaa2", (S, None, 16, 16, ref(O(ssaa=2)), ref(ID_T)), SSAA_MSG.format(v=2)),
    ("ssaa8_parity", (S, None, 16, 16, ref(O("parity", ssaa=8)), ref(ID_T)), SSAA_MSG.format(v=8)),
    ("adaptive", (S, None, 16, 16, ref(O(ssaa=4, adaptive=16)), ref(ID_T)),
     THR_MSG.format(v=ADAPT)),
    ("gpus2", (S, None, 16, 16, ref(O(gpus=2)), ref(ID_T)),
     "num_gpus 2: the row shards render no G-buffer"),
    ("cuda_P", (S, None, 16, 16, ref(O("cuda")), ref(G(id=FAKE, P=FAKE))), CUDA_MSG),
    ("cuda_N", (S, None, 16, 16, ref(O("cuda")), ref(G(N=FAKE))), CUDA_MSG),
    ("two_no_plane_ssaa2", (S, None, 16, 16, ref(O(ssaa=2)), ref(G())),
     "all four planes are null: ask for at least one of id, t, P and N"),
    ("two_ssaa2_gpus2", (S, None, 16, 16, ref(O(ssaa=2, gpus=2)), ref(ID_T)), SSAA_MSG.format(v=2)),
    ("two_gpus2_cuda_P", (S, None, 16, 16, ref(O("cuda", gpus=2)), ref(ALL4)),
     "num_gpus 2: the row shards render no G-buffer"),
    ("two_cuda_P_window", (S, ref(WIN(64, 48, 60, 4)), 16, 16, ref(O("cuda")), ref(ALL4)), CUDA_MSG),
]
# what rc_window_check refuses is rc_window_check's own line
WINDOW_REFUSALS = [
    ("w0", (S, None, 0, 16, ref(O()), ref(ID_T)),
     "a 0 x 16 window of a 0 x 16 image: every size must be at least 1"),
    ("h_neg_parity", (S, None, 16, -1, ref(O("parity")), ref(ALL4)),
     "a 16 x -1 window of a 16 x -1 image: every size must be at least 1"),
    ("outside", (S, ref(WIN(64, 48, 60, 4)), 16, 16, ref(O()), ref(ID_T)),
     "a 16 x 16 window at (60, 4) reaches outside the 64 x 48 image"),
    ("x0_neg", (S, ref(WIN(64, 48, -1, 0)), 16, 16, ref(O("cuda")), ref(ID_T)),
     "origin (-1, 0): a window starts inside the image, at 0 or above"),
    ("grid_rows", (S, None, 16, 1 << 22, ref(O()), ref(ID_T)),
     "a 16 x 4194304 window at factor 1 is too large for the kernel's grid (at most 65535 rows of "
     "16-subsample tiles, 2^31 - 1 tiles)"),
]


def refused_line(export, args):
    args = [scene() if a is S else a for a in args]
    code, err = captured(lambda: getattr(rc.hip_lib(), export)(*args))
    assert code == -1, (export, code, err)
    assert err.endswith("\n") and err.count("\n") == 1, err         # exactly one line
    return err[:-1]


@pytest.mark.parametrize("export", ["rc_render_gbuffer", "rc_render_gbuffer_device"])
@pytest.mark.parametrize("cid,args,msg", PLANE_REFUSALS, ids=[c[0] for c in PLANE_REFUSALS])
def test_plane_refusals(export, cid, args, msg):
    tail = (None,) if export == "rc_render_gbuffer" else (None, None)
    line = refused_line(export, args + tail)
    if msg is None:
        assert export in line and "ssaa 3" in line
    else:
        assert line == f"Error: {export}: {msg}"


@pytest.mark.parametrize("export", ["rc_render_gbuffer", "rc_render_gbuffer_device"])
@pytest.mark.parametrize("cid,args,msg", WINDOW_REFUSALS, ids=[c[0] for c in WINDOW_REFUSALS])
def test_plane_window_refusals(export, cid, args, msg):
    tail = (None,) if export == "rc_render_gbuffer" else (None, None)
    assert refused_line(export, args + tail) == f"Error: rc_window_check: {msg}"


_XY = np.array([[0, 0], [63, 47], [5, 3], [5, 3]], np.int32)
_HITS = np.zeros(4, rc.HIT_DTYPE)
XY, HITS = _XY.ctypes.data, _HITS.ctypes.data
# (id, full_w, full_h, options, frame, n, xy, hits, message); `H`: the host entry only
PICK_REFUSALS = [
    ("null_xy", 64, 48, O(), 0, 4, None, HITS, "a null pointer"),
    ("null_hits", 64, 48, O(), 0, 4, XY, None, "a null pointer"),
    ("null_options", 64, 48, None, 0, 4, XY, HITS, "a null pointer"),
    ("ssaa2", 64, 48, O(ssaa=2), 0, 4, XY, HITS, SSAA_MSG.format(v=2)),
    ("adaptive", 64, 48, O("cuda", ssaa=4, adaptive=16), 0, 4, XY, HITS, THR_MSG.format(v=ADAPT)),
    ("gpus2", 64, 48, O("parity", gpus=2), 0, 4, XY, HITS,
     "num_gpus 2: the row shards render no G-buffer"),
    ("cuda_frame", 64, 48, O("cuda"), 1, 4, XY, HITS, CUDA_MSG),
    ("full_w0", 0, 48, O(), 0, 4, XY, HITS, "a 0 x 48 image: both sides must be at least 1"),
    ("full_h_neg", 64, -3, O(), 1, 4, XY, HITS, "a 64 x -3 image: both sides must be at least 1"),
    ("n0", 64, 48, O(), 0, 0, XY, HITS, "n 0 is not 1 .. 2^24 points"),
    ("n_neg", 64, 48, O(), 0, -1, XY, HITS, "n -1 is not 1 .. 2^24 points"),
    ("n_past", 64, 48, O(), 0, (1 << 24) + 1, XY, HITS, "n 16777217 is not 1 .. 2^24 points"),
    ("two_cuda_frame_n0", 64, 48, O("cuda"), 1, 0, XY, HITS, CUDA_MSG),
    ("two_image_n0", 64, 0, O(), 0, 0, XY, HITS, "a 64 x 0 image: both sides must be at least 1"),
]


@pytest.mark.parametrize("export", ["rc_pick", "rc_pick_device"])
@pytest.mark.parametrize("case", PICK_REFUSALS, ids=[c[0] for c in PICK_REFUSALS])
def test_pick_refusals(export, case):
    _, fw, fh, opt, frame, n, xy, hits, msg = case
    dev = export == "rc_pick_device"
    # the device entry never follows its pointers when it refuses: FAKE stands for both arrays
    args = [S, fw, fh, ref(opt), frame, n, xy and (FAKE if dev else xy),
            hits and (FAKE if dev else hits)] + ([None] if dev else [])
    assert refused_line(export, args) == f"Error: {export}: {msg}"
    assert not _HITS.view(np.uint8).any()


def test_pick_device_unaligned_records():
    args = [S, 64, 48, ref(O()), 0, 4, FAKE, ODD, None]
    assert refused_line("rc_pick_device", args) == \
        "Error: rc_pick_device: the records are not 16-byte aligned"
    # in front of the options' clauses
    args[3] = ref(O(ssaa=2))
    assert refused_line("rc_pick_device", args) == \
        "Error: rc_pick_device: the records are not 16-byte aligned"


@pytest.mark.parametrize("k,pt", [(0, (-1, 0)), (1, (64, 0)), (2, (0, 48)), (3, (3, -2147483648))])
def test_pick_refuses_a_point_outside(k, pt):
    xy = _XY.copy()
    xy[k] = pt
    hits = np.full(4, 7, np.uint8).repeat(32).view(rc.HIT_DTYPE)     # a sentinel in every byte
    line = refused_line("rc_pick", [S, 64, 48, ref(O()), 1, 4, xy.ctypes.data, hits.ctypes.data])
    assert line == f"Error: rc_pick: point {k} at ({pt[0]}, {pt[1]}) is outside the 64 x 48 image"
    assert np.all(hits.view(np.uint8) == 7)                          # hits untouched
    with pytest.raises(RuntimeError, match="rc_pick failed"):
        rc.pick(rc.Scene.from_file(scene_path("simple")), 64, 48, xy)


EDGE_REFUSALS = [
    ("null_id", (None, 16, 16, 4, 1, FAKE, None), "a null pointer"),
    ("null_rates", (FAKE, 16, 16, 4, 1, None, None), "a null pointer"),
    ("s3", (FAKE, 16, 16, 3, 1, FAKE, None), "s 3 is not 2, 4 or 8"),
    ("s1", (FAKE, 16, 16, 1, 1, FAKE, None), "s 1 is not 2, 4 or 8"),
    ("s16", (FAKE, 16, 16, 16, 0, FAKE, None), "s 16 is not 2, 4 or 8"),
    ("base2", (FAKE, 16, 16, 4, 2, FAKE, None), "base 2 is not 0 or 1"),
    ("base_neg", (FAKE, 16, 16, 8, -1, FAKE, None), "base -1 is not 0 or 1"),
    ("w0", (FAKE, 0, 16, 4, 1, FAKE, None), "0 x 16: both sides must be at least 1"),
    ("h_neg", (FAKE, 16, -2, 2, 0, FAKE, None), "16 x -2: both sides must be at least 1"),
    ("too_large", (FAKE, 65536, 65536, 4, 1, FAKE, None),
     "65536 x 65536 is too large (32-bit pixel indices)"),
    ("two_s_base", (FAKE, 16, 16, 5, 7, FAKE, None), "s 5 is not 2, 4 or 8"),
    ("two_base_size", (FAKE, 0, 0, 4, 3, FAKE, None), "base 3 is not 0 or 1"),
]


@pytest.mark.parametrize("cid,args,msg", EDGE_REFUSALS, ids=[c[0] for c in EDGE_REFUSALS])
def test_edge_map_refusals(cid, args, msg):
    assert refused_line("rc_id_edge_rates_device", list(args)) == \
        f"Error: rc_id_edge_rates_device: {msg}"


def test_phase_ms_refuses_null():
    assert rc.hip_lib().rc_gbuffer_phase_ms(None) == -1


# ------------------------------------------------ structures and Python arguments --
def test_structure_sizes_and_exports():
    assert ctypes.sizeof(rc.RcGbuffer) == 32 and ctypes.sizeof(rc.RcHit) == 32
    assert rc.HIT_DTYPE.itemsize == 32
    assert [rc.HIT_DTYPE.fields[n][1] for n in ("id", "t", "P", "N")] == [0, 4, 8, 20]
    assert [getattr(rc.RcHit, n).offset for n in ("id", "t", "P", "N")] == [0, 4, 8, 20]
    for name in ("rc_render_gbuffer", "rc_render_gbuffer_device", "rc_pick", "rc_pick_device",
                 "rc_id_edge_rates_device", "rc_gbuffer_phase_ms"):
        assert name in rc.HIP_EXPORTS and hasattr(rc.hip_lib(), name), name


def test_python_argument_errors():
    sc = rc.Scene.from_file(scene_path("simple"))
    with pytest.raises(ValueError, match="plane 'depth'"):
        rc.render_gbuffer(sc, 8, 8, planes=("id", "depth"))
    with pytest.raises(ValueError, match="no plane"):
        rc.render_gbuffer(sc, 8, 8, planes=())
    for bad in (np.zeros(4, np.int32), np.zeros((2, 3), np.int32), np.zeros((2, 2), np.float32),
                np.zeros((0, 2), np.int32), np.array([[0, 2 ** 31]], np.int64)):
        with pytest.raises(ValueError, match="pick"):
            rc.pick(sc, 8, 8, bad)
