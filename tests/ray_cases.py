"""Rays with origins: the expectation of tests/test_camera.py and tests/test_gpu_camera.py
(DESIGN.md §24).  The oracle exports its scan for any origin (rco_prim_nearest) and its shade for any
hit (rco_prim_shade) but its bounce loop only from the origin (rco_prim_shoot), so ref_trace_from
states the fast-mode loop between the two exports in float32 numpy, operation for operation
(oracle/rc_oracle.c o_shoot, o_reflect, o_normalize).  tests/test_camera.py holds it against
rco_prim_shoot at O = 0 bit for bit, which validates the restatement itself.  References are
computed once per key and are read-only."""
import ctypes

import numpy as np

import prim_cases as pc
import shade_cases as shc
import view_cases as vc
from helpers import rc

F32, F64, I32 = np.float32, np.float64, np.int32


def reflectivities(js):
    """The reflectivity of every shape of a json_data_t's shape list, in list order."""
    out, p = [], js.shapes_list
    while p:
        out.append(p.contents.reflectivity)
        p = ctypes.cast(p.contents.next, ctypes.POINTER(rc.ShapeT))
    return np.array(out, F32)


def dot(a, b):
    """o_dot: (a0 b0 + a1 b1) + a2 b2 in float."""
    s = a[:, 0] * b[:, 0]
    s = s + a[:, 1] * b[:, 1]
    return s + a[:, 2] * b[:, 2]


def reflect(v, n):
    """o_reflect: v - n * (2 dot(v, n)), every operation a float one."""
    s = (F32(2.0) * dot(v, n))[:, None]
    return (v - n * s).astype(F32)


def normalize(a):
    """o_normalize: the length is (float)sqrt of the double sum of squares; a zero length leaves
    the vector as it is."""
    d = a.astype(F64)
    s = d[:, 0] * d[:, 0]
    s = s + d[:, 1] * d[:, 1]
    s = s + d[:, 2] * d[:, 2]
    ln = np.sqrt(s).astype(F32)
    zero = ln == 0.0
    out = (a / np.where(zero, F32(1.0), ln)[:, None]).astype(F32)
    out[zero] = a[zero]
    return out


def ref_trace_from(js, O, D, maxrec):
    """(rgb [n, 3] float32, id [n], t [n], P [n, 3], N [n, 3]) of the fast-mode bounce loop for the
    rays (O, D), maxrec = max_recursion: id, t, P, N are the primary hit's (rco_prim_nearest(O, D,
    skip = -1); id -1 and zeros for a miss), rgb the colour before quantisation."""
    O = np.ascontiguousarray(O, F32).reshape(-1, 3)
    D = np.ascontiguousarray(D, F32).reshape(-1, 3)
    n = len(D)
    assert len(O) == n
    refl = reflectivities(js)
    with np.errstate(all="ignore"):
        i0, t0, P0, N0, _ = pc.ref_nearest(js, O, D, np.full(n, -1, I32))
        hit = i0 >= 0
        out = np.zeros((n, 3), F32)
        live = np.flatnonzero(hit)                  # rays still in the loop
        obj = i0[live].copy()
        S = obj.copy()
        Oc, Dc, Nc = P0[live].copy(), D[live].copy(), N0[live].copy()
        T = refl[obj]
        for _ in range(1, maxrec):
            keep = refl[obj] > 0
            live, obj, S, Oc, Dc, Nc, T = (a[keep] for a in (live, obj, S, Oc, Dc, Nc, T))
            if not len(live):
                break
            Dc = normalize(reflect(Dc, Nc))
            i, _, P, N, _ = pc.ref_nearest(js, np.ascontiguousarray(Oc), np.ascontiguousarray(Dc),
                                           np.ascontiguousarray(S, I32))
            keep = i >= 0                           # a miss ends the loop
            live, Dc, T = live[keep], Dc[keep], T[keep]
            i, P, N = i[keep], np.ascontiguousarray(P[keep]), np.ascontiguousarray(N[keep])
            if not len(live):
                break
            col, _, _ = shc.ref_shade(js, np.ascontiguousarray(i, I32), P, N,
                                      np.ascontiguousarray(Dc))
            out[live] = out[live] + (col * T[:, None]).astype(F32)
            T = (T * refl[i]).astype(F32)
            obj, S, Oc, Nc = i, i.copy(), P, N
        idx = np.flatnonzero(hit)
        if len(idx):
            prim, _, _ = shc.ref_shade(js, np.ascontiguousarray(i0[idx], I32),
                                       np.ascontiguousarray(P0[idx]), np.ascontiguousarray(N0[idx]),
                                       np.ascontiguousarray(D[idx]))
            out[idx] = out[idx] + prim
    ids = np.where(hit, i0, -1).astype(I32)
    t = np.where(hit, t0, F32(0.0)).astype(F32)
    P = np.where(hit[:, None], P0, F32(0.0)).astype(F32)
    N = np.where(hit[:, None], N0, F32(0.0)).astype(F32)
    return out, ids, t, P, N


def hits_records(ids, t, P, N, frame):
    """ref_trace_from's primary hits as HIT_DTYPE records in rc_hit's conventions (a miss: id -1
    and +0 everywhere; P and N +0 without frame)."""
    hits = np.zeros(len(ids), rc.HIT_DTYPE)
    hits["id"], hits["t"] = ids, t
    if frame:
        hits["P"], hits["N"] = P, N
    return hits


# ------------------------------------------------------------------------------ cameras --
PI = np.pi
IDENT = rc.view_identity()
# (scene, eye, view): DESIGN.md §24's table.  Checked on the CPU: every case has at least 30 %
# primary hits and, but for the far eye (1e4, 0, 0), a bounce that changes some pixel.
CAMERAS = [
    ("reflection", (2.0, 1.0, 3.0), IDENT),
    ("reflection", (0.0, -4.0, -12.5), IDENT),                   # inside a sphere
    ("reflection", (0.0, -5.0, -6.0), IDENT),                    # on the plane: num == 0
    ("reflection", (-3.0, -4.0, -17.0), IDENT),                  # on a sphere's surface
    ("reflection", (0.0, 20.0, -12.0), rc.view_euler(0.0, -PI / 2)),
    ("reflection", (0.0, -4.0, -30.0), rc.view_euler(PI, 0.0)),
    ("reflection", (1e4, 0.0, 0.0), rc.view_euler(PI / 2, 0.0)),
    ("reflection", (-0.0, -0.0, -0.0), IDENT),
    ("quadric", (0.5, 0.25, 1.0), IDENT),
    ("quadric", (0.0, -1.0, 0.0), IDENT),                        # on the plane
    ("quadric", (4.0, 0.0, -7.0), IDENT),                        # the sphere's centre
    ("quadric", (2.0, 3.0, -8.0), rc.view_euler(0.4, -0.5, 0.2)),   # inside a quadric
    ("quadric", (0.0, 0.0, -20.0), rc.view_euler(PI, 0.0)),
    ("simple", (1.0, 0.5, 2.0), rc.view_euler(0.2, 0.1)),
    ("example3", (1.0, 0.5, 2.0), rc.view_euler(0.2, 0.1)),
    ("quadric2", (1.0, 0.5, 2.0), rc.view_euler(0.2, 0.1)),
]
NO_BOUNCE = {6}        # CAMERAS[6]: the far eye sees the scene edge-on, nothing bounces
SIZE = (64, 48)
DEPTH = 6

_scenes = {}


def scene(name):
    """A scene of shade_cases.lit_scenes() or of view_cases, loaded once."""
    if name not in _scenes:
        lit = shc.lit_scenes()
        _scenes[name] = lit[name] if name in lit else vc.scene(name)
    return _scenes[name]


def camera_dirs(sc, m, full, xy):
    return rc.view_dirs(sc.js.camera_width, sc.js.camera_height, full, xy, m)


_REF = {}


def camera_samples(name, eye, m, s=1, size=SIZE, window=None, depth=DEPTH):
    """(rgb8 [s*h, s*w, 3] of the oracle's samples, rgb float, ids) for the camera (eye, m) at
    factor s: the whole size image, or the size window at window = (full_w, full_h, x0, y0)."""
    key = (name, tuple(np.asarray(eye, F32).view(np.uint32).tolist()), np.asarray(m, F32).tobytes(),
           s, size, window, depth)
    if key not in _REF:
        sc = scene(name)
        w, h = size
        fw, fh, x0, y0 = window if window else (w, h, 0, 0)
        d = camera_dirs(sc, m, (s * fw, s * fh), rc.view_grid(s * w, s * h, s * x0, s * y0))
        O = np.tile(np.asarray(eye, F32), (len(d), 1))
        rgb, ids, _, _, _ = ref_trace_from(sc.js, O, d, depth + 1)
        px = vc.oracle_quant(rgb).reshape(s * h, s * w, 3)
        for a in (px, rgb, ids):
            a.setflags(write=False)
        _REF[key] = (px, rgb, ids)
    return _REF[key]


def camera_image(name, eye, m, s=1, size=SIZE, window=None, depth=DEPTH):
    """The expected image: the integer box filter of the oracle's s*w x s*h samples."""
    return rc.box_downsample(camera_samples(name, eye, m, s, size, window, depth)[0], s)


def bounce_changes(name, eye, m, size=SIZE):
    """The share of rays whose colour the bounce loop changes (depth DEPTH against depth 0)."""
    with_b = camera_samples(name, eye, m, 1, size)[1]
    without = camera_samples(name, eye, m, 1, size, None, 0)[1]
    return float((with_b.view(np.uint32) != without.view(np.uint32)).any(axis=1).mean())
