"""Any-hit visibility and ambient occlusion: the expectation of tests/test_ao.py and
tests/test_gpu_ao.py, taken from the oracle.  Primary hits are
ray_cases.ref_trace_from's at maxrec = 1 (rco_prim_nearest(eye, d, skip = -1) and its frame);
occlusion is the contract's rule stated over the oracle's shape test (prim_cases.ref_shape), shape
by shape:
    blocked = any over k != skip of (hit_k and t_k > 0 and t_k < tmax).
tests/test_ao.py holds the rule at tmax = inf against the oracle's own shadow scan
(ref_nearest(shadow = True)) for every ray used here.  References are computed once per key and are
read-only."""
import numpy as np

import prim_cases as pc
import ray_cases as rcs
from helpers import rc

F32, I32 = np.float32, np.int32
INF = np.inf

SIZE = (33, 17)                      # no multiple of the 8 x 8 wave block, more than one tile
CAMS = (0, 1, 3, 9, 14)              # of ray_cases.CAMERAS
FULL, WINDOW = (64, 48), (64, 48, 5, 3)         # SIZE at (5, 3) of 64 x 48
CORNER, CORNER_SIZE = (64, 48, 57, 45), (7, 3)  # the 7 x 3 window in its corner
TMAXES = (INF, 2.0)
ROT = rc.view_euler(0.7, 0.3, 0.2)   # the second pass's set is the first one rotated


def blocked_rule(js, nshapes, O, D, skip, tmax):
    """The occlusion rule for the rays (O, D, skip, tmax), [n] bool; tmax a scalar or [n]."""
    O = np.ascontiguousarray(O, F32).reshape(-1, 3)
    D = np.ascontiguousarray(D, F32).reshape(-1, 3)
    skip = np.ascontiguousarray(skip, I32)
    tmax = np.broadcast_to(np.asarray(tmax, F32), skip.shape)
    out = np.zeros(len(skip), bool)
    with np.errstate(all="ignore"):
        for k in range(nshapes):
            hit, t, _ = pc.ref_shape(js, O, D, np.full(len(skip), k, I32), skip)
            out |= (hit != 0) & (skip != k) & (t > 0) & (t < tmax)
    return out


_PRIMARY, _OPEN = {}, {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def primary(name, eye, m, size=SIZE, window=None):
    """(ids [h, w], P [h, w, 3], N [h, w, 3]) of the camera's primary hits (id -1: a miss)."""
    key = (name, np.asarray(eye, F32).tobytes(), np.asarray(m, F32).tobytes(), size, window)
    if key not in _PRIMARY:
        sc, (w, h) = rcs.scene(name), size
        fw, fh, x0, y0 = window if window else (w, h, 0, 0)
        d = rcs.camera_dirs(sc, m, (fw, fh), rc.view_grid(w, h, x0, y0))
        O = np.tile(np.asarray(eye, F32), (len(d), 1))
        _, ids, _, P, N = rcs.ref_trace_from(sc.js, O, d, 1)
        _PRIMARY[key] = _frozen(ids.reshape(h, w), P.reshape(h, w, 3), N.reshape(h, w, 3))
    return _PRIMARY[key]


def hit_rays(name, eye, m, u, size=SIZE, window=None):
    """The pass's occlusion rays: (O, D, skip, pixel index), one for every hit pixel and direction,
    in pixel order and within a pixel in the set's order."""
    ids, P, N = primary(name, eye, m, size, window)
    px = np.flatnonzero(ids.ravel() >= 0)
    u = np.asarray(u, F32)
    D = rc.ao_flip(N.reshape(-1, 3)[px], u).reshape(-1, 3)
    O = np.repeat(P.reshape(-1, 3)[px], len(u), axis=0)
    return O, D, np.repeat(ids.ravel()[px], len(u)).astype(I32), np.repeat(px, len(u))


def open_add(name, eye, m, dirs, size=SIZE, window=None):
    """(open_add [h, w], hit pixels, blocked rays) of one pass with the set dirs = (u, tmax)."""
    u, tmax = np.asarray(dirs[0], F32), float(dirs[1])
    key = (name, np.asarray(eye, F32).tobytes(), np.asarray(m, F32).tobytes(), size, window,
           u.tobytes(), tmax)
    if key not in _OPEN:
        sc, (w, h) = rcs.scene(name), size
        ids = primary(name, eye, m, size, window)[0]
        O, D, skip, px = hit_rays(name, eye, m, u, size, window)
        blocked = blocked_rule(sc.js, sc.num_shapes, O, D, skip, tmax)
        add = np.full(w * h, len(u), np.int64)
        np.subtract.at(add, px, blocked.astype(np.int64))
        _OPEN[key] = _frozen(add.reshape(h, w)) + (int((ids >= 0).sum()), int(blocked.sum()))
    return _OPEN[key]


def mixed_share(name, eye, m, dirs, size=SIZE):
    """The share of the hit pixels with 0 < open < n."""
    add, hits, _ = open_add(name, eye, m, dirs, size)
    ids = primary(name, eye, m, size)[0]
    n = len(dirs[0])
    return float(((add > 0) & (add < n) & (ids >= 0)).sum()) / max(hits, 1)
