"""The G-buffer through a camera, the guided filter and the ambient compose: the expectation of
tests/test_guided.py and tests/test_gpu_guided.py, taken from the oracle.  The
guide is ao_cases.primary's (rco_prim_nearest(eye, d, skip = -1) and its frame) with t from
ray_cases.ref_trace_from(..., 1); the states are ao_cases.open_add put through rc.ao_step; the
compose's shape table is the oracle's quant (shade_cases.ref_quant) of one float32 product.  The
filter's rule itself is rc.ao_filter, the contract in numpy, which tests/test_guided.py holds against
a pixel-by-pixel restatement.  References are computed once per key and are read-only."""
import ctypes

import numpy as np

import ao_cases as aoc
import ray_cases as rcs
import shade_cases as shc
from helpers import rc

F32, I32 = np.float32, np.int32
INF = np.inf

SIZE = aoc.SIZE                      # 33 x 17
CAMS = aoc.CAMS                      # 0, 1, 3, 9, 14 of ray_cases.CAMERAS
MIXED_CAMS = (0, 3, 9, 14)           # cameras whose windows hold accepted and rejected neighbours
ALL_ACCEPTED_CAM = 1                 # the eye inside a sphere: nothing is rejected at radius <= 3
FULL, WINDOW = aoc.FULL, aoc.WINDOW
CORNER, CORNER_SIZE = aoc.CORNER, aoc.CORNER_SIZE
ROT = aoc.ROT
SHORT = ((1, (2, 1)), (3, (6, 4, 2, 1)))   # the (radius, taps) of the input conditions
NMIN, DPLANE = 0.9, 0.05

_T, _STATE = {}, {}


def planes(name, eye, m, size=SIZE, window=None):
    """{"id", "t", "P", "N"} of the camera's primary hits: rc_render_camera_gbuffer's planes."""
    key = (name, np.asarray(eye, F32).tobytes(), np.asarray(m, F32).tobytes(), size, window)
    ids, P, N = aoc.primary(name, eye, m, size, window)
    if key not in _T:
        sc, (w, h) = rcs.scene(name), size
        fw, fh, x0, y0 = window if window else (w, h, 0, 0)
        d = rcs.camera_dirs(sc, m, (fw, fh), rc.view_grid(w, h, x0, y0))
        O = np.tile(np.asarray(eye, F32), (len(d), 1))
        _, ids2, t, _, _ = rcs.ref_trace_from(sc.js, O, d, 1)
        assert (ids2.reshape(h, w) == ids).all()
        t = t.reshape(h, w)
        t.setflags(write=False)
        _T[key] = t
    return {"id": ids, "t": _T[key], "P": P, "N": N}


def state(name, eye, m, sets, size=SIZE, window=None):
    """The occlusion state after a reset pass with sets[0] and one pass a further set."""
    key = (name, np.asarray(eye, F32).tobytes(), np.asarray(m, F32).tobytes(), size, window,
           tuple((np.asarray(u, F32).tobytes(), float(t)) for u, t in sets))
    if key not in _STATE:
        w, h = size
        acc = np.zeros((h, w), rc.AO_DTYPE)
        for k, dirs in enumerate(sets):
            add = aoc.open_add(name, eye, m, dirs, size, window)[0]
            acc, sat = rc.ao_step(acc, add, len(dirs[0]), reset=k == 0)
            assert sat == 0
        acc.setflags(write=False)
        _STATE[key] = acc
    return _STATE[key]


def two_pass_sets(n=16):
    return [rc.ao_dirs(n), rc.ao_dirs(n, INF, ROT)]


def diffuse_colors(js):
    """[n_shapes, 3] float32: the shapes' diffuse colours in the scene's order."""
    out, p = [], js.shapes_list
    while p:
        s = p.contents
        out.append(list(s.diffuse_color))
        p = ctypes.cast(s.next, ctypes.POINTER(rc.ShapeT))
    return np.array(out, F32).reshape(-1, 3)


def shape_table(js, ambient):
    """[n_shapes, 3] uint8: rco_prim_quant(ambient[c] * diffuse_color_k[c]), one float32 product."""
    d = diffuse_colors(js)
    with np.errstate(all="ignore"):
        prod = (d * np.asarray(ambient, F32)[None, :]).astype(F32)
    return shc.ref_quant(np.ascontiguousarray(prod.reshape(-1))).reshape(-1, 3)


def filter_pixel_by_pixel(acc, ids, P, N, params):
    """rc.ao_filter's rule restated with Python loops and Python ints (small planes only)."""
    h, w = ids.shape
    r = params.radius
    taps = [int(params.taps[d]) for d in range(r + 1)]
    nmin, dplane = F32(params.nmin), F32(params.dplane)
    out = np.zeros((h, w), np.uint8)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                o, ry = int(acc["open"][y, x]), int(acc["rays"][y, x])
                if ids[y, x] < 0:
                    out[y, x] = (510 * o + ry) // (2 * ry) if ry else 255
                    continue
                O = R = 0
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        qy, qx = y + dy, x + dx
                        if not (0 <= qy < h and 0 <= qx < w):
                            continue
                        ok = dx == 0 and dy == 0
                        if not ok and ids[qy, qx] == ids[y, x]:
                            Np, Nq = N[y, x], N[qy, qx]
                            e = P[qy, qx] - P[y, x]
                            nd = F32(F32(Np[0] * Nq[0]) + F32(Np[1] * Nq[1])) + F32(Np[2] * Nq[2])
                            pd = F32(F32(Np[0] * e[0]) + F32(Np[1] * e[1])) + F32(Np[2] * e[2])
                            ok = bool(nd >= nmin) and bool(np.abs(pd) <= dplane)
                        if ok:
                            wgt = taps[abs(dx)] * taps[abs(dy)]
                            O += wgt * int(acc["open"][qy, qx])
                            R += wgt * int(acc["rays"][qy, qx])
                out[y, x] = (510 * O + R) // (2 * R) if R else 255
    return out


def neighbour_shares(acc, g, params):
    """(mixed, changed, unguided_differs, hits): the shares of the hit pixels that have both an
    accepted and a rejected neighbour inside the plane, whose filtered byte differs from the plain
    byte, and whose filtered byte differs from the unguided filter's (every neighbour pooled: nmin
    -inf, dplane +inf, ids ignored)."""
    ids, P, N = g["id"], g["P"], g["N"]
    h, w = ids.shape
    r = params.radius
    hit = ids >= 0
    acc_n, rej_n = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    nmin, dplane = F32(params.nmin), F32(params.dplane)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dx == 0 and dy == 0:
                    continue
                ya, yb = max(0, -dy), min(h, h - dy)
                xa, xb = max(0, -dx), min(w, w - dx)
                if ya >= yb or xa >= xb:
                    continue
                ps = (slice(ya, yb), slice(xa, xb))
                qs = (slice(ya + dy, yb + dy), slice(xa + dx, xb + dx))
                Np, Nq, e = N[ps], N[qs], P[qs] - P[ps]
                nd = (Np[..., 0] * Nq[..., 0] + Np[..., 1] * Nq[..., 1]) + Np[..., 2] * Nq[..., 2]
                pd = (Np[..., 0] * e[..., 0] + Np[..., 1] * e[..., 1]) + Np[..., 2] * e[..., 2]
                ok = (ids[qs] == ids[ps]) & (nd >= nmin) & (np.abs(pd) <= dplane)
                acc_n[ps] += ok
                rej_n[ps] += ~ok
    guided = rc.ao_filter(acc, ids, P, N, params)
    every = rc.ao_filter_params(r, [int(params.taps[d]) for d in range(r + 1)], -INF, INF)
    zeros = np.zeros_like(P)                              # every dot is 0: nothing is rejected
    unguided = rc.ao_filter(acc, np.zeros_like(ids), zeros, zeros, every)
    plain = rc.ao_byte(acc)
    n = max(int(hit.sum()), 1)
    return (float(((acc_n > 0) & (rej_n > 0) & hit).sum()) / n,
            float(((guided != plain) & hit).sum()) / n,
            float(((guided != unguided) & hit).sum()) / n, int(hit.sum()))
