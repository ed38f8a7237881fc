"""Case generators of the ray-level suite (tests/test_prim_cases.py on the CPU, tests/test_gpu_prims.py
on the device).  Seeded and deterministic.  Every family puts its cases ON the edges
the proofs in rc_device.hpp talk about — a tangent ray, a root that is exactly +-0, the quadric's
linear branch, an exponent gap of 127, a hit point at 1e38 — because no case is ever left out of a
comparison; the coverage conditions (tests/test_prim_cases.py, the oracle's own counters) keep a
family from passing vacuously.  Nothing here comes from the code under test: the references are
numpy's IEEE float32 / float64 arithmetic, libm's pow through ctypes, fractions.Fraction, and the
repository's CPU oracle (rco_prim_*, oracle/rc_oracle.h)."""
import ctypes
import functools
import os
import tempfile
from fractions import Fraction

import numpy as np

from helpers import oracle_lib, random_scene, rc, scene_path

F32, F64, I32, U32, U64 = np.float32, np.float64, np.int32, np.uint32, np.uint64
SPHERE, PLANE, QUADRIC = 0, 1, 2
INF = np.inf
MAX_CASES = 1 << 18            # per family
GOLDEN_SCENES = ["simple", "reflection", "quadric", "example2", "example3", "quadric2"]


# ------------------------------------------------------------------------------ bits --
def bits32(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=F64).view(U64)


def f32_from_bits(b):
    return np.ascontiguousarray(b, dtype=U32).view(F32)


def f64_from_bits(b):
    return np.ascontiguousarray(b, dtype=U64).view(F64)


def nudge32(x, k):
    """float32 x moved by k (an int array) places along the float line (finite x)."""
    i = bits32(x).astype(np.int64)
    o = np.where(i & 0x80000000, -(i & 0x7fffffff), i) + k      # ordered integers
    o = np.clip(o, -0x7f7fffff, 0x7f7fffff)
    return f32_from_bits(np.where(o < 0, (-o) | 0x80000000, o).astype(U32))


def accepted(hit, t):
    """The scan's rule with best = inf (C/raycast.c:441-531): hit && t > 0 && t < inf."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(hit) != 0) & (t > 0) & (t < INF)


def rand_mant64(rng, n):
    """n doubles in [1, 2) with random 52-bit mantissas."""
    return f64_from_bits((rng.integers(0, 1 << 52, n, dtype=np.uint64)) | np.uint64(0x3ff0000000000000))


def float_exponent_sweep(rng, per=6):
    """Floats over every exponent 2^-149 .. 2^127: mantissas 1.0, 2 - ulp and `per` random ones for
    the normal binades, every power of two and random values for the subnormal ones."""
    out = []
    for e in range(-126, 128):
        m = np.concatenate([[1.0, 2.0 - 2.0 ** -23], 1.0 + rng.integers(0, 1 << 23, per) * 2.0 ** -23])
        out.append(np.ldexp(m, e))
    out.append(np.ldexp(1.0, np.arange(-149, -126)))
    out.append(rng.integers(1, 1 << 23, 64) * 2.0 ** -149)
    v = np.concatenate(out).astype(F32)
    assert np.all(v.astype(F64) == np.concatenate(out))          # every one is a float
    return v


# ---------------------------------------------------------------------------- scenes --
class ListScene:
    """A json_data_t built in memory from shape dicts {type, position, u}: `u` is the union of
    shape_t (plane normal[3] / sphere radius / quadric a..j), so every bit is the test's choice."""

    def __init__(self, shapes):
        n = len(shapes)
        self.arr = (rc.ShapeT * n)()
        for k, s in enumerate(shapes):
            r = self.arr[k]
            r.type = s["type"]
            for j, v in enumerate(s.get("position", (0.0, 0.0, 0.0))):
                r.position[j] = v
            for j, v in enumerate(s["u"]):
                r.u[j] = v
            r.reflectivity, r.ior = 0.5, 1.0
            r.next = ctypes.addressof(self.arr[k + 1]) if k + 1 < n else None
        self.js = rc.JsonDataT()
        self.js.camera_width = self.js.camera_height = 2.0
        self.js.shapes_list = ctypes.cast(self.arr, ctypes.POINTER(rc.ShapeT))
        self.js.num_shapes, self.js.num_lights = n, 0


def _sph(c, r):
    return {"type": SPHERE, "position": c, "u": [r]}


def _pln(p, n):
    return {"type": PLANE, "position": p, "u": list(n)}


def _quad(a=0, b=0, c=0, d=0, e=0, f=0, g=0, h=0, i=0, j=0):
    return {"type": QUADRIC, "u": [a, b, c, d, e, f, g, h, i, j]}


# The prim scene: integer spheres (exact +-0 roots), an off-grid sphere, an axis plane and an
# unnormalised one, the example scenes' cylinders (a = 0 / b = 0), a paraboloid along x with a
# linear term (a = 0, g != 0: the linear branch with b_q != 0), an ellipsoid, a paraboloid along z
# — none with cross terms (indices < NO_CROSS: the quad_x0 forms apply) — then two quadrics with
# cross terms, one of them purely bilinear (a = b = c = 0: every axis-parallel D is linear).
PRIM_SHAPES = [
    _sph((0.0, 0.0, -5.0), 1.0),
    _sph((3.0, -2.0, -7.0), 2.0),
    _sph((-4.0, 1.0, -9.0), 3.0),
    _sph((0.3, -0.7, -4.1), 0.37),
    _pln((0.0, -2.0, 0.0), (0.0, 1.0, 0.0)),
    _pln((0.0, -3.0, 0.0), (0.3, 1.2, -0.4)),
    _quad(a=0, b=1, c=1, h=-10, i=20, j=124),
    _quad(a=1, b=0, c=1, g=4, i=10, j=28),
    _quad(a=0, b=1, c=1, g=2, h=-10, i=20, j=124),
    _quad(a=1, b=2, c=0.5, i=6, j=8),
    _quad(a=1, b=1, c=0, i=1, j=3),
    _quad(a=1, b=1, c=1, d=0.5, e=-0.3, f=0.2, g=1, h=-2, i=8, j=14),
    _quad(d=1, i=1, j=2),
]
NO_CROSS = 11


@functools.lru_cache(None)
def prim_scene():
    return ListScene(PRIM_SHAPES)


def shape_table(js):
    """(type[n], position[n,3], u[n,10]) of a json_data_t's shape list."""
    ty, pos, u = [], [], []
    p = js.shapes_list
    while p:
        s = p.contents
        ty.append(s.type)
        pos.append(list(s.position))
        u.append(list(s.u))
        p = ctypes.cast(s.next, ctypes.POINTER(rc.ShapeT))
    return (np.array(ty, I32), np.array(pos, F64).reshape(-1, 3), np.array(u, F64).reshape(-1, 10))


def quadric_form(ty, pos, u, k):
    """Shape k as the ten coefficients of a quadric, in double (generation only)."""
    if ty[k] == SPHERE:
        c, r = pos[k], u[k, 0]
        return np.array([1, 1, 1, 0, 0, 0, -2 * c[0], -2 * c[1], -2 * c[2], c @ c - r * r])
    return u[k].copy()


def abc64(q, O, D):
    """a, b, c of the quadratic in t for rays (O, D) against coefficients q, in double."""
    A, B, C, d, e, f, g, h, i, j = q
    ox, oy, oz = O[..., 0], O[..., 1], O[..., 2]
    dx, dy, dz = D[..., 0], D[..., 1], D[..., 2]
    a = A * dx * dx + B * dy * dy + C * dz * dz + d * dx * dy + e * dx * dz + f * dy * dz
    b = (2 * A * ox * dx + 2 * B * oy * dy + 2 * C * oz * dz + d * (ox * dy + oy * dx)
         + e * (ox * dz + oz * dx) + f * (oy * dz + oz * dy) + g * dx + h * dy + i * dz)
    c = (A * ox * ox + B * oy * oy + C * oz * oz + d * ox * oy + e * ox * oz + f * oy * oz
         + g * ox + h * oy + i * oz + j)
    return a, b, c


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ---------------------------------------------------------------- the oracle's exports --
class PrimCounts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "cases", "sphere", "plane", "quadric", "hits", "accepted", "t_neg", "t_zero", "t_inf",
        "t_nan", "disc_neg", "second_root", "linear", "linear_b0", "plane_den0", "plane_den_sub",
        "plane_num0", "z_rule", "cross_nan")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def ref_shape(js, O, D, shape, skip, cuda=False):
    """(hit, t, counts) of the oracle's shape tests (o_* of the C port, c_* of the CUDA port)."""
    n = len(shape)
    hit, t, cnt = np.zeros(n, I32), np.zeros(n, F32), PrimCounts()
    fn = oracle_lib().rco_prim_shape_cuda if cuda else oracle_lib().rco_prim_shape
    r = fn(ctypes.byref(js), ctypes.c_int64(n), _p(O), _p(D), _p(shape), _p(skip), _p(hit), _p(t),
           ctypes.byref(cnt))
    assert r == 0, r
    return hit, t, cnt.as_dict()


def ref_nearest(js, O, D, skip, shadow=False, cuda=False):
    """idx, t (and P, N, zero events for the C port without the shadow flag) of the oracle's scan."""
    n = len(skip)
    idx, t = np.zeros(n, I32), np.zeros(n, F32)
    if cuda:
        r = oracle_lib().rco_prim_nearest_cuda(ctypes.byref(js), ctypes.c_int64(n), _p(O), _p(D),
                                               _p(skip), int(shadow), _p(idx), _p(t))
        assert r == 0, r
        return idx, t
    P, N, z = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros(n, I32)
    r = oracle_lib().rco_prim_nearest(ctypes.byref(js), ctypes.c_int64(n), _p(O), _p(D), _p(skip),
                                      int(shadow), _p(idx), _p(t), _p(P), _p(N), _p(z))
    assert r == 0, r
    return idx, t, P, N, z


def ref_frame(js, shape, O, D, t):
    n = len(shape)
    P, N, z = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros(n, I32)
    r = oracle_lib().rco_prim_frame(ctypes.byref(js), ctypes.c_int64(n), _p(shape), _p(O), _p(D),
                                    _p(t), _p(P), _p(N), _p(z))
    assert r == 0, r
    return P, N, z


# ------------------------------------------------------------------ ray-level families --
class Cases:
    """n cases (O, D, shape, skip) on one scene; `own` marks the cases whose shape is the one the
    ray was aimed at (the coverage conditions count those)."""

    def __init__(self, js, O, D, shape, skip, own=None):
        self.js = js
        self.O = np.ascontiguousarray(O, F32).reshape(-1, 3)
        self.D = np.ascontiguousarray(D, F32).reshape(-1, 3)
        self.shape = np.ascontiguousarray(shape, I32)
        self.skip = np.ascontiguousarray(skip, I32)
        self.own = np.ones(len(self.shape), bool) if own is None else np.asarray(own, bool)
        assert len(self.O) == len(self.D) == len(self.shape) == len(self.skip) <= MAX_CASES

    def __len__(self):
        return len(self.shape)

    def take(self, mask):
        return Cases(self.js, self.O[mask], self.D[mask], self.shape[mask], self.skip[mask],
                     self.own[mask])


def cross_product(js, O, D, skip, shapes, aim=None):
    """Every ray against every shape of `shapes`; aim[r] = the shape ray r was built for."""
    O, D = np.asarray(O, F32).reshape(-1, 3), np.asarray(D, F32).reshape(-1, 3)
    shapes = np.asarray(shapes, I32)
    r, m = len(O), len(shapes)
    sh = np.tile(shapes, r)
    own = None if aim is None else np.repeat(np.asarray(aim, I32), m) == sh
    return Cases(js, np.repeat(O, m, 0), np.repeat(D, m, 0), sh, np.repeat(np.asarray(skip, I32), m),
                 own)


def origins(rng, n):
    """Ray origins around the camera (the shapes sit at z < 0)."""
    return rng.uniform(-1.5, 1.5, (n, 3)) * [1.0, 1.0, 0.5]


def tangent_rays(rng, js, k, n_origins=48, n_nudges=17):
    """Rays aimed at the silhouette of curved shape k: for each origin the direction where the
    discriminant changes sign (bisection in double between a direction that hits in front and one
    that misses), rounded to float, then every component moved by -8..8 ulps."""
    ty, pos, u = shape_table(js)
    q = quadric_form(ty, pos, u, k)
    O = origins(rng, n_origins)
    cand = unit(rng.normal(size=(n_origins, 256, 3)) * [1.0, 1.0, 0.6] + [0.0, 0.0, -1.0])
    a, b, c = abc64(q, O[:, None, :], cand)
    with np.errstate(invalid="ignore", divide="ignore"):
        disc = b * b - 4 * a * c
        front = (disc > 0) & (a != 0) & (((-b - np.sqrt(disc)) / (2 * a) > 1e-3)
                                        | ((-b + np.sqrt(disc)) / (2 * a) > 1e-3))
    miss = (disc < 0) & (a != 0)
    ok = front.any(1) & miss.any(1)
    O, cand, front, miss = O[ok], cand[ok], front[ok], miss[ok]
    if not len(O):
        return np.zeros((0, 3), F32), np.zeros((0, 3), F32)
    din = cand[np.arange(len(O)), front.argmax(1)]
    dout = cand[np.arange(len(O)), miss.argmax(1)]
    lo, hi = np.zeros(len(O)), np.ones(len(O))
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        d = unit(din * (1 - mid)[:, None] + dout * mid[:, None])
        a, b, c = abc64(q, O, d)
        inside = b * b - 4 * a * c > 0
        lo, hi = np.where(inside, mid, lo), np.where(inside, hi, mid)
    d = unit(din * (1 - lo)[:, None] + dout * lo[:, None]).astype(F32)
    O32 = O.astype(F32)
    ks = rng.integers(-8, 9, (len(O), n_nudges, 3))
    ks[:, 0, :] = 0
    D = nudge32(np.repeat(d[:, None, :], n_nudges, 1), ks)
    return np.repeat(O32, n_nudges, 0), D.reshape(-1, 3)


def curved(js):
    ty, _, _ = shape_table(js)
    return [k for k in range(len(ty)) if ty[k] != PLANE]


@functools.lru_cache(None)
def family_tangent():
    rng, sc = np.random.default_rng(101), prim_scene()
    Os, Ds, sh = [], [], []
    for k in curved(sc.js):
        O, D = tangent_rays(rng, sc.js, k, n_origins=96)
        Os.append(O), Ds.append(D), sh.append(np.full(len(O), k, I32))
    O, D, sh = np.concatenate(Os), np.concatenate(Ds), np.concatenate(sh)
    skip = np.where(rng.uniform(size=len(sh)) < 0.5, -1, (sh + 1) % len(PRIM_SHAPES)).astype(I32)
    return Cases(sc.js, O, D, sh, skip)


def aimed_rays(rng, js, n):
    """n rays from around the camera towards the shapes (where the golden scenes' are too)."""
    O = origins(rng, n)
    D = unit(rng.normal(size=(n, 3)) * [0.6, 0.6, 0.4] + [0.0, 0.0, -1.0])
    return O.astype(F32), D.astype(F32)


def surface_rays(rng, js, n_base=1500, n_dirs=6):
    """Bounce and shadow rays: O is the float hit point of an accepted ray (by the oracle), D a
    new direction; returns (O, D, hit shape)."""
    ty, _, _ = shape_table(js)
    n = len(ty)
    O, D = aimed_rays(rng, js, n_base)
    c = cross_product(js, O, D, np.full(n_base, -1), np.arange(n))
    hit, t, _ = ref_shape(js, c.O, c.D, c.shape, c.skip)
    acc = accepted(hit, t) & (t < 1e4)
    P = (c.O + c.D * t[:, None])[acc]                       # float32 ops, as the frame forms P
    sh = c.shape[acc]
    if len(P) > 1200:
        pick = rng.choice(len(P), 1200, replace=False)
        P, sh = P[pick], sh[pick]
    Dn = unit(rng.normal(size=(len(P), n_dirs, 3))).astype(F32)
    return np.repeat(P, n_dirs, 0), Dn.reshape(-1, 3), np.repeat(sh, n_dirs)


def zero_root_rays():
    """Hand-built roots that are exactly +-0: integer centre c and radius r, O = c +- r e_k, so
    tv = +-r e_k and c = |tv|^2 - r^2 = 0 exactly; then disc = b^2, sqrt(disc) = |b| and one root
    is (-b + |b|) / den or (-b - |b|) / den = +-0.  D = 0 along e_k makes b = +-0 as well."""
    dirs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
                     [0.5, 0.5, 0.5], [-0.25, 0.5, -0.75], [0.0, 0.6, 0.8], [-0.0, -0.6, 0.8],
                     [0.6, 0.0, -0.8], [0.6, -0.8, -0.0]], F32)
    O, D, sh = [], [], []
    for k in (0, 1, 2):
        c, r = np.array(PRIM_SHAPES[k]["position"], F32), F32(PRIM_SHAPES[k]["u"][0])
        for ax in range(3):
            for sgn in (1.0, -1.0):
                o = c.copy()
                o[ax] = c[ax] + F32(sgn) * r
                for d in dirs:
                    O.append(o), D.append(d), sh.append(k)
    return np.array(O, F32), np.array(D, F32), np.array(sh, I32)


@functools.lru_cache(None)
def family_surface():
    rng, sc = np.random.default_rng(202), prim_scene()
    n = len(PRIM_SHAPES)
    P, D, sh = surface_rays(rng, sc.js)
    zO, zD, zsh = zero_root_rays()
    O, D, aim = np.concatenate([P, zO]), np.concatenate([D, zD]), np.concatenate([sh, zsh])
    a = cross_product(sc.js, O, D, aim, np.arange(n), aim)      # skip = the hit shape
    b = cross_product(sc.js, O, D, np.full(len(aim), -1), np.arange(n), aim)
    return Cases(sc.js, np.concatenate([a.O, b.O]), np.concatenate([a.D, b.D]),
                 np.concatenate([a.shape, b.shape]), np.concatenate([a.skip, b.skip]),
                 np.concatenate([a.own, b.own]))


def surface_points(rng, js, k, n):
    """n float points (nearly) on shape k: hit points of accepted aimed rays."""
    O, D = aimed_rays(rng, js, 40 * n)
    sh = np.full(len(O), k, I32)
    hit, t, _ = ref_shape(js, O, D, sh, np.full(len(O), -1, I32))
    acc = accepted(hit, t) & (t < 1e4)
    return (O + D * t[:, None])[acc][:n]


@functools.lru_cache(None)
def family_branches():
    """The quadric's linear branch (a_q == 0 exactly: a zero squared coefficient and an
    axis-parallel D), with b_q == 0 where the axis has no linear coefficient either, and the z
    rule (D.z = +-0 or tiny with skip != -1)."""
    rng, sc = np.random.default_rng(303), prim_scene()
    ty, pos, u = shape_table(sc.js)
    quads = [k for k in range(len(ty)) if ty[k] == QUADRIC]
    mags = np.array([1.0, 0.5, 3.0, 1e-20, 1e20, 3e38, 1e-38, 1e-45], F32)
    O, D, sh, skip = [], [], [], []
    for k in quads:
        pts = np.concatenate([origins(rng, 24).astype(F32), surface_points(rng, sc.js, k, 8)])
        for ax in range(3):
            if u[k, ax] != 0.0:
                continue
            for m in mags:
                for sgn in (1.0, -1.0):
                    for z in (0.0, -0.0):
                        d = np.full(3, z, F32)
                        d[ax] = F32(sgn) * m
                        for o in pts:
                            O.append(o), D.append(d), sh.append(k)
                            skip.append(-1 if len(skip) % 2 else k)
    O, D, sh, skip = np.array(O, F32), np.array(D, F32), np.array(sh, I32), np.array(skip, I32)
    # the z rule: D.z = +-0, +-tiny, +-small on every quadric, skip != -1 (and -1 beside it)
    zs = np.array([0.0, -0.0, 1.4e-45, -1.4e-45, 1e-38, -1e-38, 1e-30, -1e-30, 1e-10, -1e-10,
                   1e-3, -1e-3, 0.3, -0.3], F32)
    zO, zD, zsh, zskip = [], [], [], []
    for k in quads:
        pts = np.concatenate([origins(rng, 24).astype(F32), surface_points(rng, sc.js, k, 8)])
        xy = unit(rng.normal(size=(len(pts), 2))).astype(F32)
        for z in zs:
            for o, d2 in zip(pts, xy):
                for s in (k, (k + 1) % len(ty), -1):
                    zO.append(o), zD.append([d2[0], d2[1], z]), zsh.append(k), zskip.append(s)
    return Cases(sc.js, np.concatenate([O, np.array(zO, F32)]), np.concatenate([D, np.array(zD, F32)]),
                 np.concatenate([sh, np.array(zsh, I32)]), np.concatenate([skip, np.array(zskip, I32)]))


@functools.lru_cache(None)
def family_plane():
    """den == 0 exactly, den subnormal, num == +-0, t overflowing to inf — on the axis plane
    (shape 4, n = (0, 1, 0), p.y = -2) — and generic rays on both planes."""
    rng, sc = np.random.default_rng(404), prim_scene()
    m = 256
    xz = rng.uniform(-2, 2, (m, 2)).astype(F32)
    sub = f32_from_bits(rng.integers(1, 1 << 23, m).astype(U32) | (rng.integers(0, 2, m).astype(U32) << 31))
    zero = np.where(rng.uniform(size=m) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    Og = origins(rng, m).astype(F32)
    O, D = [], []
    # den == 0: D.y = +-0
    O.append(Og), D.append(np.stack([xz[:, 0], zero, xz[:, 1]], 1))
    # den subnormal
    O.append(Og), D.append(np.stack([xz[:, 0], sub, xz[:, 1]], 1))
    # num == +-0: O on the plane (either sign of D.y, zero and subnormal ones too)
    On = Og.copy()
    On[:, 1] = -2.0
    O.append(On), D.append(unit(rng.normal(size=(m, 3))).astype(F32))
    O.append(On), D.append(np.stack([xz[:, 0], sub, xz[:, 1]], 1))
    O.append(On), D.append(np.stack([xz[:, 0], zero, xz[:, 1]], 1))
    # t overflows: |num| huge over |den| tiny, both signs
    Ob = Og.copy()
    Ob[:, 1] = np.where(rng.uniform(size=m) < 0.5, 1e30, -3e38).astype(F32)
    Dt = np.stack([xz[:, 0], np.where(rng.uniform(size=m) < 0.5, 1e-30, -1e-30).astype(F32), xz[:, 1]], 1)
    O.append(Ob), D.append(Dt)
    # generic
    Oa, Da = aimed_rays(rng, sc.js, 4 * m)
    O.append(Oa), D.append(Da)
    O, D = np.concatenate(O), np.concatenate(D).astype(F32)
    skip = np.where(rng.uniform(size=len(O)) < 0.5, -1, 0)
    return cross_product(sc.js, O, D, skip, [4, 5], np.full(len(O), 4))


@functools.lru_cache(None)
def family_nonfinite():
    """O or D with inf / NaN components, and |O| near 3e38 with finite D: the cross sums
    O.x*D.y + O.y*D.x overflow, so a zero cross coefficient times them is NaN (x0_reject)."""
    rng, sc = np.random.default_rng(505), prim_scene()
    n = len(PRIM_SHAPES)
    O, D = [], []
    bad = np.array([INF, -INF, np.nan], F32)
    Ob, Db = aimed_rays(rng, sc.js, 9 * 24)
    for which in (0, 1):
        o, d = Ob.copy(), Db.copy()
        tgt = o if which == 0 else d
        for r in range(len(tgt)):
            tgt[r, r % 3] = bad[(r // 3) % 3]
        O.append(o), D.append(d)
    m = 1536
    big = (rng.uniform(2.0e38, 3.4e38, (m, 3)) * rng.choice([-1.0, 1.0], (m, 3))).astype(F32)
    small = rng.uniform(-3, 3, (m, 3)).astype(F32)
    Obig = np.where(rng.uniform(size=(m, 3)) < 0.7, big, small).astype(F32)
    O.append(Obig), D.append(unit(rng.normal(size=(m, 3))).astype(F32))
    # hit points pushed to 1e38 by D: finite O, huge D
    O.append(origins(rng, 256).astype(F32))
    D.append((unit(rng.normal(size=(256, 3))) * rng.choice([1e30, 3e38, 1e19], (256, 1))).astype(F32))
    O, D = np.concatenate(O), np.concatenate(D)
    skip = np.where(rng.uniform(size=len(O)) < 0.5, -1, rng.integers(0, n, len(O)))
    return cross_product(sc.js, O, D, skip, np.arange(n))


@functools.lru_cache(None)
def family_random():
    rng, sc = np.random.default_rng(606), prim_scene()
    n = len(PRIM_SHAPES)
    O, D = aimed_rays(rng, sc.js, 4096)
    skip = np.where(rng.uniform(size=len(O)) < 0.5, -1, rng.integers(0, n, len(O)))
    return cross_product(sc.js, O, D, skip, np.arange(n))


def primary_dirs(cam_w, cam_h, W=64, H=48):
    """The W x H primary rays of a camera (C/raycast.c:109-118) in numpy's IEEE arithmetic."""
    pw, ph = F32(cam_w) / F32(W), F32(cam_h) / F32(H)
    x, y = np.meshgrid(np.arange(W, dtype=F64), np.arange(H, dtype=F64))
    dx = ((0.0 - F64(F32(cam_w)) / 2.0) + F64(pw) * (x + 0.5)).astype(F32).ravel()
    dy = ((0.0 + F64(F32(cam_h)) / 2.0) - F64(ph) * (y + 0.5)).astype(F32).ravel()
    dz = np.full(len(dx), -1.0, F32)
    s = dx.astype(F64) * dx.astype(F64)
    s = s + dy.astype(F64) * dy.astype(F64)
    s = s + dz.astype(F64) * dz.astype(F64)
    ln = np.sqrt(s).astype(F32)
    return np.stack([dx / ln, dy / ln, dz / ln], 1).astype(F32)


@functools.lru_cache(None)
def family_primary():
    """O = (+0, +0, +0) for the hit_*_o0 forms: the camera's rays and every other family's D."""
    sc = prim_scene()
    n = len(PRIM_SHAPES)
    D = [primary_dirs(2.0, 2.0), primary_dirs(0.7, 1.3, 16, 12)]
    for fam in (family_tangent, family_branches, family_plane, family_nonfinite):
        d = fam().D
        D.append(d[:: max(1, len(d) // 2500)])
    D = np.concatenate(D)
    return cross_product(sc.js, np.zeros_like(D), D, np.full(len(D), -1), np.arange(n))


RAY_FAMILIES = {"tangent": family_tangent, "surface": family_surface, "branches": family_branches,
                "plane": family_plane, "nonfinite": family_nonfinite, "random": family_random,
                "primary": family_primary}


def coverage(name):
    """The oracle's counters for a family (C port), those of its `own` cases beside them."""
    c = RAY_FAMILIES[name]()
    _, _, allc = ref_shape(c.js, c.O, c.D, c.shape, c.skip)
    o = c.take(c.own)
    _, _, own = ref_shape(o.js, o.O, o.D, o.shape, o.skip)
    return allc, own


# ------------------------------------------------------------- scenes for lists, frames --
_TMP = []


@functools.lru_cache(None)
def list_scenes():
    """name -> rc.Scene: the six golden scenes, a 14-shape random scene with cross terms and a
    65-shape one (past the 64-bit reflectivity mask)."""
    out = {n: rc.Scene.from_file(scene_path(n)) for n in GOLDEN_SCENES}
    td = tempfile.TemporaryDirectory()
    _TMP.append(td)
    for name, seed, n, cross in (("random14x", 14, 14, True), ("random65", 65, 65, False)):
        path = os.path.join(td.name, name + ".scene")
        random_scene(np.random.default_rng(seed), path, n, 2, cross=cross)
        out[name] = rc.Scene.from_file(path)
    return out


@functools.lru_cache(None)
def scene_rays(name):
    """(O, D, skip) for the whole-list routines of scene `name`: its own tangent and surface rays
    (curved shapes sampled when there are many), rays of every prim family (their skips folded into
    the scene's range) and 64 x 48 primary rays from O = 0."""
    sc = list_scenes()[name]
    rng = np.random.default_rng(707 + len(name) + sc.num_shapes)
    n = sc.num_shapes
    O, D, skip = [], [], []
    ks = curved(sc.js)
    for k in ks[:: max(1, len(ks) // 8)]:
        o, d = tangent_rays(rng, sc.js, k, n_origins=12, n_nudges=9)
        O.append(o), D.append(d), skip.append(np.where(rng.uniform(size=len(o)) < 0.5, -1, k))
    P, Dn, sh = surface_rays(rng, sc.js, n_base=400, n_dirs=4)
    O.append(P), D.append(Dn), skip.append(np.where(rng.uniform(size=len(sh)) < 0.2, -1, sh))
    for fam in ("tangent", "surface", "branches", "plane", "nonfinite", "random"):
        c = RAY_FAMILIES[fam]()
        step = max(1, len(c) // 1500)
        O.append(c.O[::step]), D.append(c.D[::step])
        skip.append(np.where(c.skip[::step] < 0, -1, c.skip[::step] % n))
    pd = primary_dirs(sc.js.camera_width, sc.js.camera_height)
    O.append(np.zeros_like(pd)), D.append(pd), skip.append(np.full(len(pd), -1))
    return (np.concatenate(O).astype(F32), np.concatenate(D).astype(F32),
            np.concatenate(skip).astype(I32))


# ------------------------------------------------------------------- scalar families --
def division_hard_cases(rng, count):
    """Quotients within 2^-54 ulp of a rounding midpoint — the worst cases of a correctly rounded
    double division.  For an odd 54-bit M (M / 2^54 is the midpoint between two doubles of [1/2, 1))
    take the 53-bit d with d M = +-1 (mod 2^54) and n = (d M -+ 1) / 2^54: then n / d =
    M / 2^54 -+ 1 / (2^54 d).  The operands have full 53-bit mantissas, so they are not
    float-derived: they test the division sequence itself, whose residual correction must see a
    reciprocal good to an ulp (random quotients never come this close)."""
    ns, ds = [], []
    while len(ns) < count:
        M = int(rng.integers(1 << 53, 1 << 54)) | 1
        inv = pow(M, -1, 1 << 54)
        for d, one in ((inv, -1), ((1 << 54) - inv, 1)):
            n = (d * M + one) >> 54
            if (1 << 52) <= d < (1 << 53) and (1 << 52) <= n < (1 << 53):
                assert (d * M + one) % (1 << 54) == 0
                ns.append(float(n)), ds.append(float(d))
    ns, ds = np.array(ns[:count]), np.array(ds[:count])
    sign = rng.choice([-1.0, 1.0], count)
    return np.ldexp(ns, rng.integers(-200, 80, count)) * sign, np.ldexp(ds, rng.integers(-200, 80, count))


@functools.lru_cache(None)
def family_division():
    """(num, den, regular): den = (double)f or 2 (double)f over every float exponent; num =
    (double)(-b) +- sqrt((double)disc) and -(double)c from floats b, disc, c, cancelling pairs
    (disc = b*b rounded) among them, and a sweep of |num| over 2^-201 .. 2^130; then 4096 quotients
    that sit on a rounding midpoint to within 2^-54 ulp (division_hard_cases).  `regular` marks
    finite non-zero operands (subnormal floats widened among them), where every bit of the quotient
    is compared; the rest (a zero, inf or NaN operand) are compared on `accepted` only."""
    rng = np.random.default_rng(11)
    f = float_exponent_sweep(rng)
    f = np.concatenate([f, -f]).astype(F64)
    den = np.concatenate([f, 2.0 * f])
    fb = np.concatenate([float_exponent_sweep(rng, per=3), (rng.normal(size=4096) * 8).astype(F32)])
    fb = np.concatenate([fb, -fb])
    b = fb[np.isfinite(fb)]
    disc = np.abs(rng.permutation(b))
    with np.errstate(over="ignore", under="ignore"):
        canc = (b * b).astype(F32)                                  # disc = b^2 rounded to float
    nums = [(-b).astype(F64) - np.sqrt(disc.astype(F64)), (-b).astype(F64) + np.sqrt(disc.astype(F64)),
            (-b).astype(F64) - np.sqrt(canc.astype(F64)), (-b).astype(F64) + np.sqrt(canc.astype(F64)),
            -(b.astype(F64))]
    e = rng.integers(-201, 131, 8192)
    nums.append(np.ldexp(rand_mant64(rng, 8192), e) * rng.choice([-1.0, 1.0], 8192))
    num = np.concatenate(nums)
    hard_n, hard_d = division_hard_cases(rng, 4096)
    n = MAX_CASES - 4096 - len(hard_n)
    num_r, den_r = num[rng.integers(0, len(num), n)], den[rng.integers(0, len(den), n)]
    # every den against a few nums, so no exponent of the sweep is left to chance
    num_r[: len(den)] = num[rng.integers(0, len(num), len(den))]
    den_r[: len(den)] = den
    # zero, inf and NaN, and beside them subnormal floats widened and the ends of the numerators'
    # range.  (Subnormal DOUBLES are not operands: a float widened is a normal double or zero, and
    # -b +- sqrt(disc) is a multiple of 2^-201.)
    spec = np.array([0.0, -0.0, INF, -INF, np.nan, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -127,
                     -(2.0 ** -126 - 2.0 ** -149), 1.0, -1.0, 2.0 ** 130, -(2.0 ** -201)], F64)
    sn, sd = np.meshgrid(spec, spec)
    sn, sd = sn.ravel(), sd.ravel()
    k = 4096 - len(sn)
    odd = rng.uniform(size=k) < 0.5
    mix_n = np.where(odd, spec[rng.integers(0, 5, k)], num[rng.integers(0, len(num), k)])
    mix_d = np.where(odd & (rng.uniform(size=k) < 0.7), den[rng.integers(0, len(den), k)],
                     spec[rng.integers(0, 5, k)])
    num_a = np.concatenate([num_r, hard_n, sn, mix_n])
    den_a = np.concatenate([den_r, hard_d, sd, mix_d])

    def normal(x):
        return np.isfinite(x) & (np.abs(x) >= 2.0 ** -1022)
    return num_a, den_a, normal(num_a) & normal(den_a)


def sqrt_hard_cases():
    """Square roots within 2^-44 ulp of a rounding midpoint — the worst cases of a correctly
    rounded sqrt.  With y = m + 1/2 for a 53-bit m, y^2 = m (m + 1) + 1/4; for an even c, |c| <=
    1024, solve m (m + 1) = c (mod 2^k) (a square root of 1 + 4 c modulo 2^(k+2), by Hensel
    lifting) and take S = (m (m + 1) - c) / 2^k when it is a 53-bit integer: then
    sqrt(S 2^k) = y - (c + 1/4) / (2 y) to first order.  Random inputs never come this close."""
    out = []
    for k in (52, 53):
        n = k + 2
        for c in range(-1024, 1025, 2):
            a = (1 + 4 * c) % (1 << n)
            x = 1
            for i in range(3, n):                       # x^2 = a (mod 2^i) -> (mod 2^(i+1))
                if (x * x - a) % (1 << (i + 1)):
                    x += 1 << (i - 1)
            assert (x * x - a) % (1 << n) == 0
            for r in (x, -x, x + (1 << (n - 1)), -x + (1 << (n - 1))):
                m = ((r % (1 << n)) - 1) // 2 % (1 << k)
                if not (1 << 52) <= m < (1 << 53) or (m * (m + 1) - c) % (1 << k):
                    continue
                S = (m * (m + 1) - c) >> k
                if (1 << 52) <= S < (1 << 53):
                    for j in (-300, -1, 0, 7, 200):
                        out.append(float(np.ldexp(float(S), k + 2 * j - 104)))
    return np.array(sorted(set(out)), F64)


@functools.lru_cache(None)
def family_sqrt():
    """+-0, every binade from 2^-767 up, sums of squares of floats, widened floats down to 2^-149,
    one ulp either side of perfect squares, inf and NaN; then the constructed roots that sit on a
    rounding midpoint (sqrt_hard_cases)."""
    rng = np.random.default_rng(22)
    out = [np.array([0.0, -0.0, INF, np.nan], F64)]
    e = np.arange(-767, 1024)
    for m in (1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52, 1.5, 2.0 ** 0.5):
        out.append(np.ldexp(m, e))
    for _ in range(24):
        out.append(np.ldexp(rand_mant64(rng, len(e)), e))
    f = float_exponent_sweep(rng).astype(F64)
    out.append(f)
    tri = rng.permutation(np.concatenate([f, (rng.normal(size=(20000)) * 4)]).astype(F32))
    tri = tri[: len(tri) // 3 * 3].reshape(-1, 3).astype(F64)
    s = tri[:, 0] * tri[:, 0]
    s = s + tri[:, 1] * tri[:, 1]
    s = s + tri[:, 2] * tri[:, 2]
    out.append(s)
    k = np.ldexp(rng.integers(1 << 25, 1 << 26, 20000).astype(F64), rng.integers(-380, 480, 20000))
    sq = k * k                                                       # exact: 26-bit k
    out += [sq, np.nextafter(sq, 0.0), np.nextafter(sq, INF), sqrt_hard_cases()]
    return np.concatenate(out)


@functools.lru_cache(None)
def family_vec():
    """(a[n,3], len[n]) for length and div3: random float triples, components spanning
    2^-149 .. 2^127, len = inf, quotients that are exact floats, triples whose sum of squares is
    subnormal in float; div3 also gets arbitrary (a, len) pairs and len = inf, NaN.  len = 0 is the
    caller's case (normalize) and is not a div3 input."""
    rng = np.random.default_rng(33)
    f = float_exponent_sweep(rng, per=10)
    f = np.concatenate([f, -f])
    a = [rng.normal(size=(30000, 3)).astype(F32), rng.permutation(f)[: len(f) // 3 * 3].reshape(-1, 3),
         (rng.uniform(1.0, 3.3, (2000, 3)) * 1e38).astype(F32),                 # len = inf
         (rng.normal(size=(4000, 3)) * 1e-23).astype(F32),                      # subnormal sum
         (rng.normal(size=(4000, 3)) * rng.choice([1e-30, 1e-12, 1e12, 1e30], (4000, 1))).astype(F32)]
    mixed = rng.choice(f, (20000, 3))
    a.append(mixed)
    a = np.concatenate(a).astype(F32)
    sq = a.astype(F64)
    s = sq[:, 0] * sq[:, 0]
    s = s + sq[:, 1] * sq[:, 1]
    s = s + sq[:, 2] * sq[:, 2]
    with np.errstate(over="ignore"):
        ln = np.sqrt(s).astype(F32)                                  # (float)sqrt(double sum)
    keep = ln != 0
    a3, l3 = [a[keep]], [ln[keep]]
    # exact quotients: a = k * len, small integers k
    ex_l = rng.choice(f[np.abs(f) < 1e30], 6000).astype(F32)
    ex_l = ex_l[ex_l != 0]
    ks = rng.integers(-64, 65, (len(ex_l), 3)).astype(F32)
    a3.append((ks * ex_l[:, None]).astype(F32)), l3.append(ex_l)
    # arbitrary pairs, and len = inf / NaN with finite, infinite and NaN components
    pa, pl = rng.choice(f, (30000, 3)), rng.choice(f, 30000)
    pl = pl[pl != 0] if np.any(pl == 0) else pl
    a3.append(pa[: len(pl)]), l3.append(pl)
    odd = np.array([[1.0, -2.0, 0.0], [INF, -INF, np.nan], [3e38, -1e-45, -0.0]], F32)
    for v in (INF, np.nan):
        a3.append(odd), l3.append(np.full(3, v, F32))
    return a, ln, np.concatenate(a3).astype(F32), np.concatenate(l3).astype(F32)


@functools.lru_cache(None)
def family_quot_class():
    """(num, den): exponent gaps -160 .. 140 with mantissas 1.0, 2 - ulp (double's and float's) on
    each side and both signs; the gaps outside [-148, 126] again with random mantissas; zero,
    subnormal, inf and NaN operands against each other and against random normal ones."""
    rng = np.random.default_rng(44)
    mant = np.array([1.0, 2.0 - 2.0 ** -52, 2.0 - 2.0 ** -23])
    num, den = [], []
    for base in (0, -300, 250):
        for gap in range(-160, 141):
            for mn in mant:
                for md in mant:
                    for sn, sd in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                        ed = base - gap // 2
                        num.append(sn * np.ldexp(mn, ed + gap)), den.append(sd * np.ldexp(md, ed))
    num, den = [np.array(num)], [np.array(den)]
    gaps = np.concatenate([np.arange(-160, -148), np.arange(127, 141)])
    g = np.repeat(gaps, 400)
    ed = rng.integers(-200, 200, len(g))
    num.append(np.ldexp(rand_mant64(rng, len(g)), ed + g) * rng.choice([-1.0, 1.0], len(g)))
    den.append(np.ldexp(rand_mant64(rng, len(g)), ed) * rng.choice([-1.0, 1.0], len(g)))
    spec = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -2.2e-308, 1e-310, INF, -INF, np.nan,
                     -np.nan], F64)
    a, b = np.meshgrid(spec, spec)
    num.append(a.ravel()), den.append(b.ravel())
    m = 1200
    for s in spec:
        r = np.ldexp(rand_mant64(rng, m), rng.integers(-201, 131, m)) * rng.choice([-1.0, 1.0], m)
        num.append(np.full(m, s)), den.append(r)
        num.append(r), den.append(np.full(m, s))
    return np.concatenate(num), np.concatenate(den)


def quot_class_ref(num, den):
    """The class of float32(float64(num) / float64(den)): 0 t < 0, 1 t = +-0, 2 0 < t < inf,
    3 inf or NaN (rc_device.hpp kQNeg .. kQOther)."""
    with np.errstate(all="ignore"):
        t = (num / den).astype(F32)
        return np.where(t < 0, 0, np.where(t == 0, 1, np.where(t < INF, 2, 3))).astype(I32)


def quot_class_fast(num, den):
    """Does quot_class decide (num, den) from the exponents alone (its stated domain)?"""
    en = ((bits64(num) >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64)
    ed = ((bits64(den) >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64)
    e = en - ed
    return (en != 0) & (en != 0x7ff) & (ed != 0) & (ed != 0x7ff) & (e >= -148) & (e <= 126)


@functools.lru_cache(None)
def family_x0():
    """(O, D) for x0_reject: the non-finite family's rays and ordinary ones."""
    a, b = family_nonfinite(), family_random()
    n = len(PRIM_SHAPES)
    return np.concatenate([a.O[::n], b.O[::n]]), np.concatenate([a.D[::n], b.D[::n]])


def x0_reject_ref(O, D):
    """Is some cross term of a quadric with d = e = f = +-0 NaN (the oracle's own condition,
    rc_oracle.c o_quadric)?  float32 arithmetic as written there."""
    with np.errstate(all="ignore"):
        z = F32(0.0)
        terms = [z * D[:, 0] * D[:, 1], z * D[:, 0] * D[:, 2], z * D[:, 1] * D[:, 2],
                 z * (O[:, 0] * D[:, 1] + O[:, 1] * D[:, 0]), z * (O[:, 0] * D[:, 2] + O[:, 2] * D[:, 0]),
                 z * (O[:, 1] * D[:, 2] + O[:, 2] * D[:, 1]), z * O[:, 0] * O[:, 1],
                 z * O[:, 0] * O[:, 2], z * O[:, 1] * O[:, 2]]
        return np.any(np.isnan(np.stack(terms)), 0)


# ------------------------------------------------------------------------- powers --
POW20_SL = np.array([1.0, 0.5, 2.0, 0.1, 0.3, 0.7, 1.5, 4.0, 0.05, 3.3, 0.25, 0.9, 1.2, 2.7, 0.6,
                     0.01], F32)
POWN_EXPONENTS = list(range(-8, 0)) + list(range(3, 13)) + [20, 31]
PROBE_EXPONENTS = [-1, -2, -3, -5, -9]      # scripts/spot_exp_probe.py's integer angular-a0 values
PROBE_THETAS = [0.3, 0.9]
POWN_EDGE_BASES = [0.0, INF, np.nan, 1e-30, 1e-10, 1e20, 1e30, 3e38, 1.4e-45, 1e-38, 2.0 ** -13,
                   2.0 ** -14, 2.0 ** 13, 2.0 ** 14, 0.75, 1.0]     # and the negative of each
POWN_EDGE_EXPONENTS = list(range(-64, 65))


@functools.lru_cache(None)
def family_pow20():
    """x = (double)float in [-1, 0] (the specular term's angle is <= 0 there): 2^15 inputs, the
    ends, negative powers of two and their neighbours among them."""
    rng = np.random.default_rng(55)
    k = -np.ldexp(1.0, -np.arange(0, 40)).astype(F32)
    edge = np.concatenate([[-0.0, 0.0], k, np.nextafter(k, F32(0)), np.nextafter(k, F32(-2))[1:]])
    x = np.concatenate([edge.astype(F32), -rng.uniform(0, 1, (1 << 15) - len(edge)).astype(F32)])
    return x.astype(F64)


@functools.lru_cache(None)
def family_pown():
    """(a, n): alpha = (double)float against every integer exponent of POWN_EXPONENTS, and the
    spot-exponent probe's cases (its integer exponents, alpha in [cos_theta, 1] for its thetas, with
    the scene reader's cos_theta = (float)cos(theta * 180 / PI_f)); then POWN_EDGE_BASES of both
    signs (+-0, +-inf, NaN, 1e-30 .. 3e38, the two sides of pown_dd's range guard) against every
    exponent -64 .. 64."""
    rng = np.random.default_rng(66)
    a = np.concatenate([rng.uniform(0.05, 1.0, 3000), rng.uniform(1.0, 2.0, 300),
                        -rng.uniform(0.05, 1.5, 300), np.ldexp(1.0, -np.arange(0, 16)),
                        1.0 - np.ldexp(1.0, -np.arange(1, 25)), [2.0 ** -20, 1.0 + 2.0 ** -23]]).astype(F32)
    A = [np.tile(a, len(POWN_EXPONENTS))]
    N = [np.repeat(np.array(POWN_EXPONENTS, I32), len(a))]
    for th in PROBE_THETAS:
        deg = F32(F64(F32(th)) * (180.0 / F64(F32(3.141592654))))
        cos_theta = F32(np.cos(F64(deg)))
        al = np.concatenate([[cos_theta, 1.0], rng.uniform(min(cos_theta, 1.0), 1.0, 700)]).astype(F32)
        for n in PROBE_EXPONENTS:
            A.append(al), N.append(np.full(len(al), n, I32))
    # the edges: alpha is a dot product with a direction nobody normalises, so it can be +-0 (P - L.pos
    # perpendicular to the direction), huge, tiny, infinite or NaN — against every exponent the
    # packer treats as an integer
    edge = np.array(POWN_EDGE_BASES, F32)
    edge = np.concatenate([edge, -edge])
    ne = np.array(POWN_EDGE_EXPONENTS, I32)
    A.append(np.repeat(edge, len(ne))), N.append(np.tile(ne, len(edge)))
    A, N = np.concatenate(A).astype(F64), np.concatenate(N)
    assert len(A) <= 1 << 17
    return A, N


def pown_regular(a, n):
    """Cases inside the range pown_dd states for its double-double product: a finite and non-zero,
    (|x| + 1) |n| <= 900 for x = floor(log2 |a|), so that a^|n| and its error term are normal
    doubles.  There the double itself is compared with the exactly rounded power.  Everywhere else
    — zero, infinite and NaN bases, powers at least 2^772 from 1, all of which overflow or
    underflow float — only the narrowed value is."""
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.frexp(np.abs(a))[1] - 1
        return np.isfinite(a) & (a != 0) & ((np.abs(x) + 1) * np.abs(n) <= 900)


_libm = None


def libm_pow(x, y):
    """glibc's pow — the reference's function — one call a case."""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL("libm.so.6")
        _libm.pow.restype = ctypes.c_double
        _libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]
    y = np.broadcast_to(np.asarray(y, F64), x.shape)
    return np.array([_libm.pow(float(a), float(b)) for a, b in zip(x, y)], F64)


def exact_pow(x, n):
    """x^n rounded ONCE to double: rational arithmetic, then Python's correctly rounded
    int / int division (x != 0 for n < 0; results here stay in the normal range)."""
    n = np.broadcast_to(np.asarray(n), x.shape)
    out = np.empty(len(x), F64)
    for i, (a, k) in enumerate(zip(x, n)):
        k = int(k)
        fa = Fraction(float(a))
        if fa == 0:
            z = float(a) if k % 2 else 0.0                   # an odd power keeps the zero's sign
            out[i] = z if k > 0 else np.copysign(INF, z)
            continue
        p = fa ** abs(k)
        p = 1 / p if k < 0 else p
        out[i] = p.numerator / p.denominator
    return out


def ulp_distance(a, b):
    """Places between doubles a and b along the float line (finite, same-sign or zero)."""
    ia, ib = bits64(a).astype(np.int64), bits64(b).astype(np.int64)
    oa = np.where(ia < 0, -(ia & 0x7fffffffffffffff), ia)
    ob = np.where(ib < 0, -(ib & 0x7fffffffffffffff), ib)
    return np.abs(oa - ob)
