"""Case generators of the hit-level suite (tests/test_shade_cases.py on the CPU, tests/test_gpu_shading.py
on the device): what happens AFTER the hit — calc_color (shade, cu_shade), the bounce
loop (shoot<MODE>, shade_dep_cont), quant and primary_dir.  Seeded and deterministic.  A family is a
list of ShadeCases (one scene each: the shape a case shades, its hit point P, normal N and ray
direction D) or ShootCases (primary directions, carry-ins and a recursion limit).  Scenes whose
every bit matters (a light's cos_theta, an unnormalised direction, a reflectivity that is NaN) are
built in memory as the reference's lists; the others are the golden scene files and seeded random
scenes through the scene reader.  The references are the repository's CPU oracle (rco_prim_shade,
rco_prim_shoot, rco_prim_quant: oracle/rc_oracle.h) and numpy's IEEE arithmetic; nothing here comes
from the code under test."""
import ctypes
import functools
import os
import re
import tempfile

import numpy as np

import prim_cases as pc
from helpers import oracle_lib, random_scene, rc, scene_path

F32, F64, I32, U8 = np.float32, np.float64, np.int32, np.uint8
INF, NAN = np.inf, np.nan
MAX_CASES = 1 << 16            # per family
POINT, SPOT = 0, 1
_p = pc._p


# ---------------------------------------------------------------------------- scenes --
class LitScene:
    """A json_data_t built in memory: shapes as prim_cases.ListScene's dicts plus diffuse, specular,
    refl, refr; lights {pos, color, radial, spot, cos_theta, a0, dir}.  A spot light's cos_theta and
    direction are stored as given (the scene reader derives cos_theta from an angle and normalises
    nothing)."""

    def __init__(self, shapes, lights, cam=(2.0, 2.0)):
        n, m = len(shapes), len(lights)
        self.arr = (rc.ShapeT * max(n, 1))()
        for k, s in enumerate(shapes):
            r = self.arr[k]
            r.type = s["type"]
            for j in range(3):
                r.position[j] = s.get("position", (0.0, 0.0, 0.0))[j]
                r.diffuse_color[j] = s.get("diffuse", (0.8, 0.6, 0.4))[j]
                r.specular_color[j] = s.get("specular", (0.5, 0.7, 0.9))[j]
            for j, v in enumerate(s["u"]):
                r.u[j] = v
            r.reflectivity, r.refractivity, r.ior = s.get("refl", 0.25), s.get("refr", 0.0), 1.0
            r.next = ctypes.addressof(self.arr[k + 1]) if k + 1 < n else None
        self.larr = (rc.LightT * max(m, 1))()
        for k, l in enumerate(lights):
            r = self.larr[k]
            for j in range(3):
                r.position[j] = l.get("pos", (0.0, 0.0, 0.0))[j]
                r.color[j] = l.get("color", (1.5, 1.25, 0.75))[j]
                r.radial_coef[j] = l.get("radial", (0.0125, 0.0125, 0.01))[j]
            if l.get("spot"):
                r.type = SPOT
                r.theta, r.cos_theta, r.a0 = 1.0, l["cos_theta"], l["a0"]
                for j in range(3):
                    r.direction[j] = l["dir"][j]
            r.next = ctypes.addressof(self.larr[k + 1]) if k + 1 < m else None
        self.js = rc.JsonDataT()
        self.js.camera_width, self.js.camera_height = cam
        self.js.shapes_list = ctypes.cast(self.arr, ctypes.POINTER(rc.ShapeT)) if n else None
        self.js.lights_list = ctypes.cast(self.larr, ctypes.POINTER(rc.LightT)) if m else None
        self.js.num_shapes, self.js.num_lights = n, m
        self.num_shapes, self.num_lights = n, m


_FAR = dict(pc._pln((0.0, -1000.0, 0.0), (0.0, 1.0, 0.0)))     # the shaded record: never in the way
                                                                # (its own shadow rays skip it)

_TMP = []


def _text_scene(name, text):
    if not _TMP:
        _TMP.append(tempfile.TemporaryDirectory())
    path = os.path.join(_TMP[0].name, name + ".scene")
    with open(path, "w") as f:
        f.write(text)
    return rc.Scene.from_file(path)


def _light_line(rng, spot):
    col = rng.uniform(0.4, 2.5, 3)
    pos = [rng.uniform(-8, 8), rng.uniform(1, 9), rng.uniform(-12, 2)]
    extra = ""
    if spot:
        d = rng.normal(size=3) * [0.4, 0.4, 0.2] + [0, -0.6, -0.8]
        extra = (f", theta: {rng.uniform(0.2, 1.2):.3f}, angular-a0: {int(rng.integers(0, 5))}, "
                 f"direction: [{d[0]:.3f}, {d[1]:.3f}, {d[2]:.3f}]")
    return (f"light, color: [{col[0]:.2f}, {col[1]:.2f}, {col[2]:.2f}], radial-a2: 0.01, radial-a1: "
            f"0.0125, radial-a0: 0.0125, position: [{pos[0]:.2f}, {pos[1]:.2f}, {pos[2]:.2f}]{extra}")


def _unit_normals(text):
    """The scene text with every plane normal scaled to length 1 (six decimals).  shade hands
    pow20 the dot product of -D and reflect(ld, N); pow20 states the domain |x| <= 4, which holds
    for unit N (|x| <= 3) but not for a normal of any length (|x| <= 1 + 2 |N|^2)."""
    def fix(m):
        v = np.array([float(t) for t in m.group(1).split(",")])
        v = v / np.linalg.norm(v)
        return f"normal: [{v[0]:.6f}, {v[1]:.6f}, {v[2]:.6f}]"
    return re.sub(r"normal: \[([^\]]*)\]", fix, text)


def random_unit_scene(name, seed, n, cross=False):
    """helpers.random_scene with unit plane normals, through the scene reader."""
    if not _TMP:
        _TMP.append(tempfile.TemporaryDirectory())
    raw = os.path.join(_TMP[0].name, name + ".raw")
    random_scene(np.random.default_rng(seed), raw, n, 2, cross=cross)
    return _text_scene(name, _unit_normals(open(raw).read()))


@functools.lru_cache(None)
def lit_scenes():
    """name -> rc.Scene: the six golden scenes (1, 2 or 3 lights each), a 14-shape random scene
    with cross terms, a 64- and a 65-shape one (either side of the 64-bit reflectivity mask), and
    the quadric example's shapes under 0, 3 and 6 lights, point and spot mixed."""
    out = {n: rc.Scene.from_file(scene_path(n)) for n in pc.GOLDEN_SCENES}
    out["random14x"] = random_unit_scene("random14x", 14, 14, cross=True)
    out["random64"] = random_unit_scene("random64", 64, 64)
    out["random65"] = random_unit_scene("random65", 65, 65)
    shapes = [ln for ln in open(scene_path("quadric")).read().splitlines() if not ln.startswith("light")]
    rng = np.random.default_rng(2020)
    for m in (0, 3, 6):
        lights = [_light_line(rng, k % 2 == 1) for k in range(m)]
        out[f"lights{m}"] = _text_scene(f"lights{m}", "\n".join(shapes + lights) + "\n")
    return out


# ---------------------------------------------------------------- the oracle's exports --
class ShadeCounts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "shades", "opacity_le0", "phantom", "lights", "shadowed", "dist0", "th_le0", "th_nan", "spot",
        "cone_out", "alpha_eq_cos", "alpha_zero", "alpha_neg_in", "rad_nonfinite", "ang_nonfinite",
        "specular", "spec_arg_nan")] + [("spec_arg_max", ctypes.c_double)] + [
        (n, ctypes.c_int64) for n in ("shoots", "primary_miss", "bounce_iters", "end_maxrec",
                                      "end_nonrefl", "end_miss", "dep")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def add_counts(a, b):
    return {k: (max(a[k], b[k]) if k == "spec_arg_max" else a[k] + b[k]) for k in a}


def ref_shade(js, idx, P, N, D, cuda=False):
    """(rgb[n,3], zero[n], counts) of o_shade (c_shade: no zero events, no phantom)."""
    n = len(idx)
    rgb, zero, cnt = np.zeros((n, 3), F32), np.zeros(n, I32), ShadeCounts()
    if cuda:
        r = oracle_lib().rco_prim_shade_cuda(ctypes.byref(js), ctypes.c_int64(n), _p(idx), _p(P), _p(N),
                                             _p(D), _p(rgb), ctypes.byref(cnt))
    else:
        r = oracle_lib().rco_prim_shade(ctypes.byref(js), ctypes.c_int64(n), _p(idx), _p(P), _p(N),
                                        _p(D), _p(rgb), _p(zero), ctypes.byref(cnt))
    assert r == 0, r
    return rgb, zero, cnt.as_dict()


def ref_shoot(js, d, maxrec, mode, carry_in=None):
    """(rgb[n,3] float, cls[n], carry_out[n,3], zero[n], counts) of o_shoot; mode "fast" / "parity"."""
    n = len(d)
    rgb, cls, cout = np.zeros((n, 3), F32), np.zeros(n, U8), np.zeros((n, 3), F32)
    zero, cnt = np.zeros(n, I32), ShadeCounts()
    r = oracle_lib().rco_prim_shoot(ctypes.byref(js), ctypes.c_int64(n), _p(d), int(maxrec),
                                    rc.MODES[mode], None if carry_in is None else _p(carry_in),
                                    _p(rgb), _p(cls), _p(cout), _p(zero), ctypes.byref(cnt))
    assert r == 0, r
    return rgb, cls, cout, zero, cnt.as_dict()


def ref_shoot_cuda(js, d, max_iter):
    n = len(d)
    rgb, cnt = np.zeros((n, 3), F32), ShadeCounts()
    r = oracle_lib().rco_prim_shoot_cuda(ctypes.byref(js), ctypes.c_int64(n), _p(d), int(max_iter),
                                         _p(rgb), ctypes.byref(cnt))
    assert r == 0, r
    return rgb, cnt.as_dict()


def ref_quant(c):
    q = np.zeros(len(c), U8)
    oracle_lib().rco_prim_quant(ctypes.c_int64(len(c)), _p(np.ascontiguousarray(c, F32)), _p(q))
    return q


# ----------------------------------------------------------------------- case lists --
class ShadeCases:
    """n hits on one scene: the shaded shape (-1: the phantom), P, N, D.  `label` names the scene
    inside its family.  cu_shade has no phantom: real() is the list without its phantom cases."""

    def __init__(self, scene, idx, P, N, D, label=""):
        self.scene, self.js, self.label = scene, scene.js, label
        self.idx = np.ascontiguousarray(idx, I32)
        self.P = np.ascontiguousarray(P, F32).reshape(-1, 3)
        self.N = np.ascontiguousarray(N, F32).reshape(-1, 3)
        self.D = np.ascontiguousarray(D, F32).reshape(-1, 3)
        assert len(self.idx) == len(self.P) == len(self.N) == len(self.D)

    def __len__(self):
        return len(self.idx)

    def take(self, mask):
        return ShadeCases(self.scene, self.idx[mask], self.P[mask], self.N[mask], self.D[mask],
                          self.label)

    def real(self):
        return self if (self.idx >= 0).all() else self.take(self.idx >= 0)


def _cross(*arrays):
    """Every combination of the rows of the given arrays, as a list of equally long arrays."""
    lens = [len(a) for a in arrays]
    grid = np.meshgrid(*[np.arange(k) for k in lens], indexing="ij")
    return [np.asarray(a)[g.ravel()] for a, g in zip(arrays, grid)]


def unit32(v):
    with np.errstate(all="ignore"):                      # a zero vector gives NaN: a case like any other
        return pc.unit(np.asarray(v, F64)).astype(F32)


def _rand_units(rng, n):
    return unit32(rng.normal(size=(n, 3)))


# ------------------------------------------------------------------------------ lit --
def _reflect_dirs(D, N):
    """Unit bounce directions (any unit vector will do: only the oracle's frames are bit-exact)."""
    D, N = D.astype(F64), N.astype(F64)
    r = D - N * (2.0 * (D * N).sum(1, keepdims=True))
    ln = np.linalg.norm(r, axis=1, keepdims=True)
    return (r / np.where(ln > 0, ln, 1.0)).astype(F32)


@functools.lru_cache(None)
def family_lit():
    """Hit frames the oracle computes (rco_prim_nearest) for each scene's 64 x 48 camera rays, for
    the rays reflected off those hits and for random unit rays leaving them: every golden scene,
    random14x, random64, random65, lights0/3/6."""
    rng = np.random.default_rng(2121)
    out = []
    for name, sc in lit_scenes().items():
        d = camera_dirs(sc.js)
        O = np.zeros_like(d)
        idx, t, P, N, z = pc.ref_nearest(sc.js, O, d, np.full(len(d), -1, I32))
        h = idx >= 0
        I, Ps, Ns, Ds = [idx[h]], [P[h]], [N[h]], [d[h]]
        for dirs in (_reflect_dirs(d[h], N[h]), _rand_units(rng, int(h.sum()))):
            i2, t2, P2, N2, z2 = pc.ref_nearest(sc.js, P[h], dirs, idx[h])
            h2 = i2 >= 0
            I.append(i2[h2]), Ps.append(P2[h2]), Ns.append(N2[h2]), Ds.append(dirs[h2])
        I, Ps, Ns, Ds = (np.concatenate(a) for a in (I, Ps, Ns, Ds))
        keep = np.arange(len(I))[:: max(1, len(I) // 4000)]
        out.append(ShadeCases(sc, I[keep], Ps[keep], Ns[keep], Ds[keep], name))
    return out


# ----------------------------------------------------------------------- terminator --
def _occluder(mid):
    return dict(pc._sph(tuple(float(v) for v in mid), 0.25))


@functools.lru_cache(None)
def family_terminator():
    """N perpendicular to ld exactly, and each component of N moved by -4 .. 4 ulps: th = +-0, the
    smallest positive and negative values, NaN.  The light is at the origin and P = -v, so ld = v
    exactly before it is normalised.  Three lights (one scene each): ordinary radial coefficients,
    all three 0 (rad = inf), and (-2, 1, 0), which cancel at dist = 2 (rad = inf).  Each with and
    without a sphere on the shadow ray."""
    rng = np.random.default_rng(3030)
    vs = np.array([[2, 0, 0], [0, 0, -2], [0, 2, 0], [-2, 0, 0], [1.2, 0, 1.6], [3, 0, 0],
                   [0.5, -0.25, 1.0]], F32)
    rows = []
    for v in vs:
        vd = v.astype(F64)
        # exact perpendiculars: axis vectors for the axis-parallel v, and cross products rounded
        perp = [np.cross(vd, a) for a in np.eye(3) if np.linalg.norm(np.cross(vd, a)) > 0]
        perp += [np.cross(vd, r) for r in rng.normal(size=(6, 3))]
        for q in perp:
            n0 = unit32(q)
            ks = np.concatenate([np.zeros((1, 3), np.int64), rng.integers(-4, 5, (10, 3)),
                                 np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1],
                                           [0, 0, -1]])])
            for nn in pc.nudge32(np.repeat(n0[None], len(ks), 0), ks):
                rows.append((-v, nn))
                rows.append((-v, -nn))
        for bad in ([NAN, 0, 0], [0, NAN, 0], [0, 0, NAN], [NAN, NAN, NAN], [1, NAN, -1], [NAN, 1, 0]) * 8:
            rows.append((-v, np.array(bad, F32)))
    P = np.array([r[0] for r in rows], F32)
    N = np.array([r[1] for r in rows], F32)
    D = _rand_units(rng, len(P))
    out = []
    for lname, radial in (("radial", (0.0125, 0.0125, 0.01)), ("rad_zero", (0.0, 0.0, 0.0)),
                          ("rad_cancel", (-2.0, 1.0, 0.0))):
        for occ in (False, True):
            for spot in (False, True):
                light = dict(pos=(0.0, 0.0, 0.0), radial=radial)
                if spot:
                    light.update(spot=True, cos_theta=-1.0, a0=-1.0, dir=(0.0, 0.0, -1.0))
                # one occluder per distinct v: half-way between P and the light
                shapes = [_FAR] + ([_occluder(-0.5 * v) for v in vs] if occ else [])
                sc = LitScene(shapes, [light])
                out.append(ShadeCases(sc, np.zeros(len(P), I32), P, N, D,
                                      f"{lname}{'/occluded' if occ else ''}{'/spot' if spot else ''}"))
    return out


# ------------------------------------------------------------------------- on_light --
@functools.lru_cache(None)
def family_on_light():
    """P equal to a light's position bit for bit: a point light (one zero-normalize event) and a
    spot light (two events: the shadow ray has D = +0, and no shape test of the reference accepts
    such a ray — a sphere's and a quadric's t is 0 / 0 or c / 0, a plane's den is 0 — so a light
    P sits on is never shadowed), in a scene where nothing is in the way and in one where each
    light sits inside a sphere; and points a thousandth away."""
    rng = np.random.default_rng(4040)
    A, B = (1.5, 2.25, -3.0), (-2.0, 0.5, -6.0)
    lights = [dict(pos=A), dict(pos=B, spot=True, cos_theta=-1.0, a0=2.0, dir=(0.0, -1.0, 0.0)),
              dict(pos=(4.0, 6.0, 1.0))]
    out = []
    for inside in (False, True):
        shapes = [_FAR] + ([dict(pc._sph(A, 1.0)), dict(pc._sph(B, 1.0))] if inside else [])
        sc = LitScene(shapes, lights)
        m = 96
        P = np.concatenate([np.repeat(np.array([A], F32), m, 0), np.repeat(np.array([B], F32), m, 0),
                            np.array([A], F32) + rng.normal(size=(m // 2, 3)).astype(F32) * F32(1e-3)])
        N, D = _rand_units(rng, len(P)), _rand_units(rng, len(P))
        out.append(ShadeCases(sc, np.zeros(len(P), I32), P, N, D, "inside" if inside else "free"))
    return out


# ----------------------------------------------------------------------------- cone --
CONE_EXPONENTS = [0, 1, 2, -1, -3, -9, 3, 20, 31, 64, -64]
CONE_COS = [0.5, 0.0, -0.5, 1.0]           # 60 degrees, exactly 90, 120, and theta = 0
CONE_DIRS = [(0.0, 0.0, -1.0), (-0.0, -0.0, -3.0), (0.0, 0.0, -1e-20), (-0.0, 0.0, -1e20),
             (0.0, -0.0, -3e38), (1.0, 1.0, 0.0)]


def _cone_points(rng, c, L):
    """P - L for one cone: a sweep across the cone's edge (alpha = cos_theta and 1 .. 2 ulps either
    side, for a unit direction along -z), points with P - L perpendicular to -z and to (1, 1, 0)
    (alpha = +-0, zero components of either sign and products that cancel), points behind the
    light (alpha < 0), the axis, and random ones."""
    rel = []
    if c > 0:
        x0 = F32(np.sqrt(max(1.0 / (c * c) - 1.0, 0.0)))
        xs = pc.nudge32(np.full(65, x0, F32), np.arange(-32, 33))
        rel += [[x, 0.0, -1.0] for x in xs] + [[0.0, x, -1.0] for x in xs[::4]]
    zs = [0.0, -0.0, 1.0, -1.0, 0.5, -3.0]
    rel += [[x, y, z] for x in zs for y in zs for z in (0.0, -0.0)]
    rel += [[k, -k, z] for k in (1.0, -1.0, 0.75, -2.5) for z in (0.0, -1.0, 1.0, -0.0)]
    rel += [[x, y, z] for x in (0.0, 0.3, -0.3) for y in (0.0, -0.0, 0.4) for z in (1.0, 0.25, 3.0)]
    rel += [[0.0, 0.0, -2.0], [-0.0, 0.0, -2.0], [0.0, 0.0, 2.0], [0.0, 0.0, -1e-30]]
    rel = np.concatenate([np.array(rel, F32), (rng.normal(size=(16, 3)) * 2).astype(F32)])
    return (rel + np.array(L, F32)).astype(F32)           # a zero component of rel stays one of P - L


@functools.lru_cache(None)
def family_cone():
    """One spot light a scene: every exponent x every cone x every direction (length 1, 3, 1e-20,
    1e20, 3e38, and (1, 1, 0) for products that cancel).  The light is at (0, 0, 0) or (1, 2, -4); a
    component in which P equals the light's position is +0 in P - L.pos and in L.pos - P alike."""
    rng = np.random.default_rng(5050)
    out = []
    for a0 in CONE_EXPONENTS:
        for c in CONE_COS:
            for k, d in enumerate(CONE_DIRS):
                L = (0.0, 0.0, 0.0) if (k + len(out)) % 2 == 0 else (1.0, 2.0, -4.0)
                sc = LitScene([_FAR], [dict(pos=L, spot=True, cos_theta=c, a0=float(a0), dir=d)])
                P = _cone_points(rng, c, L)
                ld = unit32(np.array(L, F64) - P.astype(F64) + 1e-300)
                N = np.where(rng.uniform(size=(len(P), 1)) < 0.7, ld, _rand_units(rng, len(P)))
                out.append(ShadeCases(sc, np.zeros(len(P), I32), P, N.astype(F32),
                                      _rand_units(rng, len(P)), f"a0={a0} cos={c} dir={d}"))
    return out


GENERAL_EXPONENTS = [2.5, 7.25, -0.5, 65.0, 100.0, -65.0]    # none an integer of |a0| <= 64


@functools.lru_cache(None)
def family_cone_general():
    """family_cone's scenes and points under the exponents the packer does NOT treat as small
    integers (non-integers, and integers just past its bound of 64): shade's general branch, which
    calls the device library's pow."""
    rng = np.random.default_rng(6161)
    out = []
    for a0 in GENERAL_EXPONENTS:
        for c in CONE_COS:
            for k, d in enumerate(CONE_DIRS):
                L = (0.0, 0.0, 0.0) if (k + len(out)) % 2 == 0 else (1.0, 2.0, -4.0)
                sc = LitScene([_FAR], [dict(pos=L, spot=True, cos_theta=c, a0=float(a0), dir=d)])
                P = _cone_points(rng, c, L)
                ld = unit32(np.array(L, F64) - P.astype(F64) + 1e-300)
                N = np.where(rng.uniform(size=(len(P), 1)) < 0.7, ld, _rand_units(rng, len(P)))
                out.append(ShadeCases(sc, np.zeros(len(P), I32), P, N.astype(F32),
                                      _rand_units(rng, len(P)), f"a0={a0} cos={c} dir={d}"))
    return out


def cone_alpha(c):
    """alpha of every case of a list whose scene has ONE light, a spot light (C/raycast.c:679-694):
    dot(normalize(P - L.pos), direction) in numpy's float32 arithmetic, with the oracle's normalize
    (the length is the float of a double square root; a zero length leaves the vector).  Returns
    (alpha, cos_theta, a0)."""
    L = c.js.lights_list.contents
    assert c.js.num_lights == 1 and L.type == SPOT
    v = c.P - np.array(list(L.position), F32)
    s = v[:, 0].astype(F64) * v[:, 0].astype(F64)
    s = s + v[:, 1].astype(F64) * v[:, 1].astype(F64)
    s = s + v[:, 2].astype(F64) * v[:, 2].astype(F64)
    with np.errstate(all="ignore"):
        ln = np.sqrt(s).astype(F32)
        v = np.where((ln == 0)[:, None], v, v / ln[:, None]).astype(F32)
        d = np.array(list(L.direction), F32)
        a = v[:, 0] * d[0]
        a = a + v[:, 1] * d[1]
        a = a + v[:, 2] * d[2]
    assert a.dtype == F32
    return a, F32(L.cos_theta), F32(L.a0)


@functools.lru_cache(None)
def family_pow_general():
    """(alpha, a0) for the scalar probe of the same expression, (float)pow((double)alpha,
    (double)a0), device library against glibc: alpha over [0, 1]
    (inside a cone), above 1 (an unnormalised direction), negative, +-0, tiny, huge, inf, NaN."""
    rng = np.random.default_rng(6060)
    al = np.concatenate([rng.uniform(0, 1, 2500), rng.uniform(1, 4, 300), -rng.uniform(0, 2, 200),
                         np.ldexp(1.0, -np.arange(0, 40)), 1.0 - np.ldexp(1.0, -np.arange(1, 25)),
                         [0.0, -0.0, 1e-30, 1e-45, 1e20, 3e38, INF, -INF, NAN, 1.0, -1.0]]).astype(F32)
    A, E = _cross(al, np.array(GENERAL_EXPONENTS, F32))
    return A.astype(F32), E.astype(F32)


# --------------------------------------------------------------------------- radial --
@functools.lru_cache(None)
def family_radial():
    """One point light at the origin a scene; radial coefficients whose denominator crosses zero
    (negative ones), r2 * dist^2 beyond float but not double, dist at 1e19 and beyond float (3e38
    in each component), and a linear part that rounds differently in float and in double."""
    rng = np.random.default_rng(7070)
    coefs = [(-2.0, 1.0, 0.0), (-4.0, 0.0, 1.0), (1.0, -1.0, 0.25), (0.0, 0.0, 3e38), (0.1, 0.7, 0.3),
             (3e38, 3e38, 0.0), (0.0, 0.0, 0.0), (-0.0125, 0.0125, -0.01), (1e-45, 0.0, 1e-45)]
    u = _rand_units(rng, 40)
    dist = np.concatenate([pc.nudge32(np.full(33, 2.0, F32), np.arange(-16, 17)),
                           np.array([1.0, 0.5, 1e-3, 1e10, 1e19, 1e-20, 3.0], F32)])
    ax = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1]], F32)
    P = np.concatenate([-(ax[:, None, :] * dist[None, :, None]).reshape(-1, 3),
                        -(u[:, None, :] * dist[None, ::3, None]).reshape(-1, 3),
                        np.array([[3e38, 3e38, 3e38], [-3e38, 1e19, 0], [1e19, 1e19, -1e19]], F32)])
    P = P.astype(F32)
    N = unit32(-P.astype(F64) + 1e-300)
    N[::5] = _rand_units(rng, len(N[::5]))
    D = _rand_units(rng, len(P))
    return [ShadeCases(LitScene([_FAR], [dict(pos=(0.0, 0.0, 0.0), radial=c)]),
                       np.zeros(len(P), I32), P, N, D, f"radial={c}") for c in coefs]


# ------------------------------------------------------------------------- specular --
@functools.lru_cache(None)
def family_specular():
    """dot(view, reflect(ld, N)) exactly +-0, the smallest magnitudes of both signs, and > 0; N, D
    unit within rounding, the exact zero vector, and NaN-carrying; a surface whose specular colour
    is 0 (sl = 0 times the power) beside an ordinary one."""
    rng = np.random.default_rng(8080)
    # light straight above P = 0: ld = (0, 1, 0), N = (0, 1, 0) gives reflect = (0, -1, 0) and
    # angle = D.y: its sign and size are D's
    tiny = pc.nudge32(np.zeros(17, F32), np.arange(-8, 9))
    Dy = np.concatenate([tiny, np.array([0.0, -0.0, 1e-38, -1e-38, 1e-20, -1e-20, 0.5, -0.5, 1.0, -1.0],
                                        F32)])
    rows = [((0, 0, 0), (0, 1, 0), (1, y, 0)) for y in Dy] + [((0, 0, 0), (0, 1, 0), (0, y, -1)) for y in Dy]
    for bad in ([0, 0, 0], [NAN, 0, 1], [0, NAN, 0], [NAN, NAN, NAN]):
        rows += [((0, 0, 0), bad, (0, -1, 0)), ((0, 0, 0), (0, 1, 0), bad), ((0.5, 1, -2), bad, bad)]
    P = np.array([r[0] for r in rows], F32)
    N = np.array([r[1] for r in rows], F32)
    D = np.array([r[2] for r in rows], F32)
    m = 1500
    Pr = (rng.normal(size=(m, 3)) * [2, 0.5, 2]).astype(F32)
    Nr = unit32(rng.normal(size=(m, 3)) * [0.4, 0.4, 0.4] + [0, 1, 0])
    Dr = _rand_units(rng, m)
    P, N, D = np.concatenate([P, Pr]), np.concatenate([N, Nr]), np.concatenate([D, Dr])
    out = []
    for name, spec in (("specular", (0.5, 0.7, 0.9)), ("sl=0", (0.0, 0.0, -0.0))):
        shape = dict(_FAR, specular=spec)
        sc = LitScene([shape], [dict(pos=(0.0, 5.0, 0.0)), dict(pos=(3.0, 4.0, -1.0), color=(0.5, 2.0, 1.0))])
        out.append(ShadeCases(sc, np.zeros(len(P), I32), P, N, D, name))
    return out


# -------------------------------------------------------------------------- opacity --
@functools.lru_cache(None)
def family_opacity():
    """refl + refr equal to 1 exactly, 1 -+ an ulp, above 1, NaN and negative; and the phantom
    record (index -1) of phantom_two and phantom_four (lit phantoms), of the quadric scene with its
    light moved so that the phantom is lit (helpers.phantom_lit_scene) and of a golden scene whose
    phantom is black."""
    rng = np.random.default_rng(9090)
    one_m, one_p = float(np.nextafter(F32(0.5), F32(0))), float(np.nextafter(F32(0.5), F32(1)))
    pairs = [(0.5, 0.5), (0.5, one_m), (0.5, one_p), (0.75, 0.75), (NAN, 0.0), (0.0, NAN),
             (-0.5, 0.0), (0.0, 0.0), (1.0, 0.0), (1.0, -1e-8), (INF, 0.0), (-INF, 0.0)]
    shapes = [dict(_FAR, position=(0.0, -1000.0 - k, 0.0), refl=a, refr=b) for k, (a, b) in enumerate(pairs)]
    sc = LitScene(shapes, [dict(pos=(2.0, 6.0, 1.0)), dict(pos=(-3.0, 4.0, -5.0), color=(0.5, 2.0, 1.0))])
    m = 24
    idx = np.repeat(np.arange(len(pairs), dtype=I32), m)
    P = (rng.normal(size=(len(idx), 3)) * 2).astype(F32)
    N = unit32(rng.normal(size=(len(idx), 3)) * 0.3 + [0, 1, 0])
    out = [ShadeCases(sc, idx, P, N, _rand_units(rng, len(idx)), "opacity")]
    from helpers import phantom_lit_scene
    if not _TMP:
        _TMP.append(tempfile.TemporaryDirectory())
    scenes = {"phantom_two": rc.Scene.from_file(scene_path("phantom_two")),
              "phantom_four": rc.Scene.from_file(scene_path("phantom_four")),
              "phantom_lit": rc.Scene.from_file(phantom_lit_scene(
                  os.path.join(_TMP[0].name, "phantom_lit.scene"), "four-lights")),
              "reflection": rc.Scene.from_file(scene_path("reflection"))}
    for name, s in scenes.items():
        k = 300
        P = (rng.normal(size=(k, 3)) * [4, 3, 4] + [0, 0, -6]).astype(F32)
        P[:10] = 0.0                                               # the first carry of a frame
        idx = np.full(k, -1, I32)
        idx[k // 2:: 7] = 0                                        # a real shape among them
        out.append(ShadeCases(s, idx, P, _rand_units(rng, k), _rand_units(rng, k), name))
    return out


# ------------------------------------------------------------------------ nonfinite --
@functools.lru_cache(None)
def family_nonfinite():
    """inf / NaN components in P and in light positions; lights at 3e38."""
    rng = np.random.default_rng(1212)
    lights = [dict(pos=(3e38, 3e38, -3e38)), dict(pos=(INF, 1.0, 0.0), color=(0.5, 2.0, 1.0)),
              dict(pos=(0.0, NAN, 2.0)), dict(pos=(1.0, 5.0, -2.0)),
              dict(pos=(-3e38, 1.0, 0.0), spot=True, cos_theta=-0.5, a0=3.0, dir=(1.0, 0.0, 0.0))]
    out = []
    m = 600
    P = (rng.normal(size=(m, 3)) * 3).astype(F32)
    bad = np.array([INF, -INF, NAN, 3e38, -3e38], F32)
    for r in range(m // 2):
        P[r, r % 3] = bad[(r // 3) % 5]
    N = unit32(rng.normal(size=(m, 3)) * 0.3 + [0, 1, 0])
    D = _rand_units(rng, m)
    for k in range(len(lights)):
        sc = LitScene([_FAR, dict(pc._sph((0.0, 2.0, -1.0), 0.5))], [lights[k], lights[3]])
        out.append(ShadeCases(sc, np.zeros(m, I32), P, N, D, f"light{k}"))
    out.append(ShadeCases(LitScene([_FAR], lights), np.zeros(m, I32), P, N, D, "all"))
    return out


SHADE_FAMILIES = {"lit": family_lit, "terminator": family_terminator, "on_light": family_on_light,
                  "cone": family_cone, "cone_general": family_cone_general, "radial": family_radial, "specular": family_specular,
                  "opacity": family_opacity, "nonfinite": family_nonfinite}


def family_size(name):
    return sum(len(c) for c in SHADE_FAMILIES[name]())


_REF = {}


def shade_reference(name, cuda=False):
    """[(rgb, zero)] per case list of a family (cuda: of its real() cases) and the family's summed
    counters; computed once."""
    key = (name, cuda)
    if key not in _REF:
        res, total = [], None
        for c in SHADE_FAMILIES[name]():
            if cuda:
                c = c.real()                              # cu_shade has no phantom
            rgb, zero, cnt = ref_shade(c.js, c.idx, c.P, c.N, c.D, cuda=cuda)
            rgb.setflags(write=False), zero.setflags(write=False)
            res.append((rgb, zero))
            total = cnt if total is None else add_counts(total, cnt)
        _REF[key] = (res, total)
    return _REF[key]


# ---------------------------------------------------------------------------- shoot --
class ShootCases:
    def __init__(self, scene, d, carry, maxrec, label):
        self.scene, self.js, self.label, self.maxrec = scene, scene.js, label, int(maxrec)
        self.d = np.ascontiguousarray(d, F32).reshape(-1, 3)
        self.carry = np.ascontiguousarray(carry, F32).reshape(-1, 3)
        assert len(self.d) == len(self.carry)

    def __len__(self):
        return len(self.d)


def camera_dirs(js, W=64, H=48):
    return pc.primary_dirs(js.camera_width, js.camera_height, W, H)


def camera_dirs_cuda(js, W=64, H=48):
    """The CUDA port's primary rays (CUDA/raycast.cu:154-158): the same d.x, d.y, then its
    normalize, whose sum of squares is a float sum."""
    cw, ch = F32(js.camera_width), F32(js.camera_height)
    pw, ph = cw / F32(W), ch / F32(H)
    x, y = np.meshgrid(np.arange(W, dtype=F64), np.arange(H, dtype=F64))
    dx = ((0.0 - F64(cw) / 2.0) + F64(pw) * (x + 0.5)).astype(F32).ravel()
    dy = ((0.0 + F64(ch) / 2.0) - F64(ph) * (y + 0.5)).astype(F32).ravel()
    dz = np.full(len(dx), -1.0, F32)
    s = dx * dx
    s = s + dy * dy
    s = s + dz * dz
    ln = np.sqrt(s.astype(F64)).astype(F32)
    return np.stack([dx / ln, dy / ln, dz / ln], 1).astype(F32)


def scan_carries(js, d, maxrec):
    """The oracle's own scan-order carry-ins of the rays d under parity: pixel i starts from the
    carry pixel i - 1 left."""
    n = len(d)
    cin = np.zeros((n, 3), F32)
    c = np.zeros((1, 3), F32)
    for i in range(n):
        cin[i] = c[0]
        _, _, c, _, _ = ref_shoot(js, d[i:i + 1], maxrec, "parity", c)
    return cin


def _mirror_scene(refl_a, refl_b, lights=True):
    """Two facing mirrors (planes z = -4 and z = 1 around the camera) and a sphere between them."""
    shapes = [dict(pc._pln((0.0, 0.0, -4.0), (0.0, 0.0, 1.0)), refl=refl_a),
              dict(pc._pln((0.0, 0.0, 1.0), (0.0, 0.0, -1.0)), refl=refl_b),
              dict(pc._sph((0.6, -0.4, -2.5), 0.5), refl=0.4, refr=0.1),
              dict(pc._pln((0.0, -1.0, 0.0), (0.0, 1.0, 0.0)), refl=0.0)]
    li = [dict(pos=(0.5, 3.0, -1.0)), dict(pos=(-2.0, 5.0, 6.0), color=(0.6, 0.7, 2.0))] if lights else []
    return LitScene(shapes, li)


@functools.lru_cache(None)
def family_shoot():
    """Primary directions of the 64 x 48 camera of every golden scene, random14x, random64 (the
    reflectivity mask's last bit) and random65 (reflective() reads the record), two
    facing mirrors (the loop runs to maxrec) with reflectivities 0, -0.5, 1, 1.5 and NaN, and the
    mirrors without lights (m = 0); maxrec 1, 2, 3, 6, 7.  Carry-ins: zeros, the oracle's own
    scan-order carries (every 16th row) and points inside a shape."""
    rng = np.random.default_rng(1313)
    out = []
    scenes = {k: v for k, v in lit_scenes().items() if not k.startswith("lights")}
    recs = {"simple": (7, 2), "reflection": (7, 3), "quadric": (7, 1), "example2": (6,), "example3": (3,),
            "quadric2": (7,), "random14x": (7, 2), "random65": (7,), "random64": (7,)}
    for name, sc in scenes.items():
        d = camera_dirs(sc.js)
        for mr in recs[name]:
            sel = d if mr == 7 else d[::3]
            carry = np.zeros_like(sel)
            if mr == 7 and name in ("reflection", "quadric", "random14x"):
                rows = sel.reshape(48, 64, 3)[::16].reshape(-1, 3)          # three whole rows
                out.append(ShootCases(sc, rows, scan_carries(sc.js, rows, mr), mr, f"{name}/scan"))
                inside = (rng.normal(size=(len(rows), 3)) * 0.2 + [0, 0, -5]).astype(F32)
                out.append(ShootCases(sc, rows, inside, mr, f"{name}/inside"))
            out.append(ShootCases(sc, sel, carry, mr, f"{name}/d{mr}"))
    d = pc.primary_dirs(2.0, 2.0, 32, 24)
    for ra, rb in ((1.0, 1.0), (1.5, 0.75), (0.0, 1.0), (-0.5, 1.0), (NAN, 1.0), (1.0, NAN), (0.9, 0.0)):
        for mr in (6, 7, 2):
            out.append(ShootCases(_mirror_scene(ra, rb), d, np.zeros_like(d), mr, f"mirrors({ra},{rb})/d{mr}"))
    out.append(ShootCases(_mirror_scene(1.0, 0.5, lights=False), d, np.zeros_like(d), 7, "mirrors/m=0"))
    return out


CUDA_ITERS = (0, 1, 49)


# ---------------------------------------------------------------------------- quant --
@functools.lru_cache(None)
def family_quant():
    """c with c * 255 within 4 ulps of every integer 0 .. 256; +-0, subnormals, negatives, values
    above 1, 3e38, +-inf, NaNs of both signs with several payloads, and 2^15 random values."""
    rng = np.random.default_rng(1414)
    k = np.arange(0, 257, dtype=F64)
    base = (k / 255.0).astype(F32)
    near = pc.nudge32(np.repeat(base, 17), np.tile(np.arange(-8, 9), len(base)))
    nans = pc.f32_from_bits(np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff,
                                      0xffffffff, 0x7fc12345, 0xffa00000], np.uint32))
    spec = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38, -1.0, -0.5, 1.0, 1.5, 2.0, 3e38, -3e38,
                     INF, -INF, 1.0 / 255.0, 0.00392, 0.999999, 1.0000001, 8421504.0, 2.2e9 / 255], F32)
    rnd = np.concatenate([rng.uniform(-0.25, 1.25, 1 << 14), rng.normal(size=1 << 13) * 3,
                          np.ldexp(rng.uniform(1, 2, 1 << 13), rng.integers(-149, 128, 1 << 13))]).astype(F32)
    return np.concatenate([near, nans, spec, rnd]).astype(F32)


# ---------------------------------------------------------------------- primary_dir --
@functools.lru_cache(None)
def family_primary_dir():
    """(hx, hy, pw, ph, x, y) as the launchers form them (make_cam) for W x H from 1 x 1 through odd
    sizes and 8192^2 up to 33 554 433 x 33 554 431 and cameras 0.5 x 0.5 .. 2000 x 2000: the four
    corners, the centre pair and random pixels."""
    rng = np.random.default_rng(1515)
    sizes = [(1, 1), (2, 2), (3, 5), (64, 48), (65, 65), (127, 33), (1023, 767), (8192, 8192),
             (33554433, 33554431), (16777217, 3), (5, 16777216)]
    cams = [(0.5, 0.5), (2.0, 2.0), (2.0, 2.03125), (0.7, 1.3), (2000.0, 2000.0), (1e-3, 3.0)]
    rows = []
    for W, H in sizes:
        for cw, ch in cams:
            xs = np.concatenate([[0, W - 1, 0, W - 1, W // 2, max(W // 2 - 1, 0)], rng.integers(0, W, 26)])
            ys = np.concatenate([[0, 0, H - 1, H - 1, H // 2, max(H // 2 - 1, 0)], rng.integers(0, H, 26)])
            for x, y in zip(xs, ys):
                rows.append((cw, ch, W, H, int(x), int(y)))
    r = np.array(rows, F64)
    cw, ch = r[:, 0].astype(F32), r[:, 1].astype(F32)
    W, H = r[:, 2].astype(np.int64), r[:, 3].astype(np.int64)
    cam = np.stack([0.0 - cw.astype(F64) / 2.0, 0.0 + ch.astype(F64) / 2.0], 1)          # hx, hy
    pix = np.zeros((len(r), 4), F32)
    pix[:, 0] = cw / W.astype(F32)                                                        # pw
    pix[:, 1] = ch / H.astype(F32)                                                        # ph
    xy = np.stack([r[:, 4], r[:, 5]], 1).astype(I32)
    return np.ascontiguousarray(cam), pix, xy


def primary_dir_ref(cam, pix, xy):
    """C/raycast.c:115-118 in numpy's IEEE arithmetic with the oracle's normalize: the direction and
    its zero-normalize events (none: d.z = -1)."""
    pw, ph = pix[:, 0].astype(F64), pix[:, 1].astype(F64)
    dx = (cam[:, 0] + pw * (xy[:, 0].astype(F64) + 0.5)).astype(F32)
    dy = (cam[:, 1] - ph * (xy[:, 1].astype(F64) + 0.5)).astype(F32)
    dz = np.full(len(dx), -1.0, F32)
    s = dx.astype(F64) * dx.astype(F64)
    s = s + dy.astype(F64) * dy.astype(F64)
    s = s + dz.astype(F64) * dz.astype(F64)
    with np.errstate(over="ignore"):
        ln = np.sqrt(s).astype(F32)
    return np.stack([dx / ln, dy / ln, dz / ln], 1).astype(F32), np.zeros(len(dx), I32)
