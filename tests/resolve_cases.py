"""Cases of the entry-level tests of the carry resolver ("Entry-level tests of the carry
resolver"): shared by tests/test_resolve_cases.py (CPU: the edges are where the lists say they
are) and tests/test_gpu_resolve.py (device against the oracle).  Seeded; the references are the
CPU oracle's alone.

An evaluator case is (scene, primary direction d, carry-in c, maxrec); its reference is
rco_prim_shoot(d, maxrec, parity, c): class 3 <=> the hit flag, carry-out = f_p(c).  A chain is
(scene, directions, initial carry, maxrec); its reference is that call iterated entry by entry,
the carry after entry k being entry k + 1's carry-in."""
import ctypes
import functools

import numpy as np

import prim_cases as pc
import shade_cases as sc
from helpers import RcoStats, oracle_lib, rc, scene_path

F32, F64, U32, I32, U8 = np.float32, np.float64, np.uint32, np.int32, np.uint8
MAX_CASES = 1 << 16            # per evaluator family
MAXRECS = (2, 3, 4, 7, 8)      # 2: no level at all; odd and even level counts
PARITY = rc.MODES["parity"]


# ------------------------------------------------------------------------- the oracle --
def render_cls(scene, W, H, maxrec):
    """rco_render_cls: (image, class per pixel [W*H], carry-in per pixel [W*H, 3])."""
    lib = oracle_lib()
    lib.rco_render_cls.argtypes = lib.rco_render.argtypes + [ctypes.c_void_p]
    img = np.empty((H, W, 3), U8)
    cin, cls, st = np.zeros((H * W, 3), F32), np.zeros(H * W, U8), RcoStats()
    r = lib.rco_render_cls(ctypes.byref(scene.js), W, H, int(maxrec), PARITY, img.ctypes.data_as(ctypes.c_void_p),
                           ctypes.byref(st), cin.ctypes.data_as(ctypes.c_void_p),
                           cls.ctypes.data_as(ctypes.c_void_p))
    assert r == 0
    return img, cls, cin


def shoot(js, d, carry, maxrec):
    """rco_prim_shoot under parity: (carry-out [n, 3], hit flag [n] = class 3, class [n])."""
    d, carry = np.ascontiguousarray(d, F32), np.ascontiguousarray(carry, F32)
    _, cls, cout, _, _ = sc.ref_shoot(js, d, maxrec, "parity", carry)
    return cout, cls == 3, cls


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_rows(a, b):
    """Row by row: all three components the same bits."""
    return (bits(a) == bits(b)).reshape(len(a), 3).all(1)


def same_nan(a, b):
    """Row by row, the suite's convention: the same bits, or a NaN on both sides (a generated
    NaN's sign is the hardware's); -0 is not +0."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return ((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).reshape(len(a), 3).all(1)


def nudge(x, k):
    """x moved k float steps in bit space (the creep's own unit)."""
    return (bits(x).astype(np.int64) + k).astype(U32).view(F32)


# -------------------------------------------------------------------------- the scenes --
DEGENERATE = {
    "mirror-box": "".join(
        f"plane, normal: [{n}], diffuse_color: [0.4, 0.5, 0.6], specular_color: [1, 1, 1], "
        f"position: [{p}], reflectivity: 0.9\n"
        for n, p in (("0, 1, 0", "0, -2, 0"), ("0, -1, 0", "0, 2, 0"), ("1, 0, 0", "-2, 0, 0"),
                     ("-1, 0, 0", "2, 0, 0"), ("0, 0, 1", "0, 0, -8"))),
    "lone-mirror-plane": "plane, normal: [0, 0.6, 0.8], diffuse_color: [0.2, 0.7, 0.3], "
                         "specular_color: [1, 1, 1], position: [0, 0, -6], reflectivity: 1.0\n",
    "full-reflect-sphere": "sphere, radius: 2.0, diffuse_color: [0, 0, 1], specular_color: "
                           "[1, 1, 1], position: [0, 0, -6], reflectivity: 1.0, refractivity: 0, ior: 1\n",
}
_LIGHT = ("light, color: [1.5, 1.2, 1.0], radial-a2: 0.01, radial-a1: 0.0125, radial-a0: 0.0125, "
          "position: [3, 6, 1]\n")
GOLDEN = ["simple", "reflection", "quadric", "example2", "example3", "quadric2", "phantom_two", "phantom_four"]
RANDOM = [("random14", 14, False), ("random14x", 14, True), ("random20", 20, False), ("random20x", 20, True),
          ("random33", 33, False), ("random33x", 33, True), ("random64", 64, False), ("random64x", 64, True),
          ("random65", 65, False), ("random65x", 65, True)]


@functools.lru_cache(None)
def scenes():
    """name -> rc.Scene: the eight golden scenes, random scenes of 14, 20, 33, 64 and 65 shapes with
    and without cross terms, the degenerate texts and the tie scenes."""
    out = {n: rc.Scene.from_file(scene_path(n)) for n in GOLDEN}
    for name, n, cross in RANDOM:
        out[name] = sc.random_unit_scene("resolve_" + name, 7000 + n + (500 if cross else 0), n, cross=cross)
    for name, text in DEGENERATE.items():
        out[name] = sc._text_scene("resolve_" + name, "camera, width: 2.0, height: 2.0\n" + text + _LIGHT)
    out.update(tie_scenes())
    return out


def n_shapes(scene):
    return int(scene.js.num_shapes)


def reflectivity(js):
    out, p = [], js.shapes_list
    while p:
        s = p.contents
        out.append(s.reflectivity)
        p = ctypes.cast(s.next, ctypes.POINTER(rc.ShapeT))
    return np.array(out, F32)


TIE_PAIRS = (0, 3, 7, 15)    # the duplicate sits at p, p + 1: across a quad's lanes 0/1, a quad
                             # boundary 3/4, an 8-lane half 7/8 and a 16-lane row 15/16 (with G = 16
                             # the two speculative halves of an entry)


def _filler(k):
    return (f"sphere, diffuse_color: [0.5, 0.5, 0.5], specular_color: [0.2, 0.2, 0.2], position: "
            f"[{30 + 3 * k}, 40, 30], radius: 1, reflectivity: 0.1, refractivity: 0, ior: 1.5")


def tie_scenes():
    """The quadric example with one of its shapes twice, at the list positions p and p + 1 (the
    others behind small spheres out of every ray's way): the two see the same t bit for bit and the
    lower index must win.  One copy is matte (reflectivity 0), first or second: the winner decides
    whether the bounce loop goes on."""
    lines = open(scene_path("quadric")).read().splitlines()
    cam, shapes = lines[0], [ln for ln in lines[1:] if not ln.startswith("light")]
    lights = [ln for ln in lines if ln.startswith("light")]
    out = {}
    for p in TIE_PAIRS:
        for which, matte_first in ((0, False), (1, True), (3, False), (2, True)):
            dup = shapes[which]
            head, refl = dup.rsplit("reflectivity:", 1)
            matte = head + "reflectivity: 0.0" + (refl[refl.index(","):] if "," in refl else "")
            pair = [matte, dup] if matte_first else [dup, matte]
            rest = [s for k, s in enumerate(shapes) if k != which]
            body = [_filler(k) for k in range(p)] + pair + rest
            body += [_filler(100 + k) for k in range(max(0, 17 - len(body)))]
            name = f"tie{p}-{which}{'m' if matte_first else 'r'}"
            out[name] = sc._text_scene("resolve_" + name, "\n".join([cam] + body + lights) + "\n")
    return out


# --------------------------------------------- the bounce levels, restated on the oracle --
def _dot(a, b):
    s = a[:, 0] * b[:, 0]
    s = s + a[:, 1] * b[:, 1]
    return s + a[:, 2] * b[:, 2]


def _reflect_norm(D, N):
    """normalize(reflect(D, N)) as C/v3math.c does them (oracle/rc_oracle.c o_reflect, o_normalize:
    float products and sums, the length through a double sum; a zero length leaves the vector)."""
    with np.errstate(all="ignore"):
        s = F32(2.0) * _dot(D, N)
        r = D - N * s[:, None]
        q = r.astype(F64)
        ss = q[:, 0] * q[:, 0]
        ss = ss + q[:, 1] * q[:, 1]
        ss = ss + q[:, 2] * q[:, 2]
        ln = np.sqrt(ss).astype(F32)
        return np.where((ln == 0)[:, None], r, r / ln[:, None]).astype(F32)


def levels(js, d, carry, maxrec):
    """The bounce loop of DEP entries level by level: o_shoot's control flow in numpy around the
    oracle's own o_nearest (rco_prim_nearest).  Returns (win [n, maxrec - 2]: the shape level
    2 + k hit, -1 a miss, -2 not run; carry-out [n, 3]; the rays of every level as a list of (O, D,
    S, run mask)).  A selection aid only: test_resolve_cases.py counts it against rco_prim_shoot."""
    d, C = np.ascontiguousarray(d, F32), np.ascontiguousarray(carry, F32).copy()
    n = len(d)
    refl = reflectivity(js)
    i0, _, P0, N0, _ = pc.ref_nearest(js, np.zeros_like(d), d, np.full(n, -1, I32))
    assert (i0 >= 0).all(), "a DEP entry has a primary hit"
    obj, N = i0.copy(), N0.copy()
    D = _reflect_norm(d, N)                        # level 1: it missed (the entry is DEP)
    alive = refl[obj] > 0
    win = np.full((n, max(0, maxrec - 2)), -2, I32)
    rays = []
    S = np.full(n, -1, I32)
    for lvl in range(2, maxrec):
        alive = alive & (refl[obj] > 0)
        D = np.where(alive[:, None], _reflect_norm(D, N), D)
        idx, _, P, Nn, _ = pc.ref_nearest(js, C, D, S)
        rays.append((C.copy(), D.copy(), S.copy(), alive.copy()))
        hit = alive & (idx >= 0)
        win[alive, lvl - 2] = idx[alive]
        C[hit], N[hit], obj[hit] = P[hit], Nn[hit], idx[hit]
        S = np.where(alive, idx, S).astype(I32)
    return win, C, rays


# ------------------------------------------------------------------ evaluator families --
class EvalCases:
    def __init__(self, scene, d, carry, maxrec, label):
        self.scene, self.js, self.label, self.maxrec = scene, scene.js, label, int(maxrec)
        self.d = np.ascontiguousarray(d, F32).reshape(-1, 3)
        self.carry = np.ascontiguousarray(carry, F32).reshape(-1, 3)
        assert len(self.d) == len(self.carry)

    def __len__(self):
        return len(self.d)

    @functools.cached_property
    def ref(self):
        """(carry-out, hit flag, class) of the oracle: computed once, shared, left unchanged."""
        out = shoot(self.js, self.d, self.carry, self.maxrec)
        for a in out:
            a.setflags(write=False)
        return out


CAMERAS = ((64, 48), (96, 72))
SCAN_SCENES = GOLDEN + [n for n, _, _ in RANDOM]


@functools.lru_cache(None)
def scan_pixels(name, W, H, maxrec):
    """(d, carry-in) of the DEP pixels of one oracle frame, in scan order, and the frame's classes."""
    s = scenes()[name]
    _, cls, cin = render_cls(s, W, H, maxrec)
    d = pc.primary_dirs(s.js.camera_width, s.js.camera_height, W, H)
    dep = cls >= 2
    return d[dep], cin[dep], cls


@functools.lru_cache(None)
def family_scan():
    """DEP pixels of the 64 x 48 and 96 x 72 cameras of the eight golden scenes and the ten random
    scenes, each at the carry-in the oracle's scan gave it, maxrec 2, 3, 4, 7, 8.  Thinned evenly
    (every k-th pixel of a frame) to MAX_CASES."""
    frames = [(n, w, h, mr) for n in SCAN_SCENES for (w, h) in CAMERAS for mr in MAXRECS]
    total = sum(len(scan_pixels(*f)[0]) for f in frames)
    step = -(-total // (MAX_CASES - len(frames)))
    out = []
    for k, f in enumerate(frames):
        d, c, _ = scan_pixels(*f)
        if len(d):
            out.append(EvalCases(scenes()[f[0]], d[k % step::step], c[k % step::step], f[3],
                                 f"scan/{f[0]}/{f[1]}x{f[2]}/m{f[3]}"))
    return out


CREEP_SCENES = ("quadric", "reflection", "quadric2", "random14x", "random33", "random64x", "random65")


@functools.lru_cache(None)
def family_creep():
    """Carry-ins on a surface: the oracle's carry-out of an entry that hit (the stale point then
    re-hits its own shape at t ~ 0) fed back to the entry and to its scan-order neighbour, as it is
    and with each component moved -4 .. 4 float steps."""
    out = []
    for name in CREEP_SCENES:
        for mr in (7, 4):
            d, c, _ = scan_pixels(name, 64, 48, mr)
            cout, hit, _ = shoot(scenes()[name].js, d, c, mr)
            idx = np.flatnonzero(hit)[:90 if mr == 7 else 30]
            if not len(idx):
                continue
            D, C = [], []
            for src, dst in ((idx, idx), (idx, np.minimum(idx + 1, len(d) - 1))):
                base = cout[src]
                for comp in range(3):
                    for k in range(-4, 5):
                        if k == 0 and comp:
                            continue
                        v = base.copy()
                        v[:, comp] = nudge(v[:, comp], k)
                        D.append(d[dst])
                        C.append(v)
            out.append(EvalCases(scenes()[name], np.concatenate(D), np.concatenate(C), mr, f"creep/{name}/m{mr}"))
    assert sum(len(c) for c in out) <= MAX_CASES
    return out


PATTERNS = {"hit-miss-hit-miss": (1, 0, 1, 0), "miss-miss-hit": (0, 0, 1)}


def pattern_mask(win, pat):
    """Entries whose levels 2, 3, .. start with the hit (1) / miss (0) pattern, every level run."""
    if win.shape[1] < len(pat):
        return np.zeros(len(win), bool)
    m = np.ones(len(win), bool)
    for k, h in enumerate(pat):
        m &= (win[:, k] >= 0) if h else (win[:, k] == -1)
    return m


@functools.lru_cache(None)
def family_pattern():
    """The entries of `scan`, `creep`, `skip` and `tie` (maxrec 7 and 8) whose levels go hit / miss / hit / miss —
    the speculation's five levels in three steps — and miss / miss / hit, where the second group's
    result is used and then its successor's directions; selected by levels()."""
    out = []
    whole = [EvalCases(scenes()[n], *scan_pixels(n, 96, 72, mr)[:2], mr, f"whole/{n}/m{mr}")
             for n in SCAN_SCENES for mr in (7, 8)]      # the frames `scan` thinned, every pixel
    for pname, pat in PATTERNS.items():
        for cs in family_scan() + family_creep() + family_skip() + family_tie() + whole:
            if cs.maxrec < 7 or not len(cs) or (cs.label.startswith("whole") and pat[0]):
                continue
            win, _, _ = levels(cs.js, cs.d, cs.carry, cs.maxrec)
            m = pattern_mask(win, pat)
            if m.any():
                out.append(EvalCases(cs.scene, cs.d[m], cs.carry[m], cs.maxrec, f"pattern/{pname}/{cs.label}"))
    return out


@functools.lru_cache(None)
def family_tie():
    """The tie scenes' DEP pixels (64 x 48, maxrec 7 and 4) at their scan carry-ins and at the
    oracle's carry-outs fed back (the levels then start on the duplicated surface)."""
    out = []
    for name in tie_scenes():
        s = scenes()[name]
        for mr in (7, 4):
            d, c, _ = scan_pixels(name, 64, 48, mr)
            if not len(d):
                continue
            cout, _, _ = shoot(s.js, d, c, mr)
            out.append(EvalCases(s, np.concatenate([d, d]), np.concatenate([c, cout]), mr, f"tie/{name}/m{mr}"))
    assert sum(len(c) for c in out) <= MAX_CASES
    return out


def tie_levels(cs):
    """Per case: levels whose winner is the lower copy of the scene's pair while the upper copy, not
    skipped, has the same t bit for bit (the oracle's own shape test on the level's ray)."""
    p = int(cs.label.split("/")[1].split("-")[0][3:])
    win, _, rays = levels(cs.js, cs.d, cs.carry, cs.maxrec)
    count = np.zeros(len(cs), I32)
    for k, (O, D, S, run) in enumerate(rays):
        m = run & (win[:, k] == p) & (S != p + 1)
        if not m.any():
            continue
        n = int(m.sum())
        h0, t0, _ = pc.ref_shape(cs.js, O[m], D[m], np.full(n, p, I32), S[m])
        h1, t1, _ = pc.ref_shape(cs.js, O[m], D[m], np.full(n, p + 1, I32), S[m])
        tied = (h0 != 0) & (h1 != 0) & (bits(t0) == bits(t1))
        count[np.flatnonzero(m)[tied]] += 1
    return count


@functools.lru_cache(None)
def family_skip():
    """Carry-ins exactly on the entry's own primary shape and on another shape (the oracle's hit
    points of rays aimed at each shape), so that S — the shape skipped after a hit, none after a
    miss — decides the next level."""
    out = []
    for name in ("quadric", "reflection", "quadric2", "random14x", "random20"):
        s = scenes()[name]
        d, _, _ = scan_pixels(name, 64, 48, 7)
        if not len(d):
            continue
        d = d[:: max(1, len(d) // 400)]
        n = len(d)
        i0, _, P0, _, _ = pc.ref_nearest(s.js, np.zeros_like(d), d, np.full(n, -1, I32))
        rng = np.random.default_rng(4242)
        # points on the shapes: the primary hit points of the whole camera, by shape
        dd = pc.primary_dirs(s.js.camera_width, s.js.camera_height, 64, 48)
        ia, _, Pa, _, _ = pc.ref_nearest(s.js, np.zeros_like(dd), dd, np.full(len(dd), -1, I32))
        D, C = [d], [P0]                                    # on the entry's own obj0
        for k in np.unique(ia[ia >= 0]):
            pts = Pa[ia == k]
            D.append(d)
            C.append(pts[rng.integers(0, len(pts), n)])     # on shape k, own or another
        for mr in (7, 4):
            out.append(EvalCases(s, np.concatenate(D), np.concatenate(C), mr, f"skip/{name}/m{mr}"))
    assert sum(len(c) for c in out) <= MAX_CASES
    return out


NONFINITE = [np.inf, -np.inf, np.nan, -0.0, 3e38, -3e38]


@functools.lru_cache(None)
def family_nonfinite():
    """+-inf, NaN, -0 and 3e38 in one, two or all components of the carry-in."""
    out = []
    for name in ("quadric", "reflection", "random14x", "random33"):
        s = scenes()[name]
        d, c, _ = scan_pixels(name, 64, 48, 7)
        if not len(d):
            continue
        sel = np.arange(0, len(d), max(1, len(d) // 60))
        D, C = [], []
        for v in NONFINITE:
            for comps in ((0,), (1,), (2,), (0, 1), (0, 1, 2)):
                cc = c[sel].copy()
                cc[:, comps] = v
                D.append(d[sel])
                C.append(cc)
        for mr in (7, 3):
            out.append(EvalCases(s, np.concatenate(D), np.concatenate(C), mr, f"nonfinite/{name}/m{mr}"))
    return out


EVAL_FAMILIES = {"scan": family_scan, "creep": family_creep, "pattern": family_pattern, "tie": family_tie,
                 "skip": family_skip, "nonfinite": family_nonfinite}


def group_sizes(n):
    """The cooperative evaluator's legal group sizes for n shapes: powers of two from 2 that hold them."""
    return [g for g in (2, 4, 8, 16, 32, 64) if g >= n]


def eval_forms(scene):
    """(name, form, G, kQ) of every evaluator form legal for the scene (rv_eval's arguments):
    carry_path; carry_path_coop at every legal G; carry_path_spec<GT, kQ> for GT 4, 8, 16 and the
    runtime form (G = 32), kQ as the library's dispatch takes it (0: no quadric, 1: quadrics) and,
    where no quadric has cross terms, also the cross-term-free form (kQ = 2)."""
    n = n_shapes(scene)
    ty, _, u = pc.shape_table(scene.js)
    quad = ty == pc.QUADRIC
    kqs = [0] if not quad.any() else ([1] if (u[quad][:, 3:6] != 0).any() else [1, 2])
    out = [("lane", 0, 0, kqs[0])]
    for g in group_sizes(n):
        out.append((f"coop{g}", 1, g, kqs[0]))
        if g in (4, 8, 16, 32):
            out += [(f"spec{g}q{kq}", 2, g, kq) for kq in kqs]
    return out


# ------------------------------------------------------------------------------ chains --
class Chain:
    def __init__(self, scene, d, init, maxrec, label):
        self.scene, self.js, self.label, self.maxrec = scene, scene.js, label, int(maxrec)
        self.d = np.ascontiguousarray(d, F32).reshape(-1, 3)
        self.init = np.ascontiguousarray(init, F32).reshape(3)

    def __len__(self):
        return len(self.d)

    @functools.cached_property
    def ref(self):
        """The chained oracle: (carry-in of every entry [n, 3], hit flag [n], changer [n]: carry-out
        bits != carry-in bits, final carry [3]), entry by entry."""
        n = len(self.d)
        lib, js = oracle_lib(), ctypes.byref(self.js)
        cin, hit, chg = np.zeros((n, 3), F32), np.zeros(n, bool), np.zeros(n, bool)
        c, o = self.init.copy(), np.zeros(3, F32)
        rgb, cls, zero, cnt = np.zeros(3, F32), np.zeros(1, U8), np.zeros(1, I32), sc.ShadeCounts()
        pc_, po, pr, pk, pz = sc._p(c), sc._p(o), sc._p(rgb), sc._p(cls), sc._p(zero)
        for k in range(n):
            cin[k] = c
            r = lib.rco_prim_shoot(js, ctypes.c_int64(1), sc._p(self.d[k]), self.maxrec, PARITY, pc_, pr, pk,
                                   po, pz, ctypes.byref(cnt))
            assert r == 0 and cls[0] >= 2, (self.label, k, r, cls[0])
            hit[k] = cls[0] == 3
            chg[k] = (o.view(U32) != c.view(U32)).any()
            c[:] = o
        for a in (cin, hit, chg):
            a.setflags(write=False)
        return cin, hit, chg, c.copy()


def segments(name, W, H, maxrec):
    """The carry segments of one oracle frame: [(d [n, 3], initial carry)] in scan order — runs of
    DEP pixels between writers; the first entry's carry-in is the segment's initial carry."""
    s = scenes()[name]
    d, cin, cls = scan_pixels(name, W, H, maxrec)
    seg = np.cumsum(cls == 1)[cls >= 2]
    out = []
    if len(seg):
        cuts = np.flatnonzero(np.diff(seg)) + 1
        for a, b in zip(np.r_[0, cuts], np.r_[cuts, len(seg)]):
            out.append((d[a:b], cin[a]))
    return s, out


@functools.lru_cache(None)
def natural_chains():
    """Whole segments of quadric 256 x 256, depth 6, and the 96 x 72 segments of the random and the
    degenerate scenes (full-reflect-sphere and lone-mirror-plane are one segment each)."""
    out = []
    s, segs = segments("quadric", 256, 256, 7)
    out += [Chain(s, d, c, 7, f"natural/quadric256/{k}") for k, (d, c) in enumerate(segs)]
    for name in [n for n, _, _ in RANDOM] + list(DEGENERATE):
        s, segs = segments(name, 96, 72, 7)
        out += [Chain(s, d, c, 7, f"natural/{name}/{k}") for k, (d, c) in enumerate(segs)]
    return out


CUT_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 3 * 256 + 1)


@functools.lru_cache(None)
def cut_chains():
    """quadric 256 x 256's entries cut to the lengths around the windows' sizes, each length from
    several starts: at a changer (a changer in lane 0), 63 before one (lane 63), so that one ends
    the chain (the last valid lane of a short window) or follows a window boundary, inside the
    longest clean stretch (no changer), inside the longest run of changers (every entry a changer),
    and where exactly one clean entry sits between two changers."""
    s, segs = segments("quadric", 256, 256, 7)
    whole = [Chain(s, d, c, 7, "") for d, c in segs if len(d) >= 64]
    out = []
    for ci, ch in enumerate(whole):
        cin, _, chg, _ = ch.ref
        n = len(ch)
        idx = np.flatnonzero(chg)
        starts = set()
        if len(idx):
            runs = np.split(idx, np.flatnonzero(np.diff(idx) > 1) + 1)
            longest = max(runs, key=len)
            gaps = np.diff(idx)
            starts |= {int(idx[0]), max(0, int(idx[0]) - 63), int(longest[0])}
            one = np.flatnonzero(gaps == 2)
            if len(one):
                starts.add(int(idx[one[0]]))
            far = np.flatnonzero(gaps > 300)
            if len(far):
                starts.add(int(idx[far[0]]) + 1)
            for L in CUT_LENGTHS:              # a changer as the chain's last entry
                if idx[-1] - L + 1 >= 0:
                    starts.add(int(idx[-1]) - L + 1)
                    break
            mid = int(idx[len(idx) // 2])
            starts |= {max(0, mid - 64), max(0, mid - 255), max(0, mid - 256)}   # right after a boundary; lane 255
        for st in sorted(starts)[:10]:
            for L in CUT_LENGTHS:
                if st + L <= n:
                    out.append(Chain(s, ch.d[st:st + L], cin[st], 7, f"cut/quadric256/{ci}@{st}+{L}"))
        if len(out) > 400:
            break
    return out


def window_census(chains, width=64):
    """Over the chains' windows of `width` entries (the wave's 64, the workgroup's 256): the edges
    the cut chains are there for, as counts."""
    c = dict(windows=0, changer_lane0=0, changer_last_lane=0, changer_last_valid_short=0, changer_after_boundary=0,
             no_changer=0, all_changers=0, one_clean_between=0)
    for ch in chains:
        chg = ch.ref[2]
        for b in range(0, len(ch), width):
            w = chg[b:b + width]
            c["windows"] += 1
            c["changer_lane0"] += bool(w[0])
            c["changer_last_lane"] += len(w) == width and bool(w[-1])
            c["changer_last_valid_short"] += len(w) < width and bool(w[-1])
            c["changer_after_boundary"] += b > 0 and bool(w[0])
            c["no_changer"] += not w.any()
            c["all_changers"] += len(w) > 1 and bool(w.all())
            x = w.astype(np.int8)
            c["one_clean_between"] += bool(((x[:-2] == 1) & (x[1:-1] == 0) & (x[2:] == 1)).any()) if len(w) > 2 else 0
    return c


# ------------------------------------------------ the predictor, restated (hist_guess) --
def _i32(x):
    return (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31


def hist_guess(h, c, q, mult=1):
    """rc_resolve.hpp hist_guess on bit patterns: h = the history (latest first, 2..4 rows of three
    uint32), c the carry, q = 1.. the guess.  Returns three uint32."""
    m = len(h) - 1
    o = h[m]
    dl = []
    for k in range(3):
        d = _i32(int(h[0][k]) - int(o[k]))
        r = 1 if d >= 0 else -1
        if m > 1:
            t = d + r
            d = abs(t) // m * (1 if t >= 0 else -1)      # C's division truncates
        dl.append(d * mult)
    j = q - 1
    off = -((j + 1) >> 1) if (j & 1) else (j >> 1)
    a = [abs(x) for x in dl]
    mv = 0 if (a[0] >= a[1] and a[0] >= a[2]) else (1 if a[1] >= a[2] else 2)
    dl[mv] += off
    return np.array([(int(c[k]) + dl[k]) % 2 ** 32 for k in range(3)], U32)


def predictor_census(chain, nguess):
    """The predictive step on the chain's exact carries: (matches, misses, matches followed by a
    clean entry) over the steps that have a history of two carries and a changer at pos, with
    nguess guesses (the wave's 3, the workgroup's 15).  The history is pushed and dropped as
    wave_window does it along a chain (a clean entry drops it; a change after one starts it with
    the carry before and after)."""
    cin, _, chg, fin = chain.ref
    cb = np.concatenate([bits(cin), bits(fin).reshape(1, 3)])     # cb[k + 1] = carry after entry k
    n, pos, hist = len(chain), 0, []
    match = miss = match_then_clean = 0
    while pos < n:
        c, o0 = cb[pos], cb[pos + 1]
        if not chg[pos]:
            hist, pos = [], pos + 1
            continue
        if len(hist) < 2 or pos + 1 >= n:
            hist = ([o0] + (hist or [c]))[:4]
            pos += 1
            continue
        if any((hist_guess(hist, c, q) == o0).all() for q in range(1, nguess + 1)):
            match += 1
            hist = ([o0] + hist)[:4]
            if chg[pos + 1]:
                hist = ([cb[pos + 2]] + hist)[:4]
            else:
                match_then_clean += 1
                hist = []
            pos += 2
        else:
            miss += 1
            hist, pos = ([o0] + hist)[:4], pos + 1
    return match, miss, match_then_clean


@functools.lru_cache(None)
def dense_chains():
    """Dense runs for the predictor: the runs of at least 16 changers in a row of quadric 256 x 256
    (from 8 entries before the run to 8 after it), and the rows of the 4096 x 4096 image's dense
    region through the window's primary directions — a chain needs directions and an initial carry,
    not a rendered image."""
    out = []
    s, segs = segments("quadric", 256, 256, 7)
    for si, (d, c0) in enumerate(segs):
        if len(d) < 24:
            continue
        ch = Chain(s, d, c0, 7, "")
        cin, _, chg, _ = ch.ref
        idx = np.flatnonzero(chg)
        if not len(idx):
            continue
        for run in np.split(idx, np.flatnonzero(np.diff(idx) > 1) + 1):
            if len(run) >= 16:
                a, b = max(0, int(run[0]) - 8), min(len(d), int(run[-1]) + 9)
                out.append(Chain(s, d[a:b], cin[a], 7, f"dense/quadric256/{si}@{a}+{b - a}"))
    out += virtual_dense_chains()
    return out


VIRTUAL = dict(size=4096, rows=(2040, 2048, 2056, 2064), x0=0, x1=4096)


def virtual_dense_chains(max_len=700, want=6):
    """Rows of the quadric example's 4096 x 4096 image (never rendered): the row's DEP pixels by the
    oracle's class, the chain from zeros over each row's first segment, kept where more than half
    of its entries change the carry."""
    s = scenes()["quadric"]
    W = VIRTUAL["size"]
    out = []
    for y in range(1024, 3072, 64):
        if len(out) >= want:
            break
        d = row_dirs(s.js, W, W, y)
        _, _, cls = shoot(s.js, d, np.zeros_like(d), 7)
        dep = cls >= 2
        if dep.sum() < 64:
            continue
        seg = np.cumsum(cls == 1)[dep]
        dd = d[dep]
        first = np.flatnonzero(seg == np.bincount(seg).argmax())
        dd = dd[first[0]:first[-1] + 1][:max_len]
        probe = Chain(s, dd[:96], np.zeros(3, F32), 7, "")
        if probe.ref[2].mean() > 0.5:
            out.append(Chain(s, dd, np.zeros(3, F32), 7, f"dense/quadric4096/row{y}+{len(dd)}"))
    return out


def row_dirs(js, W, H, y):
    """pc.primary_dirs' row y of the W x H image."""
    cw, chh = F32(js.camera_width), F32(js.camera_height)
    pw, ph = cw / F32(W), chh / F32(H)
    x = np.arange(W, dtype=F64)
    dx = ((0.0 - F64(cw) / 2.0) + F64(pw) * (x + 0.5)).astype(F32)
    dy = np.full(W, ((0.0 + F64(chh) / 2.0) - F64(ph) * (F64(y) + 0.5)), F64).astype(F32)
    dz = np.full(W, -1.0, F32)
    ss = dx.astype(F64) * dx.astype(F64)
    ss = ss + dy.astype(F64) * dy.astype(F64)
    ss = ss + dz.astype(F64) * dz.astype(F64)
    ln = np.sqrt(ss).astype(F32)
    return np.stack([dx / ln, dy / ln, dz / ln], 1).astype(F32)


ZERO_VALUES = (0.0, -0.0, np.nan)


@functools.lru_cache(None)
def zero_chains():
    """Chains whose initial carry has +0, -0 or NaN components and whose entries all leave it as it
    is: the longest clean stretch of a frame's longest segments, its own carry with one, two or
    three components replaced, cut where the first entry would move it.  Every carry-in must keep
    the initial bits, signs and NaN included (a NaN is unequal to itself, and -0 equals +0: only a
    comparison of the bits calls these entries clean)."""
    out = []
    for name, W, H in (("quadric", 256, 256), ("full-reflect-sphere", 96, 72), ("lone-mirror-plane", 96, 72),
                       ("random14x", 96, 72)):
        s, segs = segments(name, W, H, 7)
        for si, (d, c0) in enumerate(sorted(segs, key=lambda t: -len(t[0]))[:3]):
            cin, _, chg, _ = Chain(s, d, c0, 7, "").ref
            edges = np.r_[-1, np.flatnonzero(chg), len(d)]
            k = int(np.argmax(np.diff(edges)))
            a, e = int(edges[k]) + 1, int(edges[k + 1])
            if e - a < 65:
                continue
            for comps in ((0,), (1,), (2,), (0, 2), (0, 1, 2)):
                for z in ZERO_VALUES:
                    cc = cin[a].copy()
                    cc[list(comps)] = z
                    tiled = np.tile(cc, (e - a, 1))
                    moved = np.flatnonzero(~same_rows(shoot(s.js, d[a:e], tiled, 7)[0], tiled))
                    n = min(int(moved[0]) if len(moved) else e - a, 200)
                    if n >= 65:
                        tag = "nan" if np.isnan(z) else ("-0" if np.signbit(z) else "+0")
                        out.append(Chain(s, d[a:a + n], cc, 7, f"zeros/{name}/{si}/{tag}{comps}+{n}"))
    return out


CHAIN_FAMILIES = {"natural": natural_chains, "cut": cut_chains, "dense": dense_chains, "zeros": zero_chains}


# -------------------------------------------------------------------------- the frames --
FRAMES = [("quadric", 256, 256), ("quadric", 333, 517), ("reflection", 256, 256), ("full-reflect-sphere", 96, 72),
          ("mirror-box", 96, 72), ("random33", 96, 72), ("random65", 96, 72),
          # one segment of 1 248 / 1 562 entries with runs of 23 / 46 changers: with a short hand_run a
          # helper takes them at 64 lanes an entry
          ("random33x", 96, 72), ("random64x", 96, 72)]
FRAME_DEPTHS = (4, 6)
# the first frames here to cross an LDS chunk of the compaction (4 096 pixels of a row: 770 DEP pixels
# beyond it) and a scan chunk (2 048 rows: 160 segment starts beyond it); depth 6, default tuning only
CHUNK_FRAMES = [("reflection", 8195, 3), ("reflection", 3, 4099)]
# the schedules of tests/test_gpu.py's test_parity_schedules that change the resolver ...
SCHEDULES = {"default": {}, "side-0": dict(side=0), "side-1": dict(side=1), "side-3": dict(side=3),
             "side-4": dict(side=4), "no-dep-fast": dict(dep_fast=0), "no-coop": dict(coop=0),
             "helpers-0": dict(helpers=0), "helpers-1": dict(helpers=1), "hand-run-1": dict(hand_run=1),
             "block-min-0": dict(block_min=0), "block-min-256": dict(block_min=256),
             "small-grid": dict(resolve_grid=64, team_blocks=16), "resolve-shared": dict(resolve_shared=1),
             "no-headb-first": dict(headb_first=0), "no-x0": dict(x0=0),
             # ... and the ones nothing ran before: the wave's and the leader's clean-step counts
             "wave-k-1": dict(wave_k=1), "wave-k-8": dict(wave_k=8), "resolve-k-8": dict(resolve_k=8)}
# the team on short segments: long_len 64 sends 54 segments of quadric 256 x 256 through it, 256 one
TEAM_SCHEDULES = {f"long-{ll}-team-{tb}-cscan-{cs}-clean-{rcl}": dict(long_len=ll, team_cscan=cs, resolve_clean=rcl,
                                                                      **({"team_blocks": tb} if tb else {}))
                  for ll in (64, 256) for tb in (16, 0) for cs in (0, 1) for rcl in (1, 4)}
# the helper hand-off after 8 and 32 changes in a row, quadric 512 x 512
HAND_SCHEDULES = {f"hand-run-{hr}-helpers-{hp}": dict(hand_run=hr, helpers=hp) for hr in (8, 32) for hp in (1, 8)}
HAND_FRAME = ("quadric", 512, 512)


@functools.lru_cache(None)
def frame_reference(name, W, H, depth):
    """(image, DEP pixel indices in scan order, their carry-ins, their hit bits) of rco_render_cls."""
    img, cls, cin = render_cls(scenes()[name], W, H, depth + 1)
    dep = np.flatnonzero(cls >= 2)
    out = (img, dep.astype(np.int64), cin[dep], (cls[dep] == 3).astype(U8))
    for a in out:
        a.setflags(write=False)
    return out
