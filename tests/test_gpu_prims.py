"""Ray-level differential tests: the product's own device routines (rc_device.hpp, rc_cudasem.hpp,
run one thread per case by tests/tools/prim_check.hip) against the CPU oracle's shape tests and
against numpy, libm and rational arithmetic, on the case lists of tests/prim_cases.py
(DESIGN.md §19).

Contract.  A case is ACCEPTED iff hit && t > 0 && t < inf (the scan's rule with best = inf).  The
device and the reference agree on ACCEPTED for every case, and where they accept, on every bit of
t.  A rejected t is not compared (the proofs promise only its class).  A shadow form's boolean is
compared with ACCEPTED.  Hit points, normals and zero-normalize counts are compared bit for bit,
with one NaN equal to another: the sign and payload of a NaN that arithmetic produces are the
hardware's (x86 gives the negative quiet NaN, gfx950 the positive one) and no caller can see them.
No case is left out of a comparison.  The harness is built by `make primcheck`; if it cannot be
built these tests fail."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import prim_cases as pc
from helpers import ROOT

pytestmark = pytest.mark.gpu

F32, F64, I32 = np.float32, np.float64, np.int32
INF = np.inf

# tests/tools/prim_check.hip's enums
OP = {n: k for k, n in enumerate(["div", "div_mut", "sqrt", "sqrt_mut", "length", "div3", "pow20",
                                  "pown", "quot_class", "quot_class_mut", "x0_reject", "quant",
                                  "primary_dir", "pow_general"])}
FORM = {n: k for k, n in enumerate(["test", "test_x0", "o0", "o0_x0", "shadow", "shadow_x0",
                                    "uni_noquad", "uni_quad", "uni_quad_x0", "cuda"])}
LIST = {n: k for k, n in enumerate(["nearest", "primary", "shadowed", "cu_nearest", "cu_shadowed"])}
FRAME = {n: k for k, n in enumerate(["hit_frame", "sel_noquad", "sel_quad"])}


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _ok(r, what):
    """0, or the entry's refusal (-2) as a failure; a HIP error ends the session: nothing more is
    started on a device that has reported one."""
    if r > 0:
        pytest.exit(f"{what}: HIP error {r}", returncode=3)
    assert r == 0, f"{what} returned {r}"


class Harness:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.pc_scene_create.restype = ctypes.c_void_p
        self.lib.pc_scene_create.argtypes = [ctypes.c_void_p]
        self.lib.pc_scene_destroy.argtypes = [ctypes.c_void_p]
        self.lib.pc_scene_info.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int)] * 3
        self.lib.pc_scalar.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4
        self.lib.pc_shape.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
        self.lib.pc_list.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 5
        self.lib.pc_frame.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 7
        self._scenes = {}

    def scene(self, js):
        key = ctypes.addressof(js)
        if key not in self._scenes:
            h = self.lib.pc_scene_create(ctypes.addressof(js))
            assert h, "pc_scene_create failed"
            self._scenes[key] = h
        return self._scenes[key]

    def info(self, js):
        n, hq, o0 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self.lib.pc_scene_info(self.scene(js), n, hq, o0)
        return n.value, hq.value, o0.value

    def scalar(self, op, a, b=None, o0=None, o1=None):
        a = np.ascontiguousarray(a)
        b = None if b is None else np.ascontiguousarray(b)
        n = len(a)
        r = self.lib.pc_scalar(OP[op], n, _p(a), _p(b), _p(o0), _p(o1))
        _ok(r, f"pc_scalar({op})")

    def shape(self, form, c):
        hit, t = np.zeros(len(c), I32), np.zeros(len(c), F32)
        r = self.lib.pc_shape(self.scene(c.js), FORM[form], len(c), _p(c.O), _p(c.D), _p(c.shape),
                              _p(c.skip), _p(hit), _p(t))
        _ok(r, f"pc_shape({form})")
        return hit, t

    def list(self, form, js, O, D, skip, has_quadric=-1, o0_ok=-1):
        idx, t = np.zeros(len(skip), I32), np.zeros(len(skip), F32)
        r = self.lib.pc_list(self.scene(js), LIST[form], has_quadric, o0_ok, len(skip), _p(O), _p(D),
                             _p(skip), _p(idx), _p(t))
        _ok(r, f"pc_list({form})")
        return idx, t

    def frame(self, form, js, shape, O, D, t):
        n = len(shape)
        P, N, z = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros(n, I32)
        r = self.lib.pc_frame(self.scene(js), FRAME[form], n, _p(shape), _p(O), _p(D), _p(t), _p(P),
                              _p(N), _p(z))
        _ok(r, f"pc_frame({form})")
        return P, N, z

    def close(self):
        for h in self._scenes.values():
            self.lib.pc_scene_destroy(h)
        self._scenes = {}


@pytest.fixture(scope="module")
def hw():
    """The harness library; built here (no build, no pass)."""
    subprocess.run(["make", "-s", "primcheck"], cwd=ROOT, check=True, capture_output=True)
    h = Harness(os.path.join(ROOT, "tests", "build", "libprimcheck.so"))
    yield h
    h.close()


# ------------------------------------------------------------------------ reporting --
def _hex32(a):
    return " ".join(f"{v:08x}" for v in pc.bits32(np.atleast_1d(a)))


def _hex64(a):
    return " ".join(f"{v:016x}" for v in pc.bits64(np.atleast_1d(a)))


def _fail_case(what, c, i, dev, ref):
    pytest.fail(f"{what}: case {i} of {len(c)}: shape {c.shape[i]} skip {c.skip[i]} "
                f"O {_hex32(c.O[i])} D {_hex32(c.D[i])} | device {dev} | reference {ref}")


def check_contract(what, c, dev_hit, dev_t, ref_hit, ref_t, shadow=False):
    """The comparison contract on every case of c; the first mismatch in hex."""
    acc_ref = pc.accepted(ref_hit, ref_t)
    acc_dev = (dev_hit != 0) if shadow else pc.accepted(dev_hit, dev_t)
    bad = acc_dev != acc_ref
    if not shadow:
        bad |= acc_ref & (pc.bits32(dev_t) != pc.bits32(ref_t))
    print(f"[gpu_prims] {what}: {len(c)} cases, {int(acc_ref.sum())} accepted, {int(bad.sum())} mismatches")
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        _fail_case(what, c, i, f"hit {dev_hit[i]} t {_hex32(dev_t[i])}",
                   f"hit {ref_hit[i]} t {_hex32(ref_t[i])} accepted {bool(acc_ref[i])}")


def same_bits32(a, b):
    """Bit equality of float32 arrays, one NaN equal to another."""
    return (pc.bits32(a) == pc.bits32(b)) | (np.isnan(a) & np.isnan(b))


def same_bits64(a, b):
    return (pc.bits64(a) == pc.bits64(b)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------- shape-test families --
_REF = {}


def reference(name, cuda=False):
    """The oracle's (hit, t) of a family, computed once and shared."""
    key = (name, cuda)
    if key not in _REF:
        c = pc.RAY_FAMILIES[name]()
        hit, t, _ = pc.ref_shape(c.js, c.O, c.D, c.shape, c.skip, cuda=cuda)
        hit.setflags(write=False), t.setflags(write=False)
        _REF[key] = (hit, t)
    return _REF[key]


def run_forms(hw, name):
    """Every form that applies to a case, on every case of the family."""
    c = pc.RAY_FAMILIES[name]()
    ty, _, _ = pc.shape_table(c.js)
    ref_hit, ref_t = reference(name)
    cu_hit, cu_t = reference(name, cuda=True)
    no_cross = c.shape < pc.NO_CROSS                  # the quad_x0 forms: zero cross coefficients
    no_quad = ty[c.shape] != pc.QUADRIC               # test_unified<false>: scenes without quadrics
    at_zero = ~c.O.any(1) & ~np.signbit(c.O).any(1)   # the o0 forms: O = (+0, +0, +0)
    plan = [("test", None, False), ("shadow", None, True), ("uni_quad", None, False),
            ("test_x0", no_cross, False), ("shadow_x0", no_cross, True),
            ("uni_quad_x0", no_cross, False), ("uni_noquad", no_quad, False)]
    if at_zero.all():
        plan += [("o0", None, False), ("o0_x0", no_cross, False)]
    for form, mask, shadow in plan:
        sub = c if mask is None else c.take(mask)
        rh, rt = (ref_hit, ref_t) if mask is None else (ref_hit[mask], ref_t[mask])
        hit, t = hw.shape(form, sub)
        check_contract(f"{name}/{form}", sub, hit, t, rh, rt, shadow)
    hit, t = hw.shape("cuda", c)
    check_contract(f"{name}/cuda", c, hit, t, cu_hit, cu_t)


@pytest.mark.parametrize("name", ["tangent", "surface", "branches", "plane", "nonfinite", "random",
                                  "primary"])
def test_shape_forms(hw, name):
    """test_shape, the hit_*_o0 forms (O = 0), the shadow forms, test_unified<false>, <true, false>,
    <true, true> and cu_test against o_* / c_* of the oracle."""
    run_forms(hw, name)


def test_x0_reject(hw):
    O, D = pc.family_x0()
    got = np.zeros(len(O), I32)
    hw.scalar("x0_reject", O, D, o1=got)
    want = pc.x0_reject_ref(O, D)
    bad = (got != 0) != want
    print(f"[gpu_prims] x0_reject: {len(O)} cases, {int(want.sum())} rejected, {int(bad.sum())} mismatches")
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        pytest.fail(f"x0_reject case {i}: O {_hex32(O[i])} D {_hex32(D[i])} device {got[i]} "
                    f"reference {int(want[i])}")


# --------------------------------------------------------------- whole lists, frames --
SCENES = pc.GOLDEN_SCENES + ["random14x", "random65"]


@pytest.mark.parametrize("name", SCENES)
def test_lists(hw, name):
    """nearest, nearest_primary, shadowed, cu_nearest and cu_shadowed over the whole shape list,
    under the library's has_quadric / o0_ok for the scene and with the cross-term-free and the o0
    forms switched off."""
    sc = pc.list_scenes()[name]
    O, D, skip = pc.scene_rays(name)
    n, hq, o0 = hw.info(sc.js)
    assert n == sc.num_shapes
    idx, t, _, _, _ = pc.ref_nearest(sc.js, O, D, skip)
    rays = pc.Cases(sc.js, O, D, np.maximum(idx, 0), skip)

    def check(what, rays, di, dt, ri, rt, boolean=False):
        if boolean:
            bad = (di != 0) != (ri >= 0)
        else:
            bad = (di != ri) | ((ri >= 0) & (pc.bits32(dt) != pc.bits32(rt)))
        print(f"[gpu_prims] {name}/{what}: {len(ri)} rays, {int((ri >= 0).sum())} hit, "
              f"{int(bad.sum())} mismatches")
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            _fail_case(f"{name}/{what}", rays, i, f"idx {di[i]} t {_hex32(dt[i])}",
                       f"idx {ri[i]} t {_hex32(rt[i])}")

    forms = sorted({hq, min(hq, 1)})      # the library's value, and the cross-term form forced
    for q in forms:
        check(f"nearest[hq={q}]", rays, *hw.list("nearest", sc.js, O, D, skip, has_quadric=q), idx, t)
        check(f"shadowed[hq={q}]", rays, *hw.list("shadowed", sc.js, O, D, skip, has_quadric=q),
              idx, t, boolean=True)
    prim = ~O.any(1) & ~np.signbit(O).any(1) & (skip == -1)
    assert prim.sum() >= 64 * 48
    for q in forms:
        for o in sorted({o0, 0}):         # ... and nearest_primary's fallback forced
            di, dt = hw.list("primary", sc.js, O[prim], D[prim], skip[prim], has_quadric=q, o0_ok=o)
            check(f"nearest_primary[hq={q},o0={o}]", rays.take(prim), di, dt, idx[prim], t[prim])
    ci, ct = pc.ref_nearest(sc.js, O, D, skip, cuda=True)
    check("cu_nearest", rays, *hw.list("cu_nearest", sc.js, O, D, skip), ci, ct)
    check("cu_shadowed", rays, *hw.list("cu_shadowed", sc.js, O, D, skip), ci, ct, boolean=True)


def frame_cases(name):
    """(shape, O, D, t): the oracle's accepted hits of the scene's rays, the same rays at t = 1e38,
    3e38 and 1e-40 (hit points that overflow or do not move), and t = 0 from every sphere's centre
    (a zero-length normal: one zero-normalize event)."""
    sc = pc.list_scenes()[name]
    O, D, skip = pc.scene_rays(name)
    idx, t, _, _, _ = pc.ref_nearest(sc.js, O, D, skip)
    hit = idx >= 0
    sh, O, D, t = [idx[hit]], [O[hit]], [D[hit]], [t[hit]]
    step = max(1, len(sh[0]) // 500)
    for tv in (1e38, 3e38, 1e-40, -2.5):
        sh.append(sh[0][::step]), O.append(O[0][::step]), D.append(D[0][::step])
        t.append(np.full(len(sh[-1]), tv, F32))
    ty, pos, _ = pc.shape_table(sc.js)
    for k in np.flatnonzero(ty == pc.SPHERE):
        for d in ([0, 0, -1], [1, 0, 0], [0.6, 0.8, 0]):
            sh.append(np.array([k], I32)), O.append(pos[k][None].astype(F32))
            D.append(np.array([d], F32)), t.append(np.zeros(1, F32))
    return (sc, np.concatenate(sh).astype(I32), np.concatenate(O).astype(F32),
            np.concatenate(D).astype(F32), np.concatenate(t).astype(F32))


@pytest.mark.parametrize("name", SCENES)
def test_frames(hw, name):
    """hit_frame and hit_frame_sel<kQuad>: P, N (and hit_frame's zero-normalize count) bit for bit."""
    sc, sh, O, D, t = frame_cases(name)
    P, N, z = pc.ref_frame(sc.js, sh, O, D, t)
    ty, _, _ = pc.shape_table(sc.js)
    c = pc.Cases(sc.js, O, D, sh, np.full(len(sh), -1, I32))
    has_sphere = bool((ty == pc.SPHERE).any())
    assert z.sum() >= 1 or not has_sphere

    def check(what, sel, dP, dN, dz=None):
        bad = ~(same_bits32(dP, P[sel]).all(1) & same_bits32(dN, N[sel]).all(1))
        if dz is not None:
            bad |= dz != z[sel]
        print(f"[gpu_prims] {name}/{what}: {int(sel.sum())} frames, {int(z[sel].sum())} zero events, "
              f"{int(bad.sum())} mismatches")
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            j = int(np.flatnonzero(sel)[i])
            _fail_case(f"{name}/{what} (t {_hex32(t[j])})", c, j,
                       f"P {_hex32(dP[i])} N {_hex32(dN[i])} zero {None if dz is None else dz[i]}",
                       f"P {_hex32(P[j])} N {_hex32(N[j])} zero {z[j]}")

    every = np.ones(len(sh), bool)
    check("hit_frame", every, *hw.frame("hit_frame", sc.js, sh, O, D, t))
    dP, dN, _ = hw.frame("sel_quad", sc.js, sh, O, D, t)
    check("hit_frame_sel<true>", every, dP, dN)
    nq = ty[sh] != pc.QUADRIC
    if nq.any():
        dP, dN, _ = hw.frame("sel_noquad", sc.js, sh[nq], O[nq], D[nq], t[nq])
        check("hit_frame_sel<false>", nq, dP, dN)


# ------------------------------------------------------------------ scalar primitives --
def _first(bad):
    return int(np.flatnonzero(bad)[0])


def division_mismatches(hw, op):
    num, den, regular = pc.family_division()
    q, t = np.zeros(len(num), F64), np.zeros(len(num), F32)
    hw.scalar(op, num, den, o0=q, o1=t)
    with np.errstate(all="ignore"):
        want = num / den
        want_t = want.astype(F32)
    bad = regular & ((pc.bits64(q) != pc.bits64(want)) | (pc.bits32(t) != pc.bits32(want_t)))
    one = np.ones(len(num), I32)
    bad |= pc.accepted(one, t) != pc.accepted(one, want_t)
    return num, den, q, t, want, want_t, bad


def test_division(hw):
    """div_nr(n, d, recip_nr(d)) is IEEE n / d in every bit for finite non-zero float-derived
    operands (|n| in [2^-201, 2^130], |d| in [2^-149, 2^129]; subnormal floats widened among them),
    tquot its float; with a zero, inf or NaN operand tquot agrees with (float)(n / d) on ACCEPTED."""
    num, den, q, t, want, want_t, bad = division_mismatches(hw, "div")
    print(f"[gpu_prims] division: {len(num)} cases, {int(bad.sum())} mismatches")
    if bad.any():
        i = _first(bad)
        pytest.fail(f"div_nr case {i}: num {_hex64(num[i])} den {_hex64(den[i])} | device q "
                    f"{_hex64(q[i])} t {_hex32(t[i])} | reference q {_hex64(want[i])} t {_hex32(want_t[i])}")


def sqrt_mismatches(hw, op):
    s = pc.family_sqrt()
    got = np.zeros(len(s), F64)
    hw.scalar(op, s, o0=got)
    return s, got, np.sqrt(s), ~same_bits64(got, np.sqrt(s))


def test_sqrt(hw):
    """sqrt_ns is the correctly rounded square root for +-0, [2^-767, max], inf and NaN."""
    s, got, want, bad = sqrt_mismatches(hw, "sqrt")
    print(f"[gpu_prims] sqrt: {len(s)} cases, {int(bad.sum())} mismatches")
    if bad.any():
        i = _first(bad)
        pytest.fail(f"sqrt_ns case {i}: s {_hex64(s[i])} | device {_hex64(got[i])} | reference "
                    f"{_hex64(want[i])}")


def test_length_div3(hw):
    """length = (float)sqrt(double sum of squares); div3 = the IEEE float32 quotients."""
    a, ln, a3, l3 = pc.family_vec()
    got = np.zeros(len(a), F32)
    hw.scalar("length", a, o1=got)
    bad = ~same_bits32(got, ln)
    print(f"[gpu_prims] length: {len(a)} cases, {int(bad.sum())} mismatches")
    if bad.any():
        i = _first(bad)
        pytest.fail(f"length case {i}: a {_hex32(a[i])} | device {_hex32(got[i])} | reference {_hex32(ln[i])}")
    got3 = np.zeros((len(a3), 3), F32)
    hw.scalar("div3", a3, l3, o1=got3)
    with np.errstate(all="ignore"):
        want3 = a3 / l3[:, None]                                     # float32 / float32
    assert want3.dtype == F32
    bad = ~same_bits32(got3, want3).all(1)
    print(f"[gpu_prims] div3: {len(a3)} cases, {int(bad.sum())} mismatches")
    if bad.any():
        i = _first(bad)
        pytest.fail(f"div3 case {i}: a {_hex32(a3[i])} len {_hex32(l3[i])} | device {_hex32(got3[i])} "
                    f"| reference {_hex32(want3[i])}")


def quot_class_mismatches(hw, op):
    num, den = pc.family_quot_class()
    got = np.zeros(len(num), I32)
    hw.scalar(op, num, den, o1=got)
    want = pc.quot_class_ref(num, den)
    return num, den, got, want, got != want


def test_quot_class(hw):
    """quot_class is the class of (float)(num / den): exponent path and division path alike."""
    num, den, got, want, bad = quot_class_mismatches(hw, "quot_class")
    print(f"[gpu_prims] quot_class: {len(num)} cases, {int(bad.sum())} mismatches")
    if bad.any():
        i = _first(bad)
        pytest.fail(f"quot_class case {i}: num {_hex64(num[i])} den {_hex64(den[i])} | device {got[i]} "
                    f"| reference {want[i]}")


def test_mutants_are_caught(hw):
    """The lists have teeth: one Newton step less in the reciprocal, sqrt_ns without its second
    correction and quot_class with the bound 127 each differ from the reference somewhere."""
    caught = {"div_nr with one Newton step": int(division_mismatches(hw, "div_mut")[-1].sum()),
              "sqrt_ns with one correction": int(sqrt_mismatches(hw, "sqrt_mut")[-1].sum()),
              "quot_class with the bound 127": int(quot_class_mismatches(hw, "quot_class_mut")[-1].sum())}
    for k, v in caught.items():
        print(f"[gpu_prims] mutant {k}: {v} cases caught")
    assert all(caught.values()), f"a mutant passes the case lists: {caught}"


# ----------------------------------------------------------------------------- powers --
def test_pow20(hw):
    """pow20 against libm's pow(x, 20) — the reference's call — narrowed the way shade narrows it,
    (float)((double)sl * p) for 16 fixed sl; and within one ulp of the exactly rounded x^20."""
    x = pc.family_pow20()
    dev = np.zeros(len(x), F64)
    hw.scalar("pow20", x, o0=dev)
    lm = pc.libm_pow(x, 20.0)
    ex = pc.exact_pow(x, 20)
    sl = pc.POW20_SL.astype(F64)[None, :]
    got, want = (sl * dev[:, None]).astype(F32), (sl * lm[:, None]).astype(F32)
    bad = (pc.bits32(got) != pc.bits32(want)).any(1)
    d_ex, l_ex = pc.ulp_distance(dev, ex), pc.ulp_distance(lm, ex)
    print(f"[gpu_prims] pow20: {len(x)} inputs; device != exact rounding: {int((d_ex != 0).sum())}, "
          f"libm != exact rounding: {int((l_ex != 0).sum())}, device != libm: "
          f"{int((pc.bits64(dev) != pc.bits64(lm)).sum())}, narrowed mismatches: {int(bad.sum())}")
    if bad.any():
        i = _first(bad)
        pytest.fail(f"pow20 case {i}: x {_hex64(x[i])} | device {_hex64(dev[i])} -> {_hex32(got[i])} | "
                    f"libm {_hex64(lm[i])} -> {_hex32(want[i])}")
    assert d_ex.max() <= 1, f"pow20 is {int(d_ex.max())} ulps from the exact power at x {_hex64(x[d_ex.argmax()])}"


def test_pown(hw):
    """pown_dd(a, n), n in -8..-1, 3..12, 20, 31 and the spot-exponent probe's cases: (float)p equals
    (float)pow(a, n) of libm; the double is within one ulp of the exactly rounded power.  The edge
    bases (+-0, +-inf, NaN, 1e-30 .. 3e38) against every exponent -64 .. 64: (float)p equals
    (float)pow(a, n) in every bit, the sign of a zero included (a NaN for a NaN); their doubles are
    compared with the exact power where it is a normal double (pc.pown_regular)."""
    a, n = pc.family_pown()
    dev = np.zeros(len(a), F64)
    hw.scalar("pown", a, n, o0=dev)
    lm = pc.libm_pow(a, n.astype(F64))
    reg = pc.pown_regular(a, n)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        got, want = dev.astype(F32), lm.astype(F32)
    bad = ~same_bits32(got, want)
    ex = pc.exact_pow(a[reg], n[reg])
    d_ex, l_ex = np.zeros(len(a), np.int64), np.zeros(len(a), np.int64)
    d_ex[reg], l_ex[reg] = pc.ulp_distance(dev[reg], ex), pc.ulp_distance(lm[reg], ex)
    print(f"[gpu_prims] pown: {len(a)} cases, {int(reg.sum())} regular; device != exact rounding: "
          f"{int((d_ex != 0).sum())}, libm != exact rounding: {int((l_ex != 0).sum())}, device != libm: "
          f"{int((~same_bits64(dev, lm))[reg].sum())}, narrowed mismatches: {int(bad.sum())} "
          f"({int(bad[~reg].sum())} of {int((~reg).sum())} edge cases)")
    for e in sorted(set(n.tolist())):
        m = (n == e) & reg
        print(f"[gpu_prims]   n = {e}: {int(m.sum())} regular cases, device != exact "
              f"{int((d_ex[m] != 0).sum())}, libm != exact {int((l_ex[m] != 0).sum())}")
    if bad.any():
        i = _first(bad)
        pytest.fail(f"pown_dd case {i}: a {_hex64(a[i])} n {n[i]} | device {_hex64(dev[i])} -> "
                    f"{_hex32(got[i])} | libm {_hex64(lm[i])} -> {_hex32(want[i])}")
    assert d_ex.max() <= 1, (f"pown_dd is {int(d_ex.max())} ulps from the exact power at a "
                             f"{_hex64(a[d_ex.argmax()])} n {n[d_ex.argmax()]}")
