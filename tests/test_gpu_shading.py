"""Hit-level differential tests: the product's own device routines after the hit — shade, cu_shade,
the bounce loops shoot<MODE> and shade_dep_cont, quant and primary_dir (rc_device.hpp,
rc_cudasem.hpp, run one thread per case by tests/tools/prim_check.hip) — against the CPU oracle's
o_shade / o_shoot / o_quant and numpy, on the case lists of tests/shade_cases.py.

Contract.  Device and oracle agree on every bit of every output float, one NaN equal to another as
in tests/test_gpu_prims.py (the NaN's sign is the hardware's); on the class; on the carry after the
pixel where the class says the pixel wrote it; and on the zero-normalize events, case by case.  No
case is left out of a comparison.  The one exception is `cone_general`: a spot exponent that is no
small integer goes through the device library's pow where the reference calls glibc's; a double
pow accurate to a few double ulps on either side can make the narrowed floats differ only at a
rounding midpoint, so the narrowed value is required within one float ulp and the number of
cases that differ at all is printed.  The harness is built by `make primcheck`; if it cannot be
built these tests fail."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import prim_cases as pc
import shade_cases as sc
from helpers import ROOT
from test_gpu_prims import Harness, _ok, _p, same_bits32

pytestmark = pytest.mark.gpu

F32, F64, I32 = np.float32, np.float64, np.int32

# tests/tools/prim_check.hip's enums (the scalar operations' are test_gpu_prims.OP)
SHADE = {n: k for k, n in enumerate(["shade", "staged", "cuda", "mut_inert", "mut_alpha", "mut_zero"])}
SHOOT = {n: k for k, n in enumerate(["fast", "parity_a", "parity_c", "classify", "dep_cont"])}
CLS_IDENT, CLS_WRITER, CLS_DEP = 0, 1, 2


class ShadeHarness(Harness):
    def __init__(self, path):
        super().__init__(path)
        self.lib.pc_shade.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
        self.lib.pc_shoot.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 7
        self.lib.pc_render_pixel.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2
        self.lib.pc_scene_lit_info.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int)] * 3

    def lit_info(self, js):
        m, dep_fast, staged = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self.lib.pc_scene_lit_info(self.scene(js), m, dep_fast, staged)
        return m.value, dep_fast.value, staged.value

    def shade(self, form, c):
        rgb, zero = np.zeros((len(c), 3), F32), np.zeros(len(c), I32)
        r = self.lib.pc_shade(self.scene(c.js), SHADE[form], len(c), _p(c.idx), _p(c.P), _p(c.N),
                              _p(c.D), _p(rgb), _p(zero))
        _ok(r, f"pc_shade({form})")
        return rgb, zero

    def shoot(self, form, c, carry=None, dep_fast=-1):
        n = len(c)
        carry = np.ascontiguousarray(c.carry if carry is None else carry, F32)
        rgb, cls, cout = np.zeros((n, 3), F32), np.zeros(n, I32), np.zeros((n, 3), F32)
        zero, flag = np.zeros(n, I32), np.zeros(n, I32)
        r = self.lib.pc_shoot(self.scene(c.js), SHOOT[form], dep_fast, n, c.maxrec, _p(c.d), _p(carry),
                              _p(rgb), _p(cls), _p(cout), _p(zero), _p(flag))
        _ok(r, f"pc_shoot({form})")
        return rgb, cls, cout, zero, flag

    def render_pixel(self, js, W, H, max_iter, xy):
        xy = np.ascontiguousarray(xy, I32)
        rgb = np.zeros((len(xy), 3), F32)
        r = self.lib.pc_render_pixel(self.scene(js), W, H, max_iter, len(xy), _p(xy), _p(rgb))
        _ok(r, "pc_render_pixel")
        return rgb


@pytest.fixture(scope="module")
def hw():
    """The harness library; built here (no build, no pass)."""
    subprocess.run(["make", "-s", "primcheck"], cwd=ROOT, check=True, capture_output=True)
    h = ShadeHarness(os.path.join(ROOT, "tests", "build", "libprimcheck.so"))
    yield h
    h.close()


def _hex32(a):
    return " ".join(f"{v:08x}" for v in pc.bits32(np.atleast_1d(a)))


def _fail_shade(what, c, i, dev, ref):
    pytest.fail(f"{what} [{c.label}]: case {i} of {len(c)}: shape {c.idx[i]} P {_hex32(c.P[i])} "
                f"N {_hex32(c.N[i])} D {_hex32(c.D[i])} | device {dev} | reference {ref}")


# ---------------------------------------------------------------------------- shade --
def stage_fits(js):
    """rc_pixel.hpp's stage_fits, restated: do the pixel kernels stage this scene in LDS?"""
    n, m = js.num_shapes, js.num_lights
    return n + 1 <= 32 and (n + 1) * m <= 128


def ulps32(a, b):
    """Places between finite float32 values along the float line (huge where either is not finite)."""
    def ordered(x):
        i = pc.bits32(x).astype(np.int64)
        return np.where(i & 0x80000000, -(i & 0x7fffffff), i)
    d = np.abs(ordered(a) - ordered(b))
    return np.where(np.isfinite(a) & np.isfinite(b), d, np.int64(1) << 40)


def pow_agreement(hw, c):
    """For a cone_general list: per case, does the device library's pow give the very float glibc's
    gives for the case's own (alpha, a0) — or is alpha outside the cone, where no pow is taken?
    Returns (agree, within): `within` = the two narrowed values are at most one float ulp apart."""
    alpha, cos_theta, a0 = sc.cone_alpha(c)
    got = np.zeros(len(c), F32)
    hw.scalar("pow_general", alpha, np.full(len(c), a0, F32), o1=got)
    with np.errstate(all="ignore"):
        want = pc.libm_pow(alpha.astype(F64), np.full(len(c), a0, F64)).astype(F32)
        outside = alpha < cos_theta
    same = same_bits32(got, want) | outside
    return same, same | (ulps32(got, want) <= 1)


def shade_mismatches(hw, name, form, cuda=False):
    """(cases, mismatches, first, relaxed) of one form over a family: every case compared (cuda:
    every case but the phantom's, which cu_shade does not have)."""
    res, _ = sc.shade_reference(name, cuda=cuda)
    cases = bad_total = relaxed = 0
    first = None
    for c, ref in zip(sc.SHADE_FAMILIES[name](), res):
        if cuda:
            c = c.real()
        if form == "staged" and not hw.lit_info(c.js)[2]:
            assert not stage_fits(c.js)
            continue
        rgb, zero = hw.shade(form, c)
        bad = ~same_bits32(rgb, ref[0]).all(1)
        if name == "cone_general":
            # The contract's one exception.  Where the two pows give the same float for the case's
            # own alpha, every bit is compared as everywhere else.  Where they do not, ang may be
            # one float ulp off (asserted), and the colour — ((dif + spe) * rad) * ang added to +0
            # and multiplied by the opacity: two roundings after ang — at most 4 ulps a channel.
            agree, within = pow_agreement(hw, c)
            loose = ~agree & within & (ulps32(rgb, ref[0]) <= 4).all(1)
            relaxed += int((~agree).sum())
            bad &= ~loose
            bad |= ~within
        if not cuda:
            bad |= zero != ref[1]
        cases += len(c)
        bad_total += int(bad.sum())
        if bad.any() and first is None:
            i = int(np.flatnonzero(bad)[0])
            first = (c, i, f"rgb {_hex32(rgb[i])} zero {zero[i]}", f"rgb {_hex32(ref[0][i])} zero {ref[1][i]}")
    return cases, bad_total, first, relaxed


@pytest.mark.parametrize("name", list(sc.SHADE_FAMILIES))
def test_shade(hw, name):
    """shade from global records, shade with the scene staged in LDS (stage_scene<true>, where the
    pixel kernels would stage it) and cu_shade, against o_shade / c_shade.  Every form runs every
    case it applies to: the counts are checked against the lists themselves."""
    fam = sc.SHADE_FAMILIES[name]()
    expect = {"shade": sum(len(c) for c in fam),
              "staged": sum(len(c) for c in fam if stage_fits(c.js)),
              "cuda": sum(int((c.idx >= 0).sum()) for c in fam)}
    assert expect["shade"] == sc.family_size(name) and expect["staged"] > 0 and expect["cuda"] > 0
    for form, cuda in (("shade", False), ("staged", False), ("cuda", True)):
        cases, bad, first, relaxed = shade_mismatches(hw, name, form, cuda)
        print(f"[gpu_shading] {name}/{form}: {cases} cases, {bad} mismatches"
              + (f", {relaxed} cases where the device pow and glibc's differ" if name == "cone_general" else ""))
        if first:
            _fail_shade(f"{name}/{form}", *first)
        assert cases == expect[form], (form, cases, expect[form])


def test_shade_mutants_are_caught(hw):
    """The lists have teeth: `inert` without its finiteness tests, alpha as the negated dot product
    with ld, and no second zero event for a spot light P sits on each differ from the oracle."""
    caught = {}
    for form in ("mut_inert", "mut_alpha", "mut_zero"):
        per = {name: shade_mismatches(hw, name, form)[1] for name in sc.SHADE_FAMILIES}
        assert form != "mut_alpha" or per["cone"] > 0
        caught[form] = sum(per.values())
        print(f"[gpu_shading] mutant {form}: {caught[form]} cases caught "
              + ", ".join(f"{k} {v}" for k, v in per.items() if v))
    assert all(caught.values()), f"a mutant passes the case lists: {caught}"


def test_pow_general_probe(hw):
    """(float)pow((double)alpha, (double)a0) with the device library's pow against glibc's, on a
    sweep of alpha beside the cone_general family's own values: the source of the "differ at all"
    count.  (shade's general branch itself is the cone_general family of test_shade.)"""
    al, a0 = sc.family_pow_general()
    got = np.zeros(len(al), F32)
    hw.scalar("pow_general", al, a0, o1=got)
    with np.errstate(all="ignore"):
        want = pc.libm_pow(al.astype(F64), a0.astype(F64)).astype(F32)
    same = same_bits32(got, want)
    fin = np.isfinite(got) & np.isfinite(want)
    far = ~same & ~(fin & ((got == pc.nudge32(want, np.ones(len(want), np.int64)))
                           | (got == pc.nudge32(want, -np.ones(len(want), np.int64)))))
    print(f"[gpu_shading] pow_general probe: {len(al)} cases, {int((~same).sum())} differ at all, "
          f"{int(far.sum())} by more than one float ulp")
    if far.any():
        i = int(np.flatnonzero(far)[0])
        pytest.fail(f"pow case {i}: alpha {_hex32(al[i])} a0 {a0[i]} | device {_hex32(got[i])} | glibc "
                    f"{_hex32(want[i])}")


# ---------------------------------------------------------------------------- shoot --
def _check(what, c, bad, dev, ref):
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        pytest.fail(f"{what} [{c.label}]: case {i} of {len(c)}: d {_hex32(c.d[i])} carry {_hex32(c.carry[i])} "
                    f"maxrec {c.maxrec} | device {dev(i)} | reference {ref(i)}")


def test_shoot(hw):
    """shoot<kModeFast>, <kModeParityA>, <kModeParityC> from the case's carry-in, <kModeClassify>,
    and shade_dep_cont on the lines phase A produces (with dep_fast as the library derives it, and
    phase C's full shoot where it is off), against o_shoot."""
    tot = {}

    def add(form, cases, bad):
        a = tot.setdefault(form, [0, 0])
        a[0] += cases
        a[1] += int(bad.sum())

    flagged = 0
    for c in sc.family_shoot():
        f_rgb, f_cls, f_cout, f_zero, _ = sc.ref_shoot(c.js, c.d, c.maxrec, "fast", c.carry)
        p_rgb, p_cls, p_cout, p_zero, _ = sc.ref_shoot(c.js, c.d, c.maxrec, "parity", c.carry)
        # fast
        rgb, cls, cout, zero, _ = hw.shoot("fast", c)
        wrote = (f_cls & 1) != 0
        bad = ~same_bits32(rgb, f_rgb).all(1) | (zero != f_zero) | (cls != (f_cls & 1))
        bad |= wrote & ~same_bits32(cout, f_cout).all(1)
        add("fast", len(c), bad)
        _check("shoot<fast>", c, bad, lambda i: f"rgb {_hex32(rgb[i])} cls {cls[i]} carry {_hex32(cout[i])} zero {zero[i]}",
               lambda i: f"rgb {_hex32(f_rgb[i])} cls {f_cls[i]} carry {_hex32(f_cout[i])} zero {f_zero[i]}")
        # phase C: the whole pixel from its carry-in
        rgb, cls, cout, zero, _ = hw.shoot("parity_c", c)
        wrote = (p_cls & 1) != 0
        bad = ~same_bits32(rgb, p_rgb).all(1) | (zero != p_zero) | (cls != (p_cls & 1))
        bad |= wrote & ~same_bits32(cout, p_cout).all(1)
        add("parity_c", len(c), bad)
        _check("shoot<parity C>", c, bad, lambda i: f"rgb {_hex32(rgb[i])} cls {cls[i]} carry {_hex32(cout[i])} zero {zero[i]}",
               lambda i: f"rgb {_hex32(p_rgb[i])} cls {p_cls[i]} carry {_hex32(p_cout[i])} zero {p_zero[i]}")
        # phase A and classify: the class; colour, carry and events of the pixels that are not DEP
        dep = p_cls >= 2
        want_cls = np.where(dep, CLS_DEP, p_cls & 1)
        for form in ("parity_a", "classify"):
            rgb, cls, cout, zero, _ = hw.shoot(form, c)
            bad = cls != want_cls
            bad |= ~dep & (p_cls == 1) & ~same_bits32(cout, p_cout).all(1)
            if form == "parity_a":
                bad |= ~dep & (~same_bits32(rgb, p_rgb).all(1) | (zero != p_zero))
            else:
                bad |= (pc.bits32(rgb) != 0).any(1)
            add(form, len(c), bad)
            _check(f"shoot<{form}>", c, bad, lambda i: f"rgb {_hex32(rgb[i])} cls {cls[i]} carry {_hex32(cout[i])} zero {zero[i]}",
                   lambda i: f"rgb {_hex32(p_rgb[i])} cls {p_cls[i]} carry {_hex32(p_cout[i])} zero {p_zero[i]}")
        # phase A + shade_dep_cont: a DEP pixel's colour and events from its carry-in
        rgb, cls, cout, zero, flag = hw.shoot("dep_cont", c)
        dep_fast = hw.lit_info(c.js)[1]
        bad = (flag != 0) != (dep & bool(dep_fast))
        done = flag != 0
        bad |= done & (~same_bits32(rgb, p_rgb).all(1) | (zero != p_zero))
        flagged += int(done.sum())
        add("dep_cont", len(c), bad)
        _check("shade_dep_cont", c, bad, lambda i: f"rgb {_hex32(rgb[i])} flag {flag[i]} zero {zero[i]}",
               lambda i: f"rgb {_hex32(p_rgb[i])} cls {p_cls[i]} zero {p_zero[i]} dep_fast {dep_fast}")
        # ... and with dep_fast forced off nothing takes the shortcut: phase A's outputs as they are
        if dep_fast:
            o_rgb, o_cls, o_cout, o_zero, o_flag = hw.shoot("dep_cont", c, dep_fast=0)
            a_rgb, a_cls, a_cout, a_zero, _ = hw.shoot("parity_a", c, dep_fast=0)
            bad = (o_flag != 0) | (o_cls != a_cls) | (o_zero != a_zero) | ~same_bits32(o_rgb, a_rgb).all(1)
            bad |= (a_cls != want_cls)
            add("dep_fast off", len(c), bad)
            _check("dep_cont with dep_fast off", c, bad, lambda i: f"flag {o_flag[i]} cls {o_cls[i]} zero {o_zero[i]}",
                   lambda i: f"flag 0 cls {a_cls[i]} zero {a_zero[i]}")
    assert tot["dep_fast off"][0] >= 1000
    for form, (cases, bad) in tot.items():
        print(f"[gpu_shading] shoot/{form}: {cases} cases, {bad} mismatches")
    print(f"[gpu_shading] shade_dep_cont ran on {flagged} DEP pixels")
    assert flagged >= 1000


def test_cuda_render_pixel(hw):
    """cusem::render_pixel over the 64 x 48 camera of every golden and random scene and of the
    facing mirrors, max_iter 0, 1 and 49, against c_shoot on the CUDA port's primary rays."""
    W, H = 64, 48
    x, y = np.meshgrid(np.arange(W, dtype=I32), np.arange(H, dtype=I32))
    xy = np.stack([x.ravel(), y.ravel()], 1)
    scenes = {k: v for k, v in sc.lit_scenes().items() if not k.startswith("lights")}
    scenes["mirrors"] = sc.family_shoot()[-2].scene
    scenes["mirrors/m=0"] = sc.family_shoot()[-1].scene
    cases = mism = 0
    for name, s in scenes.items():
        d = sc.camera_dirs_cuda(s.js, W, H)
        for it in sc.CUDA_ITERS:
            want, _ = sc.ref_shoot_cuda(s.js, d, it)
            got = hw.render_pixel(s.js, W, H, it, xy)
            bad = ~same_bits32(got, want).all(1)
            cases, mism = cases + len(xy), mism + int(bad.sum())
            if bad.any():
                i = int(np.flatnonzero(bad)[0])
                pytest.fail(f"render_pixel [{name}] max_iter {it}: pixel {xy[i]} | device {_hex32(got[i])} | "
                            f"reference {_hex32(want[i])}")
    print(f"[gpu_shading] cuda render_pixel: {cases} cases, {mism} mismatches")


# --------------------------------------------------------------------------- scalars --
def test_quant(hw):
    c = sc.family_quant()
    got = np.zeros(len(c), I32)
    hw.scalar("quant", c, o1=got)
    want = sc.ref_quant(c).astype(I32)
    bad = got != want
    print(f"[gpu_shading] quant: {len(c)} cases, {int(bad.sum())} mismatches")
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        pytest.fail(f"quant case {i}: c {_hex32(c[i])} | device {got[i]} | reference {want[i]}")


def test_primary_dir(hw):
    cam, pix, xy = sc.family_primary_dir()
    b = np.zeros((len(cam), 4), F32)
    b[:, :2] = pix[:, :2]
    b.view(I32)[:, 2:] = xy
    got, zero = np.zeros((len(cam), 3), F32), np.zeros(len(cam), I32)
    hw.scalar("primary_dir", cam, b, o0=zero, o1=got)
    want, want_zero = sc.primary_dir_ref(cam, pix, xy)
    bad = ~same_bits32(got, want).all(1) | (zero != want_zero)
    print(f"[gpu_shading] primary_dir: {len(cam)} cases, {int(bad.sum())} mismatches")
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        pytest.fail(f"primary_dir case {i}: hx hy {cam[i]} pw ph {_hex32(pix[i, :2])} x y {xy[i]} | device "
                    f"{_hex32(got[i])} zero {zero[i]} | reference {_hex32(want[i])}")
