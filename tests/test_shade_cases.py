"""The case lists of the hit-level suite (tests/shade_cases.py) put their cases on the edges, and the
oracle's hit-level exports are the renderer's own code.  CPU only.

Edges: every family's named edge is counted by the counters o_shade / o_shoot bump themselves
(rco_shade_counts, oracle/rc_oracle.h) and has a floor of at least 1 % of the family, chosen from
what the seeded generators give.  No case is ever left out of a comparison on the device
(tests/test_gpu_shading.py), so these floors are what keeps a family from passing vacuously.

Identity: rco_prim_shoot + rco_prim_quant over the 64 x 48 camera reproduce rco_render byte for
byte on the six golden scenes (fast mode, and parity mode with the carry chained in scan order);
the _cuda forms reproduce rco_render_cuda.  Each test prints its counts (pytest -s)."""
import ctypes

import numpy as np
import pytest

import prim_cases as pc
import shade_cases as sc
from helpers import oracle_lib, oracle_render, oracle_render_cuda

F32, I32 = np.float32, np.int32


def _report(name, **counts):
    print(f"[shade_cases] {name}: " + ", ".join(f"{k}={v}" for k, v in counts.items()))


def _family(name):
    n = sc.family_size(name)
    res, cnt = sc.shade_reference(name)
    _report(name, cases=n, scenes=len(res), **{k: v for k, v in cnt.items() if v})
    assert 0 < n <= sc.MAX_CASES and cnt["shades"] == n
    return n, res, cnt


def _floor(n):
    return max(1, (n + 99) // 100)      # 1 % of the family


@pytest.mark.parametrize("name", sorted(sc.SHADE_FAMILIES))
def test_family_is_deterministic(name):
    a = sc.SHADE_FAMILIES[name]()
    sc.SHADE_FAMILIES[name].cache_clear()
    b = sc.SHADE_FAMILIES[name]()
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.label == y.label and np.array_equal(x.idx, y.idx)
        for u, v in ((x.P, y.P), (x.N, y.N), (x.D, y.D)):
            assert np.array_equal(pc.bits32(u), pc.bits32(v))
        n = x.js.num_shapes
        assert x.idx.min() >= -1 and x.idx.max() < n


def test_lit_coverage():
    n, res, cnt = _family("lit")
    lights = {c.label: c.js.num_lights for c in sc.family_lit()}
    assert {0, 1, 3, 6} <= set(lights.values()) and lights["lights0"] == 0 and lights["lights6"] == 6
    assert {c.js.num_shapes for c in sc.family_lit()} >= {14, 64, 65}
    assert all(len(c) >= 2000 for c in sc.family_lit())
    f = _floor(n)
    for k in ("shadowed", "th_le0", "spot", "cone_out", "alpha_neg_in", "specular"):
        assert cnt[k] >= f, (k, cnt[k], f)
    assert cnt["lights"] - cnt["shadowed"] - cnt["th_le0"] >= 10 * f      # lit, facing the light


def test_terminator_coverage():
    n, res, cnt = _family("terminator")
    f = _floor(n)
    assert cnt["shadowed"] * 2 == cnt["lights"] == n                      # with and without occluder
    free = n - cnt["shadowed"]
    pos = free - cnt["th_le0"] - cnt["th_nan"]
    assert cnt["th_le0"] >= 10 * f and pos >= 10 * f and cnt["th_nan"] >= f
    assert cnt["rad_nonfinite"] >= 10 * f                                 # where `inert` must not fire
    # th is EXACTLY +-0, and the smallest values of both signs, by numpy's float32 arithmetic
    c = sc.family_terminator()[0]
    v = -c.P
    ln = np.sqrt((v.astype(np.float64) ** 2).sum(1)).astype(F32)
    with np.errstate(all="ignore"):
        ld = v / ln[:, None]
        th = c.N[:, 0] * ld[:, 0]
        th = th + c.N[:, 1] * ld[:, 1]
        th = th + c.N[:, 2] * ld[:, 2]
    zero, tiny = th == 0, (th != 0) & (np.abs(th) < 1e-30)
    _report("terminator/theta", zero=int(zero.sum()), neg_zero=int((zero & np.signbit(th)).sum()),
            tiny_pos=int((tiny & (th > 0)).sum()), tiny_neg=int((tiny & (th < 0)).sum()))
    k = _floor(len(c))
    assert (zero & np.signbit(th)).sum() >= k and (zero & ~np.signbit(th)).sum() >= k
    assert (tiny & (th > 0)).sum() >= k and (tiny & (th < 0)).sum() >= k


def test_on_light_coverage():
    n, res, cnt = _family("on_light")
    zero = np.concatenate([z for _, z in res])
    counts = {k: int((zero == k).sum()) for k in (0, 1, 2)}
    _report("on_light/events", **{f"zero{k}": v for k, v in counts.items()})
    f = _floor(n)
    assert cnt["dist0"] >= 10 * f and cnt["shadowed"] >= f
    assert all(v >= 10 * f for v in counts.values()) and zero.max() == 2
    free, inside = res
    c = sc.family_on_light()[0]
    on_spot = np.all(pc.bits32(c.P) == pc.bits32(np.array([-2.0, 0.5, -6.0], F32)), 1)
    # a shadow ray with D = +0 hits nothing, even from inside a sphere: two events either way
    assert on_spot.sum() >= 10 and np.all(free[1][on_spot] == 2) and np.all(inside[1][on_spot] == 2)


def test_cone_coverage():
    n, res, cnt = _family("cone")
    f = _floor(n)
    assert len(res) == len(sc.CONE_EXPONENTS) * len(sc.CONE_COS) * len(sc.CONE_DIRS)
    assert {0, 1, 2, -1, -3, -9, 3, 20, 31, 64, -64} == set(sc.CONE_EXPONENTS)
    assert min(sc.CONE_COS) < 0 and 0.0 in sc.CONE_COS and 1.0 in sc.CONE_COS
    for k in ("cone_out", "alpha_eq_cos", "alpha_zero", "alpha_neg_in", "ang_nonfinite", "dist0"):
        assert cnt[k] >= f, (k, cnt[k], f)
    assert cnt["spot"] == cnt["lights"] == n and cnt["shadowed"] == 0
    # the concrete miss: alpha == +-0 inside a cone of 90 degrees or more under a negative odd exponent
    hot = 0
    for c, (rgb, _) in zip(sc.family_cone(), res):
        L = c.js.lights_list.contents
        if L.a0 in (-1.0, -3.0, -9.0) and L.cos_theta <= 0:
            hot += int(np.isinf(rgb).any(1).sum())
    _report("cone/inf under a negative odd exponent", cases=hot)
    assert hot >= 100


def test_cone_general_coverage():
    """Exponents the packer must NOT treat as small integers (rc_scene.c: nearbyintf(a0) == a0 and
    |a0| <= 64): non-integers and 65, 100, -65.  shade_cases.cone_alpha, which the device test uses
    to ask where the two pows differ, is the oracle's alpha: its counts are the oracle's counters."""
    n, res, cnt = _family("cone_general")
    f = _floor(n)
    assert {2.5, 7.25, -0.5, 65.0, 100.0} <= set(sc.GENERAL_EXPONENTS)
    assert all(e != np.rint(e) or abs(e) > 64 for e in sc.GENERAL_EXPONENTS)
    fam = sc.family_cone_general()
    assert len(fam) == len(sc.GENERAL_EXPONENTS) * len(sc.CONE_COS) * len(sc.CONE_DIRS)
    assert cnt["spot"] == cnt["lights"] == n and cnt["shadowed"] == 0
    inside = cnt["spot"] - cnt["cone_out"]
    assert inside >= 10 * f and cnt["alpha_zero"] >= f and cnt["alpha_neg_in"] >= f
    assert cnt["ang_nonfinite"] >= f
    out = zero = eq = 0
    for c in fam:
        alpha, cos_theta, a0 = sc.cone_alpha(c)
        with np.errstate(invalid="ignore"):
            out += int((alpha < cos_theta).sum())
            zero += int((alpha == 0).sum())
            eq += int((alpha == cos_theta).sum())
    assert (out, zero, eq) == (cnt["cone_out"], cnt["alpha_zero"], cnt["alpha_eq_cos"])
    # ordinary values of ang are there too: 0 < ang < inf
    rgb = np.concatenate([r for r, _ in res])
    assert (np.isfinite(rgb).all(1) & (rgb > 0).any(1)).sum() >= 10 * f


def test_radial_coverage():
    n, res, cnt = _family("radial")
    assert cnt["rad_nonfinite"] >= 10 * _floor(n) and cnt["shadowed"] == 0
    rgb = np.concatenate([r for r, _ in res])
    assert np.isnan(rgb).any() and np.isinf(rgb).any() and (rgb < 0).any()


def test_specular_coverage():
    n, res, cnt = _family("specular")
    f = _floor(n)
    assert cnt["specular"] >= 10 * f and cnt["spec_arg_nan"] >= f
    assert 2 * (cnt["lights"] - cnt["th_le0"] - cnt["th_nan"]) - cnt["specular"] >= f   # angle > 0 too


def test_opacity_coverage():
    n, res, cnt = _family("opacity")
    f = _floor(n)
    assert cnt["opacity_le0"] >= 10 * f and cnt["phantom"] >= 10 * f
    lit_phantoms = 0
    for c, (rgb, _) in zip(sc.family_opacity(), res):
        if c.label.startswith("phantom"):
            lit_phantoms += int((rgb[c.idx < 0] != 0).any(1).sum())
    _report("opacity/lit phantom shades", cases=lit_phantoms)
    assert lit_phantoms >= f


def test_nonfinite_coverage():
    n, res, cnt = _family("nonfinite")
    f = _floor(n)
    assert cnt["th_nan"] >= 10 * f and cnt["rad_nonfinite"] >= 10 * f and cnt["shadowed"] >= f


def test_pow20_argument_domain():
    """pow20's stated domain (rc_device.hpp): |x| <= 2^50 or NaN, and |x| <= 4 where every normal is
    a unit one — the oracle's own argument of pow(angle, 20) over every shading family and over the
    bounce loops.  example2's plane normal (0, 4, 0) is not a unit vector: its figure is printed."""
    worst, worst_unit = 0.0, 0.0
    for name in sc.SHADE_FAMILIES:
        for c in sc.SHADE_FAMILIES[name]():
            v = sc.ref_shade(c.js, c.idx, c.P, c.N, c.D)[2]["spec_arg_max"]
            worst = max(worst, v)
            if c.label != "example2":
                worst_unit = max(worst_unit, v)
            else:
                _report("pow20 argument, example2", max_abs=v)
    for c in sc.family_shoot():
        v = sc.ref_shoot(c.js, c.d, c.maxrec, "parity", c.carry)[4]["spec_arg_max"]
        worst = max(worst, v)
        if not c.label.startswith("example2"):
            worst_unit = max(worst_unit, v)
    _report("pow20 argument", max_abs=worst, max_abs_unit_normals=worst_unit)
    assert worst <= 2.0 ** 50 and worst_unit <= 4.0


def test_shoot_coverage():
    fam = sc.family_shoot()
    n = sum(len(c) for c in fam)
    assert 0 < n <= sc.MAX_CASES
    assert {c.maxrec for c in fam} >= {1, 2, 3, 6, 7}
    assert {c.js.num_shapes for c in fam} >= {64, 65} and any(c.js.num_lights == 0 for c in fam)
    for mode in ("fast", "parity"):
        tot = None
        for c in fam:
            cnt = sc.ref_shoot(c.js, c.d, c.maxrec, mode, c.carry)[4]
            tot = cnt if tot is None else sc.add_counts(tot, cnt)
        _report(f"shoot/{mode}", cases=n, **{k: v for k, v in tot.items() if v})
        f = _floor(n)
        assert tot["shoots"] == n
        for k in ("bounce_iters", "end_maxrec", "end_nonrefl", "primary_miss", "phantom"):
            assert tot[k] >= f or (k == "phantom" and mode == "fast"), (mode, k, tot[k])
        assert (tot["end_miss"] >= f and tot["dep"] == 0) if mode == "fast" else tot["dep"] >= f
    assert any(np.any(c.carry) for c in fam)


def test_quant_family():
    c = sc.family_quant()
    assert len(c) <= sc.MAX_CASES
    with np.errstate(all="ignore"):
        v = c.astype(F32) * F32(255.0)
    def ordered(x):                                    # places along the float line, -0 = +0 = 0
        i = pc.bits32(x).astype(np.int64)
        return np.where(i & 0x80000000, -(i & 0x7fffffff), i)
    for k in range(257):
        near = np.abs(ordered(v) - ordered(np.array([k], F32))[0]) <= 4
        assert near.sum() >= 3 and (v[near] < k).any() == (k > 0) and (v[near] >= k).any(), k
    assert np.isnan(c).sum() >= 8 and np.signbit(c[np.isnan(c)]).any() and np.isinf(c).sum() == 2
    q = sc.ref_quant(c)
    assert set(q.tolist()) == set(range(256)) and np.all(q[np.isnan(c)] == 0)
    _report("quant", cases=len(c), nan=int(np.isnan(c).sum()))


def test_primary_dir_family():
    cam, pix, xy = sc.family_primary_dir()
    d, z = sc.primary_dir_ref(cam, pix, xy)
    assert len(d) <= sc.MAX_CASES and xy.max() == 33554432 and not np.isnan(d).any()
    assert np.all(np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1) < 1e-6)
    # the reference is prim_cases.primary_dirs' arithmetic, which the identity tests below pin
    W, H = 64, 48
    sel = (np.round(2.0 / pix[:, 0]) == W) & (np.round(2.0 / pix[:, 1]) == H) & (cam[:, 0] == -1.0) \
        & (cam[:, 1] == 1.0)
    assert sel.sum() >= 16
    want = pc.primary_dirs(2.0, 2.0, W, H).reshape(H, W, 3)[xy[sel, 1], xy[sel, 0]]
    assert np.array_equal(pc.bits32(d[sel]), pc.bits32(want))
    _report("primary_dir", cases=len(d))


# ------------------------------------------------------ the exports are the renderer --
@pytest.mark.parametrize("name", pc.GOLDEN_SCENES)
@pytest.mark.parametrize("maxrec", [7, 3])
def test_shoot_and_quant_are_the_render(name, maxrec):
    s = sc.lit_scenes()[name]
    W, H = 64, 48
    d = sc.camera_dirs(s.js, W, H)
    want, _ = oracle_render(s, W, H, maxrec - 1, "fast")
    rgb, cls, cout, zero, _ = sc.ref_shoot(s.js, d, maxrec, "fast")
    assert np.array_equal(sc.ref_quant(rgb.ravel()).reshape(H, W, 3), want)
    # parity: the carry chained in scan order, one pixel a call
    want, st, cin_want = oracle_render(s, W, H, maxrec - 1, "parity", with_carry=True)
    lib = oracle_lib()
    cls_want = np.zeros(W * H, np.uint8)
    img = np.zeros((H, W, 3), np.uint8)
    r = lib.rco_render_cls(ctypes.byref(s.js), W, H, maxrec, 0, img.ctypes.data_as(ctypes.c_void_p),
                           None, None, cls_want.ctypes.data_as(ctypes.c_void_p))
    assert r == 0 and np.array_equal(img, want)
    got = np.zeros((W * H, 3), F32)
    carry = np.zeros((1, 3), F32)
    cls_got = np.zeros(W * H, np.uint8)
    events = 0
    for i in range(W * H):
        g, k, co, z, _ = sc.ref_shoot(s.js, d[i:i + 1], maxrec, "parity", carry)
        if k[0] >= 2:                                   # a DEP pixel read exactly this carry
            assert np.array_equal(pc.bits32(cin_want.reshape(-1, 3)[i]), pc.bits32(carry[0]))
        got[i], cls_got[i], carry, events = g[0], k[0], co, events + int(z[0])
    assert np.array_equal(sc.ref_quant(got.ravel()).reshape(H, W, 3), want)
    assert np.array_equal(cls_got, cls_want)
    assert events == st["zero_normalize"]               # the primary rays' normalize adds none
    _report(f"{name} maxrec {maxrec}", dep=int((cls_got >= 2).sum()), writers=int((cls_got & 1).sum()))


@pytest.mark.parametrize("name", pc.GOLDEN_SCENES)
def test_cuda_shoot_and_quant_are_the_render(name):
    s = sc.lit_scenes()[name]
    W, H = 64, 48
    d = sc.camera_dirs_cuda(s.js, W, H)
    for it in sc.CUDA_ITERS:
        rgb, _ = sc.ref_shoot_cuda(s.js, d, it)
        assert np.array_equal(sc.ref_quant(rgb.ravel()).reshape(H, W, 3), oracle_render_cuda(s, W, H, it)), it
