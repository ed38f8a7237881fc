"""The case lists of the ray-level suite (tests/prim_cases.py) put their cases on the edges: the
coverage conditions of every family, checked with the CPU oracle's own branch counters
(rco_prim_counts) and numpy alone.  No case is ever left out of a comparison on the device
(tests/test_gpu_prims.py), so these conditions are what keeps a family from passing vacuously.
CPU only; each test prints its family's counts (pytest -s, or the captured output of a failure)."""
import numpy as np
import pytest

import prim_cases as pc


def _report(name, **counts):
    print(f"[prim_cases] {name}: " + ", ".join(f"{k}={v}" for k, v in counts.items()))


@pytest.mark.parametrize("name", sorted(pc.RAY_FAMILIES))
def test_family_sizes_and_determinism(name):
    c = pc.RAY_FAMILIES[name]()
    assert 0 < len(c) <= pc.MAX_CASES
    n = c.js.num_shapes
    assert c.shape.min() >= 0 and c.shape.max() < n and c.skip.min() >= -1 and c.skip.max() < n
    pc.RAY_FAMILIES[name].cache_clear()
    d = pc.RAY_FAMILIES[name]()
    for a, b in ((c.O, d.O), (c.D, d.D)):
        assert np.array_equal(pc.bits32(a), pc.bits32(b))
    assert np.array_equal(c.shape, d.shape) and np.array_equal(c.skip, d.skip)


def test_tangent_coverage():
    """By the reference, both outcomes — disc < 0 and accepted — are at least 20 % of the family."""
    allc, own = pc.coverage("tangent")
    _report("tangent", **own)
    assert own["cases"] == allc["cases"] >= 5000
    assert own["disc_neg"] >= 0.2 * own["cases"]
    assert own["accepted"] >= 0.2 * own["cases"]
    assert own["sphere"] >= 1000 and own["quadric"] >= 1000


def test_surface_coverage():
    """O on the surface with skip both the hit shape and -1, and at least 64 hand-built cases whose
    root is exactly +-0."""
    c = pc.family_surface()
    allc, own = pc.coverage("surface")
    _report("surface", **own)
    assert np.count_nonzero(c.own & (c.skip == c.shape)) >= 1000
    assert np.count_nonzero(c.own & (c.skip == -1)) >= 1000
    zO, zD, zsh = pc.zero_root_rays()
    hit, t, z = pc.ref_shape(c.js, zO, zD, zsh, np.full(len(zsh), -1, pc.I32))
    _report("surface/zero-roots", cases=len(zsh), t_zero=z["t_zero"],
            neg_zero=int(np.count_nonzero((t == 0) & np.signbit(t) & (hit != 0))))
    assert z["t_zero"] >= 64
    assert np.any((t == 0) & np.signbit(t) & (hit != 0)) and np.any((t == 0) & ~np.signbit(t) & (hit != 0))
    # a ray leaving its own surface: roots near zero of either sign, so all three classes occur
    assert own["accepted"] >= 500 and own["t_neg"] + own["t_zero"] >= 500 and own["second_root"] >= 500
    assert own["sphere"] and own["plane"] and own["quadric"]


def test_branches_coverage():
    """At least 1 000 cases with a_q == 0 exactly, 64 of them with b_q == 0 as well; the z rule
    fires and does not fire."""
    allc, own = pc.coverage("branches")
    _report("branches", **own)
    assert own["linear"] >= 1000 and own["linear_b0"] >= 64
    assert own["linear"] - own["linear_b0"] >= 1000
    assert own["z_rule"] >= 64 and own["accepted"] >= 64
    c = pc.family_branches()
    tiny = (np.abs(c.D[:, 2]) < 1e-20) & (c.skip != -1)
    assert np.count_nonzero(tiny & (c.D[:, 2] == 0) & np.signbit(c.D[:, 2])) >= 64
    assert np.count_nonzero(tiny & (c.D[:, 2] == 0) & ~np.signbit(c.D[:, 2])) >= 64
    assert np.count_nonzero(tiny & (c.D[:, 2] != 0)) >= 64


def test_plane_coverage():
    allc, own = pc.coverage("plane")
    _report("plane", **own)
    for k in ("plane_den0", "plane_den_sub", "plane_num0", "t_inf", "t_zero", "accepted"):
        assert own[k] >= 64, k
    assert own["cases"] - own["hits"] - own["plane_den0"] >= 64      # refused for t < 0


def test_nonfinite_coverage():
    """At least 256 cases raise the reference's NaN-cross-term counter."""
    allc, _ = pc.coverage("nonfinite")
    _report("nonfinite", **allc)
    assert allc["cross_nan"] >= 256
    assert allc["t_nan"] >= 256 and allc["accepted"] >= 64
    c = pc.family_nonfinite()
    assert np.any(np.isinf(c.O)) and np.any(np.isnan(c.O)) and np.any(np.isinf(c.D)) and np.any(np.isnan(c.D))
    O, D = pc.family_x0()
    r = pc.x0_reject_ref(O, D)
    _report("x0_reject", cases=len(r), rejected=int(r.sum()))
    assert r.sum() >= 256 and (~r).sum() >= 256
    fin = np.isfinite(O).all(1) & np.isfinite(D).all(1)
    assert np.count_nonzero(r & fin) >= 64          # finite O and D whose cross sums overflow


def test_random_and_primary_coverage():
    for name in ("random", "primary"):
        allc, _ = pc.coverage(name)
        _report(name, **allc)
        assert allc["accepted"] >= 1000 and allc["disc_neg"] >= 1000
    c = pc.family_primary()
    assert not c.O.any() and not np.signbit(c.O).any()          # O = (+0, +0, +0)


def test_cuda_port_reference_runs_the_same_cases():
    """The CUDA port's shape tests (c_*) take the linear branch and the disc < 0 exit on the
    same families."""
    c = pc.family_branches()
    _, _, cnt = pc.ref_shape(c.js, c.O, c.D, c.shape, c.skip, cuda=True)
    _report("branches/cuda", **cnt)
    assert cnt["linear"] >= 1000 and cnt["linear_b0"] >= 64
    c = pc.family_tangent()
    _, _, cnt = pc.ref_shape(c.js, c.O, c.D, c.shape, c.skip, cuda=True)
    assert cnt["disc_neg"] >= 0.2 * cnt["cases"] and cnt["accepted"] >= 0.2 * cnt["cases"]


def test_division_coverage():
    num, den, regular = pc.family_division()
    assert len(num) == len(den) <= pc.MAX_CASES
    d = den[regular]
    _, e = np.frexp(np.abs(d))
    have = set((e - 1).tolist())
    assert all(k in have for k in range(-149, 129))     # (double)f and 2 (double)f, f = 2^-149 .. 2^127
    an = np.abs(num[regular])
    _report("division", cases=len(num), regular=int(regular.sum()),
            min_abs_num=float(an.min()), max_abs_num=float(an.max()))
    assert an.min() <= 2.0 ** -190 and an.max() >= 2.0 ** 128
    s = ~regular
    for v in (num[s], den[s]):
        assert np.any(v == 0) and np.any(np.isinf(v)) and np.any(np.isnan(v))
    for v in (num[regular], den[regular]):              # subnormal floats, widened
        assert np.count_nonzero(np.abs(v) < 2.0 ** -126) >= 64


def test_division_hard_cases():
    """The constructed quotients are within 2^-53 ulp of a rounding midpoint, by rational
    arithmetic, and numpy's IEEE division rounds them to the nearer neighbour."""
    from fractions import Fraction
    n, d = pc.division_hard_cases(np.random.default_rng(5), 64)
    with np.errstate(all="ignore"):
        q = n / d
    for a, b, c in zip(n, d, q):
        exact = Fraction(float(a)) / Fraction(float(b))
        ulp = Fraction(float(np.spacing(abs(c))))
        other = Fraction(float(np.nextafter(c, np.inf if exact > Fraction(float(c)) else -np.inf)))
        mid = (Fraction(float(c)) + other) / 2
        assert abs(exact - Fraction(float(c))) < abs(exact - other)
        assert 0 < abs(exact - mid) < ulp / 2 ** 53


def test_sqrt_hard_cases():
    """The constructed inputs' roots are within 2^-43 ulp of a rounding midpoint (integer
    arithmetic), and numpy's IEEE sqrt rounds them to the nearer neighbour."""
    from fractions import Fraction
    s = pc.sqrt_hard_cases()
    assert len(s) >= 2000
    r = np.sqrt(s)
    for a, b in zip(s[::37], r[::37]):
        a, b, half = Fraction(float(a)), Fraction(float(b)), Fraction(float(np.spacing(b))) / 2
        assert (b - half) ** 2 < a < (b + half) ** 2                # b is the nearest double
        mid = b + half if a > b * b else b - half
        # |sqrt(a) - mid| = |a - mid^2| / (sqrt(a) + mid) < 2^-43 ulp
        assert 0 < abs(a - mid * mid) < (2 * half) * (2 * mid) * Fraction(1, 2 ** 43)


def test_sqrt_coverage():
    s = pc.family_sqrt()
    assert len(s) <= pc.MAX_CASES
    fin = s[np.isfinite(s) & (s > 0)]
    assert fin.min() >= 2.0 ** -767
    _, e = np.frexp(fin)
    have = set((e - 1).tolist())
    _report("sqrt", cases=len(s), binades=len(have))
    assert all(k in have for k in range(-767, 1024))
    assert np.any((s == 0) & np.signbit(s)) and np.any((s == 0) & ~np.signbit(s))
    assert np.any(np.isinf(s)) and np.any(np.isnan(s))
    r = np.sqrt(fin)
    assert np.count_nonzero(r * r == fin) >= 10000       # perfect squares (beside their neighbours)


def test_vec_coverage():
    a, ln, a3, l3 = pc.family_vec()
    assert len(a) <= pc.MAX_CASES and len(a3) <= pc.MAX_CASES
    _report("length/div3", length_cases=len(a), div3_cases=len(a3),
            len_inf=int(np.isinf(ln).sum()), len_zero=int((ln == 0).sum()))
    assert np.isinf(ln).sum() >= 1000
    with np.errstate(all="ignore"):
        s32 = (a * a).sum(1, dtype=pc.F32)
    assert np.count_nonzero((s32 < 2.0 ** -126) & (ln != 0)) >= 1000    # subnormal in float
    e = np.frexp(np.abs(a[a != 0]).astype(pc.F64))[1] - 1
    assert e.min() == -149 and e.max() == 127
    assert not np.any(l3 == 0) and np.isinf(l3).any() and np.isnan(l3).any()
    with np.errstate(all="ignore"):
        q = a3.astype(pc.F64) / l3.astype(pc.F64)[:, None]
        exact = np.isfinite(q) & (q.astype(pc.F32).astype(pc.F64) == q) & (q != 0)
    assert exact.sum() >= 5000


def test_quot_class_coverage():
    """Each of the four classes is at least 1 % of the family; the exponent path and the division
    path at least 25 % each; the gaps -160 .. 140 are all there."""
    num, den = pc.family_quot_class()
    assert len(num) <= pc.MAX_CASES
    cls, fast = pc.quot_class_ref(num, den), pc.quot_class_fast(num, den)
    shares = [float(np.mean(cls == k)) for k in range(4)]
    _report("quot_class", cases=len(num), neg=shares[0], zero=shares[1], pos=shares[2],
            other=shares[3], fast=float(fast.mean()))
    assert min(shares) >= 0.01
    assert 0.25 <= fast.mean() <= 0.75
    en = ((pc.bits64(num) >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64)
    ed = ((pc.bits64(den) >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64)
    normal = (en != 0) & (en != 0x7ff) & (ed != 0) & (ed != 0x7ff)
    gaps = set((en - ed)[normal].tolist())
    assert all(g in gaps for g in range(-160, 141))
    # the fast path's claim, on the reference alone: inside its domain the class is the sign's
    assert np.all(np.isin(cls[fast], (0, 2)))


def test_pow_families():
    x = pc.family_pow20()
    assert len(x) == 1 << 15 and x.min() == -1.0 and x.max() == 0.0
    a, n = pc.family_pown()
    assert len(a) <= 1 << 17
    assert (set(pc.POWN_EXPONENTS) | set(pc.PROBE_EXPONENTS) | set(pc.POWN_EDGE_EXPONENTS)
            == set(n.tolist()))
    assert set(pc.POWN_EXPONENTS) == set(list(range(-8, 0)) + list(range(3, 13)) + [20, 31])
    assert set(pc.POWN_EDGE_EXPONENTS) == set(range(-64, 65))
    assert len(pc.POW20_SL) == 16
    # the edge bases meet every exponent: +-0, +-inf, NaN, 1e-30, 1e-10, 1e20, 1e30, 3e38 and negatives
    f = pc.F32
    for b in (0.0, np.inf, 1e-30, 1e-10, 1e20, 1e30, 3e38):
        for s in (1.0, -1.0):
            m = (pc.bits64(a) == pc.bits64(np.array([f(s) * f(b)], np.float64))[0])
            assert set(range(-64, 65)) <= set(n[m].tolist()), (s, b)
    assert set(range(-64, 65)) <= set(n[np.isnan(a)].tolist())
    # ... and libm says what pown_dd has to return there: overflow, underflow and signed zeros
    reg = pc.pown_regular(a, n)
    lm = pc.libm_pow(a[~reg], n[~reg].astype(np.float64))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        nar = lm.astype(pc.F32)
    kinds = dict(inf=int((nar == np.inf).sum()), neg_inf=int((nar == -np.inf).sum()),
                 nan=int(np.isnan(nar).sum()), pos_zero=int(((nar == 0) & ~np.signbit(nar)).sum()),
                 neg_zero=int(((nar == 0) & np.signbit(nar)).sum()))
    assert all(v >= 100 for v in kinds.values()), kinds
    # outside the regular cases the narrowed power is never an ordinary number but 1, +-a or a*a
    odd = ~np.isin(n[~reg], (0, 1, 2)) & np.isfinite(nar) & (nar != 0)
    assert not odd.any()
    _report("pow", pow20_cases=len(x), pown_cases=len(a), pown_edge_cases=int((~reg).sum()), **kinds)


def test_libm_pow_against_exact_rounding():
    """The measurement behind the parity claim: libm's pow(x, 20) is not the
    exactly rounded power for every input — it only has to be within one ulp of it."""
    x = pc.family_pow20()[:4096]
    lm, ex = pc.libm_pow(x, 20.0), pc.exact_pow(x, 20)
    d = pc.ulp_distance(lm, ex)
    _report("libm pow(x, 20) vs exact", cases=len(x), differ=int((d != 0).sum()), max_ulp=int(d.max()))
    assert d.max() <= 1


@pytest.mark.parametrize("name", pc.GOLDEN_SCENES + ["random14x", "random65"])
def test_scene_rays(name):
    """The whole-list rays of every scene hit and miss, with and without a skip, by the oracle."""
    sc = pc.list_scenes()[name]
    O, D, skip = pc.scene_rays(name)
    assert len(skip) <= pc.MAX_CASES
    idx, t, P, N, z = pc.ref_nearest(sc.js, O, D, skip)
    sh = pc.ref_nearest(sc.js, O, D, skip, shadow=True)[0]
    _report(f"scene {name}", rays=len(skip), hit=int((idx >= 0).sum()), shadowed=int((sh >= 0).sum()),
            zero_events=int(z.sum()))
    assert np.array_equal(idx >= 0, sh >= 0)
    assert (idx >= 0).sum() >= 500 and (idx < 0).sum() >= 500
    assert np.count_nonzero((idx >= 0) & (skip >= 0)) >= 100
    assert len(set(idx[idx >= 0].tolist())) >= min(sc.num_shapes, 3)
    ci, ct = pc.ref_nearest(sc.js, O, D, skip, cuda=True)
    assert (ci >= 0).sum() >= 500
