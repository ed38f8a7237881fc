"""The cases of tests/test_gpu_resolve.py are what they claim to be (no GPU): every edge the lists
are there for is counted here with the CPU oracle and numpy alone, so a generator that drifts off
an edge fails on the CPU, not silently on the GPU ("Entry-level tests of the carry
resolver").  The counts are the oracle's; they are pinned so that a change of the lists shows."""
import numpy as np
import pytest

import resolve_cases as rv


def _total(cases):
    return sum(len(c) for c in cases)


@pytest.mark.parametrize("name", list(rv.EVAL_FAMILIES))
def test_family_sizes_and_classes(name):
    """At most 2^16 cases a family, every case a DEP entry by the oracle (class >= 2), and both
    kinds of entry present: carry moved, carry kept."""
    cases = rv.EVAL_FAMILIES[name]()
    n = _total(cases)
    assert 0 < n <= rv.MAX_CASES, (name, n)
    moved = kept = hit = 0
    for c in cases:
        cout, h, cls = c.ref
        assert (cls >= 2).all(), (c.label, int((cls < 2).sum()))
        m = ~rv.same_rows(cout, c.carry)
        assert not (m & ~h).any(), (c.label, "a carry moved without a hit")
        moved, kept, hit = moved + int(m.sum()), kept + int((~m).sum()), hit + int(h.sum())
    print(f"[resolve_cases] {name}: {len(cases)} lists, {n} cases, {moved} move the carry, {kept} keep it, "
          f"{hit} hit some level")
    assert (n, moved, hit) == WANT_FAMILY[name], (name, n, moved, hit)
    assert moved > 0 and kept > 0


# cases, cases whose carry-out differs from the carry-in, cases with a hit at some level
WANT_FAMILY = {"scan": (58573, 23938, 29971), "creep": (41550, 37823, 39947), "pattern": (14357, 9921, 14357),
               "tie": (25616, 6658, 11728), "skip": (26326, 25108, 25622), "nonfinite": (15300, 3665, 3699)}


def test_scan_covers_scenes_and_depths():
    """Every scene at every maxrec at both cameras (where the frame has a DEP pixel at all), group
    sizes from 4 lanes to none (65 shapes), maxrec 2 without a level: nothing can hit there."""
    cases = rv.family_scan()
    seen = {tuple(c.label.split("/")[1:]) for c in cases}
    for name in rv.SCAN_SCENES:
        for w, h in rv.CAMERAS:
            for mr in rv.MAXRECS:
                if len(rv.scan_pixels(name, w, h, mr)[0]):
                    assert (name, f"{w}x{h}", f"m{mr}") in seen
    sizes = sorted({rv.n_shapes(c.scene) for c in cases})
    assert min(sizes) <= 4 and {14, 20, 33, 64, 65} <= set(sizes), sizes
    for c in cases:
        if c.maxrec == 2:
            assert not c.ref[1].any() and rv.same_rows(c.ref[0], c.carry).all(), c.label
    # odd and even level counts with a hit at the last level of each
    for mr in (3, 4, 7, 8):
        last = 0
        for c in cases:
            if c.maxrec == mr:
                win, _, _ = rv.levels(c.js, c.d, c.carry, mr)
                last += int((win[:, -1] >= 0).sum())
        print(f"[resolve_cases] scan: maxrec {mr}: {last} entries hit at the last level")
        assert last > 0, mr


def test_levels_restatement_is_the_oracles():
    """levels() (numpy around rco_prim_nearest) gives rco_prim_shoot's carry-out bit for bit and its
    hit flag, on every case of scan, creep, skip and tie: the patterns are selected by a record
    that is the oracle's."""
    bad = total = hits = 0
    for fam in (rv.family_scan, rv.family_creep, rv.family_skip, rv.family_tie, rv.family_nonfinite):
        for c in fam():
            if c.maxrec < 3:
                continue
            win, cout, _ = rv.levels(c.js, c.d, c.carry, c.maxrec)
            want, h, _ = c.ref
            bad += int((~rv.same_nan(cout, want)).sum()) + int(((win >= 0).any(1) != h).sum())
            total += len(c)
            hits += int((win >= 0).sum())
    print(f"[resolve_cases] levels(): {total} cases, {hits} level hits, {bad} differences")
    assert bad == 0 and total > 100000


def test_creep_lands_and_moves():
    """Fed-back carry-outs: thousands land on the same bits again, thousands move on."""
    same = moved = 0
    for c in rv.family_creep():
        cout, h, _ = c.ref
        m = rv.same_rows(cout, c.carry)
        same += int((m & h).sum())
        moved += int((~m).sum())
    print(f"[resolve_cases] creep: {same} hit and land on the same bits, {moved} change the carry")
    assert (same, moved) == (2124, 37823)
    assert same >= 1000 and moved >= 1000


def test_patterns():
    """hit / miss / hit / miss and miss / miss / hit at levels 2.., by the oracle's levels."""
    got = {}
    for pname, pat in rv.PATTERNS.items():
        n = 0
        for c in rv.family_pattern():
            if f"/{pname}/" in c.label:
                win, _, _ = rv.levels(c.js, c.d, c.carry, c.maxrec)
                assert rv.pattern_mask(win, pat).all(), c.label
                n += len(c)
        got[pname] = n
    print(f"[resolve_cases] pattern: {got}")
    assert got == {"hit-miss-hit-miss": 14259, "miss-miss-hit": 98}


def test_ties():
    """Per pair position: levels at which both copies are hit at the same t bit for bit and the
    lower one wins; the winner is the reflective copy in some scenes and the matte one in others
    (the loop goes on / ends there)."""
    per_pair = {p: 0 for p in rv.TIE_PAIRS}
    ends = goes_on = 0
    for c in rv.family_tie():
        k = rv.tie_levels(c)
        p = int(c.label.split("/")[1].split("-")[0][3:])
        per_pair[p] += int(k.sum())
        refl = rv.reflectivity(c.js)
        if k.any():
            ends += int(not refl[p] > 0)
            goes_on += int(refl[p] > 0)
    print(f"[resolve_cases] tie: tied levels per pair {per_pair}; lists whose winner is matte {ends}, "
          f"reflective {goes_on}")
    assert all(v >= 100 for v in per_pair.values()), per_pair
    assert ends > 0 and goes_on > 0


def test_skip_carries_sit_on_shapes():
    """The skip family's carry-ins are hit points of the scene's shapes: its first level starts on
    a surface, on the entry's own primary shape in the first block of every list."""
    n_own = n = 0
    for c in rv.family_skip():
        d = c.d
        i0, _, P0, _, _ = rv.pc.ref_nearest(c.js, np.zeros_like(d), d, np.full(len(d), -1, np.int32))
        own = rv.same_rows(P0, c.carry)
        n_own += int(own.sum())
        n += len(c)
    print(f"[resolve_cases] skip: {n} cases, {n_own} on the entry's own primary hit point")
    assert n_own >= 1000 and n - n_own >= 1000


def test_nonfinite_values_present():
    c = np.concatenate([x.carry for x in rv.family_nonfinite()])
    assert np.isposinf(c).any() and np.isneginf(c).any() and np.isnan(c).any()
    assert ((c == 0) & np.signbit(c)).any() and (np.abs(c) == np.float32(3e38)).any()


def test_forms_per_scene():
    """The evaluator forms a scene takes: 3 shapes -> every group size; 33 -> 64 alone, no
    speculation (2 G > 64); 65 -> the lane form only; kQ = 2 only without cross terms."""
    s = rv.scenes()
    names = lambda k: [f[0] for f in rv.eval_forms(s[k])]
    assert names("quadric") == ["lane", "coop8", "spec8q1", "spec8q2", "coop16", "spec16q1", "spec16q2", "coop32",
                                "spec32q1", "spec32q2", "coop64"]
    assert names("simple")[:3] == ["lane", "coop4", "spec4q0"]
    assert names("full-reflect-sphere")[:2] == ["lane", "coop2"]
    assert names("random33") == ["lane", "coop64"] and names("random65") == ["lane"]
    assert "spec16q2" not in names("random14x") and "spec16q1" in names("random14x")


# ------------------------------------------------------------------------------ chains --
def test_natural_chains():
    """quadric 256 x 256, depth 6: 11 057 DEP entries in 132 segments, 54 of at least 64 entries, the
    longest 3 422; 1 379 changers inside segments (1 399 with the segments' last entries); the
    longest run of changers 89, 13 runs of at least 16.  The degenerate one-segment frames."""
    q = [c for c in rv.natural_chains() if "/quadric256/" in c.label]
    lens = [len(c) for c in q]
    chg = [c.ref[2] for c in q]
    runs = []
    for x in chg:                       # runs inside segments (a segment's last entry hands its carry to nobody)
        idx = np.flatnonzero(x[:-1])
        if len(idx):
            runs += [len(r) for r in np.split(idx, np.flatnonzero(np.diff(idx) > 1) + 1)]
    got = (sum(lens), len(q), sum(int(x.sum()) for x in chg), sum(int(x[:-1].sum()) for x in chg), max(lens),
           sum(n >= 64 for n in lens), max(runs), sum(r >= 16 for r in runs))
    print(f"[resolve_cases] natural/quadric256: {got}")
    assert got == (11057, 132, 1399, 1379, 3422, 54, 89, 13)
    for name, n in (("full-reflect-sphere", 684), ("lone-mirror-plane", 6912)):
        one = [c for c in rv.natural_chains() if f"/{name}/" in c.label]
        assert len(one) == 1 and len(one[0]) == n, (name, [len(c) for c in one])
    for name, _, _ in rv.RANDOM:
        assert any(f"/{name}/" in c.label for c in rv.natural_chains()), name
    total = sum(_total(f()) for f in rv.CHAIN_FAMILIES.values())
    print(f"[resolve_cases] chained entries in all: {total}")
    assert total <= 120000


def test_chain_reference_is_the_scan():
    """The chained rco_prim_shoot gives rco_render_cls's carry-ins (the frame's own scan) on every
    natural chain: every entry's carry-in and hit bit."""
    for name, W, H in (("quadric", 256, 256), ("random33", 96, 72), ("full-reflect-sphere", 96, 72)):
        _, dep, cin, hit = rv.frame_reference(name, W, H, 6)
        tag = "quadric256" if name == "quadric" else name
        chains = [c for c in rv.natural_chains() if f"/{tag}/" in c.label]
        got_c = np.concatenate([c.ref[0] for c in chains])
        got_h = np.concatenate([c.ref[1] for c in chains])
        assert len(got_c) == len(dep)
        assert rv.same_rows(got_c, cin).all() and (got_h == (hit != 0)).all(), name


def test_cut_chains():
    """Every length, and the windows' edges as counts over the wave's 64-entry and the workgroup's
    256-entry windows."""
    cuts = rv.cut_chains()
    assert sorted({len(c) for c in cuts}) == sorted(rv.CUT_LENGTHS)
    c64, c256 = rv.window_census(cuts, 64), rv.window_census(cuts, 256)
    print(f"[resolve_cases] cut: {len(cuts)} chains, {_total(cuts)} entries; 64: {c64}; 256: {c256}")
    for k, v in c64.items():
        assert v > 0, ("64", k)
    for k, v in c256.items():
        assert v > 0, ("256", k)
    assert c64 == WANT_CUT64 and c256 == WANT_CUT256


WANT_CUT64 = {'windows': 683, 'changer_lane0': 350, 'changer_last_lane': 68, 'changer_last_valid_short': 132,
              'changer_after_boundary': 44, 'no_changer': 235, 'all_changers': 10, 'one_clean_between': 79}
WANT_CUT256 = {'windows': 422, 'changer_lane0': 308, 'changer_last_lane': 4, 'changer_last_valid_short': 151,
               'changer_after_boundary': 2, 'no_changer': 53, 'all_changers': 4, 'one_clean_between': 79}


def test_dense_chains_feed_the_predictor():
    """On the oracle's carries: steps where one of the wave's 3 (the workgroup's 15) guesses is the
    exact next carry, steps where none is, and matches followed at once by a clean entry."""
    got = {}
    for ng in (3, 15):
        m = np.sum([rv.predictor_census(c, ng) for c in rv.dense_chains()], axis=0)
        got[ng] = tuple(int(v) for v in m)
    print(f"[resolve_cases] dense: {len(rv.dense_chains())} chains, {_total(rv.dense_chains())} entries; "
          f"(match, miss, match then clean) {got}")
    assert got == {3: (163, 274, 2), 15: (179, 244, 3)}
    for ng in (3, 15):
        assert got[ng][0] >= 100 and got[ng][1] >= 100 and got[ng][2] >= 1


def test_hist_guess_restatement():
    """hist_guess on known histories: one step back, the rounded mean of two and three, the offsets
    0, -1, +1, -2 on the component that moves most, and unsigned wrap-around."""
    b = lambda *v: np.array(v, np.uint32)
    c = b(1000, 2000, 3000)
    assert (rv.hist_guess([b(110, 5, 5), b(100, 5, 5)], c, 1) == b(1010, 2000, 3000)).all()
    assert (rv.hist_guess([b(110, 5, 5), b(100, 5, 5)], c, 2) == b(1009, 2000, 3000)).all()
    assert (rv.hist_guess([b(110, 5, 5), b(100, 5, 5)], c, 3) == b(1011, 2000, 3000)).all()
    assert (rv.hist_guess([b(110, 5, 5), b(105, 5, 5), b(101, 5, 5)], c, 1) == b(1005, 2000, 3000)).all()   # (9 + 1) / 2
    assert (rv.hist_guess([b(5, 90, 5), b(5, 95, 5), b(5, 99, 5), b(5, 100, 5)], c, 4) ==
            b(1000, 2000 - 3 - 2, 3000)).all()                                                            # (-10 - 1) / 3
    assert (rv.hist_guess([b(2, 5, 5), b(0xffffffff, 5, 5)], b(0xfffffffe, 0, 0), 1) == b(1, 0, 0)).all()


def test_zero_chains():
    """+0, -0 and NaN initial components; every entry clean by the oracle; every carry-in the
    initial bits."""
    zc = rv.zero_chains()
    tags = {c.label.split("/")[3][:3].rstrip("(") for c in zc}
    assert tags == {"+0", "-0", "nan"}, tags
    for c in zc:
        cin, _, chg, fin = c.ref
        assert not chg.any() and (rv.bits(cin) == rv.bits(c.init)).all() and (rv.bits(fin) == rv.bits(c.init)).all()
        assert len(c) >= 65
    print(f"[resolve_cases] zeros: {len(zc)} chains, {_total(zc)} entries")
    assert len(zc) == 37


def test_frame_references():
    """The frames of the frame-level test have DEP entries of both kinds (mirror-box has none at
    96 x 72 beyond the class test: its frame is the byte comparison's)."""
    for name, W, H in rv.FRAMES + [rv.HAND_FRAME]:
        _, dep, cin, hit = rv.frame_reference(name, W, H, 6)
        print(f"[resolve_cases] frame {name} {W}x{H}: {len(dep)} DEP entries, {int(hit.sum())} hit")
        if name != "mirror-box":
            assert len(dep) > 0, name
    # long_len 64 / 256 at quadric 256 x 256: 54 segments / 1 go to the team (k_resolve: >= long_len)
    lens = [len(c) for c in rv.natural_chains() if "/quadric256/" in c.label]
    assert (sum(n >= 64 for n in lens), sum(n >= 256 for n in lens)) == (54, 1)
