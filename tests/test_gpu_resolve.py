"""The carry resolver entry by entry against the CPU oracle ("Entry-level tests of the
carry resolver").  Everything is bit for bit: no tolerance, no case left out; one NaN equals another
per component (a generated NaN's sign is the hardware's), -0 is not +0.

Evaluators: tests/tools/resolve_check.hip (make resolvecheck) runs every case of
tests/resolve_cases.py through carry_path, carry_path_coop at every legal group size and
carry_path_spec<GT, kQ> in the windows' lane layout; carry-out and hit flag against rco_prim_shoot.
Chains: the product's wave_window and block_window (rc_resolve.hpp) over whole chains, stepped
as k_resolve steps them; every entry's carry-in and hit flag, the final carry and the changer
count against the oracle call iterated entry by entry.
Frames: the product's k_resolve under every schedule that changes it; rc.debug_carry_ins reads the
frame's DEP list, carry-ins and hit bits back; against rco_render_cls, and the image bytes.
Teeth: four wrong builds of the harness, each caught."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import resolve_cases as rv
from helpers import ROOT, rc
from test_gpu_prims import _ok, _p

pytestmark = pytest.mark.gpu

F32, I32, U64 = np.float32, np.int32, np.uint64
WAVE_K, RESOLVE_K = 2, 1      # rc_tuning's defaults
STOP_SLOTS = 64


class ResolveHarness:
    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        lib.rv_scene_create.restype = ctypes.c_void_p
        lib.rv_scene_create.argtypes = [ctypes.c_void_p]
        lib.rv_scene_destroy.argtypes = [ctypes.c_void_p]
        lib.rv_scene_info.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int)] * 3
        lib.rv_eval.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 5
        lib.rv_chain.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int] + \
            [ctypes.c_void_p] * 11
        lib.rv_tag.restype = ctypes.c_uint
        self.tag = int(lib.rv_tag())
        self.wrong = int(lib.rv_wrong())
        self._scenes = {}

    def scene(self, js):
        key = ctypes.addressof(js)
        if key not in self._scenes:
            h = self.lib.rv_scene_create(ctypes.addressof(js))
            assert h, "rv_scene_create failed"
            self._scenes[key] = h
        return self._scenes[key]

    def eval(self, js, form, G, kq, d, carry, maxrec):
        n = len(d)
        out, hit, cls = np.zeros((n, 3), F32), np.zeros(n, I32), np.zeros(n, I32)
        _ok(self.lib.rv_eval(self.scene(js), form, G, kq, n, maxrec, _p(d), _p(carry), _p(out), _p(hit), _p(cls)),
            f"rv_eval({form}, {G}, {kq})")
        return out, hit, cls

    def chain(self, js, mode, G, K, kq, chains, hists=None):
        """chains: up to 64 with one scene and maxrec.  Returns per chain a dict: cin (the decoded
        granules), hit, tags_ok, mine, mhit (mode -1), fin, stats, stops, cls."""
        assert 1 <= len(chains) <= 64
        offs = np.cumsum([0] + [len(c) for c in chains]).astype(I32)
        n = int(offs[-1])
        d = np.ascontiguousarray(np.concatenate([c.d for c in chains]), F32)
        init = np.ascontiguousarray(np.stack([c.init for c in chains]), F32)
        hn = np.zeros(len(chains), I32)
        hist = np.zeros((len(chains), 12), F32)
        for k, h in enumerate(hists or []):
            if h is not None:
                hn[k] = len(h)
                hist[k, :3 * len(h)] = np.asarray(h, F32).reshape(-1)
        raw = np.zeros((n, 3), U64)
        mine, mhit = np.zeros((n, 3), F32), np.zeros(n, I32)
        fin, stats = np.zeros((len(chains), 3), F32), np.zeros((len(chains), 4), I32)
        stops, cls = np.zeros((len(chains), STOP_SLOTS), I32), np.zeros(n, I32)
        _ok(self.lib.rv_chain(self.scene(js), mode, G, K, kq, len(chains), _p(offs), chains[0].maxrec, _p(d),
                              _p(init), _p(hn), _p(hist), _p(raw), _p(mine), _p(mhit), _p(fin), _p(stats),
                              _p(stops), _p(cls)), f"rv_chain({mode}, {G}, {K})")
        val = (raw & U64(0xffffffff)).astype(np.uint32).view(F32)
        tag = (raw >> U64(32)).astype(np.uint32)
        tags_ok = ((tag & 0x7fffffff) == self.tag).all(1) & (tag == tag[:, :1]).all(1)
        hit = (tag[:, 0] >> 31).astype(bool)
        out = []
        for k in range(len(chains)):
            a, b = offs[k], offs[k + 1]
            out.append(dict(cin=val[a:b], hit=hit[a:b], tags_ok=tags_ok[a:b], mine=mine[a:b], mhit=mhit[a:b] != 0,
                            fin=fin[k], stats=stats[k], stops=stops[k], cls=cls[a:b]))
        return out

    def close(self):
        for h in self._scenes.values():
            self.lib.rv_scene_destroy(h)
        self._scenes = {}


def _lib(name):
    return os.path.join(ROOT, "tests", "build", name)


@pytest.fixture(scope="module")
def built():
    """The harness libraries; built here (no build, no pass)."""
    subprocess.run(["make", "-s", "-j5", "resolvecheck"], cwd=ROOT, check=True, capture_output=True)
    rc.hip_lib()   # first: it settles which HIP runtime the process has (torch's, where torch is)


@pytest.fixture(scope="module")
def hw(built):
    h = ResolveHarness(_lib("libresolvecheck.so"))
    assert h.wrong == 0
    yield h
    h.close()


def _hex(a):
    return " ".join(f"{v:08x}" for v in rv.bits(np.atleast_1d(a)).reshape(-1))


# -------------------------------------------------------------------------- evaluators --
def eval_mismatches(h, cs, form):
    """Cases of the list whose class, carry-out or hit flag is not the oracle's, under one form."""
    name, f, G, kq = form
    want, whit, _ = cs.ref
    out, hit, cls = h.eval(cs.js, f, G, kq, cs.d, cs.carry, cs.maxrec)
    return (cls != 2) | ~rv.same_nan(out, want) | ((hit != 0) != whit), out, hit, cls


@pytest.mark.parametrize("family", list(rv.EVAL_FAMILIES))
def test_evaluators(hw, family):
    """Every form on every case, reported per form; each form's case count against the lists."""
    per_form, first = {}, None
    for cs in rv.EVAL_FAMILIES[family]():
        for form in rv.eval_forms(cs.scene):
            bad, out, hit, cls = eval_mismatches(hw, cs, form)
            n, b = per_form.get(form[0], (0, 0))
            per_form[form[0]] = (n + len(cs), b + int(bad.sum()))
            if bad.any() and first is None:
                i = int(np.flatnonzero(bad)[0])
                first = (f"{cs.label} form {form[0]}: case {i} of {len(cs)}: d {_hex(cs.d[i])} carry-in "
                         f"{_hex(cs.carry[i])} maxrec {cs.maxrec} | device class {cls[i]} carry-out {_hex(out[i])} "
                         f"hit {hit[i]} | oracle carry-out {_hex(cs.ref[0][i])} hit {int(cs.ref[1][i])}")
    for name, (n, b) in per_form.items():
        print(f"[gpu_resolve] {family} {name}: {n} cases, {b} mismatches")
    want = {}
    for cs in rv.EVAL_FAMILIES[family]():
        for form in rv.eval_forms(cs.scene):
            want[form[0]] = want.get(form[0], 0) + len(cs)
    assert {k: v[0] for k, v in per_form.items()} == want
    assert per_form["lane"][0] == sum(len(c) for c in rv.EVAL_FAMILIES[family]())
    assert first is None, first
    assert all(b == 0 for _, b in per_form.values()), per_form


def test_single_group_and_partial_waves(hw):
    """One case alone (a wave with a single active group), 65 (a second wave with one) and 130, in
    every form."""
    cs = [c for c in rv.family_scan() if c.label == "scan/quadric/96x72/m7"][0]
    for n in (1, 65, 130):
        sub = rv.EvalCases(cs.scene, cs.d[:n], cs.carry[:n], cs.maxrec, f"{cs.label}[:{n}]")
        for form in rv.eval_forms(cs.scene):
            bad = eval_mismatches(hw, sub, form)[0]
            assert not bad.any(), (n, form[0], int(bad.sum()))


# ------------------------------------------------------------------------------ chains --
def chain_groups(chains):
    """Batches of at most 64 chains of one scene and maxrec, about 16 k entries each."""
    by = {}
    for c in chains:
        by.setdefault((id(c.scene), c.maxrec), []).append(c)
    for lst in by.values():
        batch, size = [], 0
        for c in lst:
            if batch and (len(batch) == 64 or size + len(c) > 16384):
                yield batch
                batch, size = [], 0
            batch.append(c)
            size += len(c)
        if batch:
            yield batch


def chain_G(scene):
    n = rv.n_shapes(scene)
    return [0] + [g for g in (4, 8, 16, 32, 64) if g >= n and n <= 64]


def default_kq(scene):
    return rv.eval_forms(scene)[0][3]


def check_chain(c, r, wave, what):
    """One chain's device results against the chained oracle; returns a description of the first
    difference or None."""
    cin, hit, chg, fin = c.ref
    bad = (r["cls"] != 2) | ~r["tags_ok"] | ~rv.same_nan(r["cin"], cin) | (r["hit"] != hit)
    if wave:
        bad |= ~rv.same_nan(r["mine"], cin) | (r["mhit"] != hit)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        return (f"{what} {c.label}: entry {i} of {len(c)} (window lane {i % 64} / {i % 256}): class {r['cls'][i]} "
                f"tags {bool(r['tags_ok'][i])} carry-in {_hex(r['cin'][i])} hit {int(r['hit'][i])}"
                + (f" mine {_hex(r['mine'][i])} mhit {int(r['mhit'][i])}" if wave else "")
                + f" | oracle {_hex(cin[i])} hit {int(hit[i])}; {int(bad.sum())} entries differ")
    if not rv.same_nan(r["fin"][None], fin[None])[0]:
        return f"{what} {c.label}: final carry {_hex(r['fin'])} | oracle {_hex(fin)}"
    if int(r["stats"][2]) != int(chg.sum()):
        return f"{what} {c.label}: WinStats.changers {int(r['stats'][2])} | oracle {int(chg.sum())}"
    return None


def run_chains(h, chains, mode, G, K, kq=None, hists=None):
    """(chains run, chains that differ, first difference, evaluation steps, entries)."""
    ran = bad = steps = entries = 0
    first = None
    hmap = {id(c): hh for c, hh in zip(chains, hists)} if hists else None
    for batch in chain_groups(chains):
        s = batch[0].scene
        if G not in chain_G(s):
            continue
        res = h.chain(batch[0].js, mode, G, K, default_kq(s) if kq is None else kq, batch,
                      [hmap[id(c)] for c in batch] if hmap else None)
        for c, r in zip(batch, res):
            msg = check_chain(c, r, mode < 0, f"mode {mode} G {G} K {K}")
            ran += 1
            bad += msg is not None
            first = first or msg
            steps += int(r["stats"][3])
            entries += len(c)
    return ran, bad, first, steps, entries


def family_K(family):
    return (1, 2, 8) if family == "cut" else (None,)


@pytest.mark.parametrize("family", list(rv.CHAIN_FAMILIES))
def test_wave_chains(hw, family):
    """wave_window over G = 0 (LANE passes only), 4, 8, 16, 32, 64 as the scene allows; the cut chains
    at K = 1, 2, 8."""
    chains = rv.CHAIN_FAMILIES[family]()
    failures = []
    for G in (0, 4, 8, 16, 32, 64):
        for K in family_K(family):
            ran, bad, first, steps, entries = run_chains(hw, chains, -1, G, K or WAVE_K)
            print(f"[gpu_resolve] wave {family} G {G} K {K or WAVE_K}: {ran} chains, {entries} entries, {steps} "
                  f"steps, {bad} chains differ")
            if first:
                failures.append(first)
            if G == 0:
                assert ran == len(chains)
            if family == "dense" and G in (4, 8) and ran:
                # the numpy predictor finds matches on these carries (test_resolve_cases.py: 163 with
                # 3 guesses), so two-entry retirements must show
                assert steps < entries, (G, steps, entries)
    if family == "natural":   # the cross-term-free quadric form, where no quadric has cross terms
        q = [c for c in chains if "/quadric256/" in c.label]
        ran, bad, first, _, _ = run_chains(hw, q, -1, 8, WAVE_K, kq=2)
        print(f"[gpu_resolve] wave natural/quadric256 G 8 kQ 2: {ran} chains, {bad} differ")
        if first:
            failures.append(first)
    assert not failures, failures[:3]


def dense_histories(chains):
    """For the helpers' use: each dense chain from its third change in a row on, with the history
    a handing-off wave would bring (the carries after the last three changes, latest first)."""
    out, hists = [], []
    for c in chains:
        cin, _, chg, _ = c.ref
        k = next((k for k in range(2, len(c) - 8) if chg[k - 1] and chg[k - 2]), None)
        if k is None:
            continue
        sub = rv.Chain(c.scene, c.d[k:], cin[k], c.maxrec, c.label + f"[{k}:]")
        out.append(sub)
        hists.append([cin[k], cin[k - 1], cin[k - 2]])
    return out, hists


@pytest.mark.parametrize("family", list(rv.CHAIN_FAMILIES))
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_block_chains(hw, family, mode):
    """block_window in its three uses: 0 plain (whole-workgroup regular segments), 1 with a CarryHist
    (the helpers' predictive step; it starts empty, and on the dense runs also as handed off), 2 with
    stop = true (the team leader)."""
    chains = rv.CHAIN_FAMILIES[family]()
    failures = []
    for G in (0, 4, 8, 16, 32, 64):
        for K in family_K(family):
            k = K or (WAVE_K if mode == 0 else RESOLVE_K)
            ran, bad, first, steps, entries = run_chains(hw, chains, mode, G, k)
            print(f"[gpu_resolve] block mode {mode} {family} G {G} K {k}: {ran} chains, {entries} entries, "
                  f"{steps} steps, {bad} chains differ")
            if first:
                failures.append(first)
            if family == "dense" and mode == 1 and G == 8 and ran:
                assert steps < entries, (steps, entries)   # 179 matches with 15 guesses by numpy
    if family == "dense" and mode == 1:
        sub, hists = dense_histories(chains)
        assert len(sub) >= 10
        for G in (8, 16, 32, 64):
            ran, bad, first, steps, entries = run_chains(hw, sub, 1, G, RESOLVE_K, hists=hists)
            print(f"[gpu_resolve] block mode 1 dense handed-off G {G}: {ran} chains, {entries} entries, {steps} "
                  f"steps, {bad} chains differ")
            if first:
                failures.append(first)
    assert not failures, failures[:3]


def test_leader_stops(hw):
    """With stop = true the leader does hand back inside windows (the harness reports where), and the
    entries after a stop are still resolved to the oracle's carry-ins (test_block_chains checks
    them): here only that the cut chains make it stop at all."""
    stops = 0
    for batch in chain_groups(rv.cut_chains()):
        for r in hw.chain(batch[0].js, 2, 8, RESOLVE_K, default_kq(batch[0].scene), batch):
            stops += int(r["stops"][0])
    print(f"[gpu_resolve] leader stops over the cut chains: {stops}")
    assert stops > 0


# ------------------------------------------------------------------------------ frames --
def check_frame(name, W, H, depth, what):
    img, dep, cin, hit = rv.frame_reference(name, W, H, depth)
    got = rc.render(rv.scenes()[name], W, H, depth=depth, mode="parity")
    assert rc.lone_frames_check()["failed"] == 0, what
    pix, carry, h, first_bad = rc.debug_carry_ins()
    where = f"{what} {name} {W}x{H} d{depth}"
    assert first_bad == -1, (where, "entry with tags that are not the frame's", first_bad)
    assert len(pix) == len(dep) and (pix == dep).all(), (where, len(pix), len(dep))
    bad = ~rv.same_nan(carry, cin) | (h != hit)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        pytest.fail(f"{where}: DEP entry {i} of {len(dep)} (pixel {dep[i] % W}, {dep[i] // W}): carry-in "
                    f"{_hex(carry[i])} hit {h[i]} | oracle {_hex(cin[i])} hit {hit[i]}; {int(bad.sum())} entries differ; "
                    f"{int((got != img).sum())} image bytes differ")
    np.testing.assert_array_equal(got, img, err_msg=where)
    return len(dep)


@pytest.mark.parametrize("sched", list(rv.SCHEDULES))
def test_frames(built, sched):
    """The product's k_resolve, every DEP entry of every frame: the DEP list, the carry-ins and the
    hit bits read back from the frame's workspace, and the image bytes."""
    n = 0
    with rc.tuned(**rv.SCHEDULES[sched]):
        for name, W, H in rv.FRAMES:
            for depth in rv.FRAME_DEPTHS:
                n += check_frame(name, W, H, depth, sched)
        if sched == "default":
            for name, W, H in rv.CHUNK_FRAMES:
                n += check_frame(name, W, H, 6, sched)
    print(f"[gpu_resolve] frames {sched}: {n} entries, 0 mismatches")


@pytest.mark.parametrize("sched", list(rv.TEAM_SCHEDULES))
def test_frames_team_on_short_segments(built, sched):
    """long_len 64 and 256: the team's SCAN / RESOLVE rounds on 54 segments and on one of quadric
    256 x 256 (and on the other frames' segments of that length)."""
    n = 0
    with rc.tuned(**rv.TEAM_SCHEDULES[sched]):
        for name, W, H in rv.FRAMES:
            n += check_frame(name, W, H, 6, sched)
    print(f"[gpu_resolve] frames {sched}: {n} entries, 0 mismatches")


@pytest.mark.parametrize("sched", list(rv.HAND_SCHEDULES))
def test_frames_hand_off(built, sched):
    """hand_run 8 and 32 with 1 and 8 helpers at quadric 512 x 512, and at the many-shape scenes."""
    n = 0
    with rc.tuned(**rv.HAND_SCHEDULES[sched]):
        for name, W, H in [rv.HAND_FRAME] + rv.FRAMES[3:]:
            n += check_frame(name, W, H, 6, sched)
    print(f"[gpu_resolve] frames {sched}: {n} entries, 0 mismatches")


def test_carry_ins_need_a_frame(built):
    """A frame without DEP entries gives empty arrays; a process that has rendered no parity frame
    gets the entry's refusal (a fresh process: this one's workspace holds the frames above)."""
    rc.render(rv.scenes()["mirror-box"], 96, 72, depth=6, mode="parity")
    pix, carry, hit, bad = rc.debug_carry_ins()
    assert len(pix) == 0 and bad == -1
    code = ("import sys; sys.path.insert(0, %r); from helpers import rc\n"
            "try:\n    rc.debug_carry_ins()\nexcept RuntimeError as e:\n    print('refused:', e)\n"
            % os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "refused: rc_debug_carry_ins: -1" in out.stdout, (out.stdout, out.stderr)


# ------------------------------------------------------------------------------- teeth --
def _wrong(k):
    h = ResolveHarness(_lib(f"libresolvecheck_w{k}.so"))
    assert h.wrong == k
    return h


def test_teeth_equal_instead_of_same_bits(built):
    """Wrong build 1: the windows compare carries with ==.  A NaN carry is then never `unchanged`
    (every clean entry counts as a changer) and -0 equals +0."""
    h = _wrong(1)
    bad = ran = 0
    for mode, G in ((-1, 0), (-1, 8), (0, 8), (1, 8), (2, 8)):
        r, b, first, _, _ = run_chains(h, rv.zero_chains(), mode, G, WAVE_K)
        ran, bad = ran + r, bad + b
    h.close()
    print(f"[gpu_resolve] teeth 1 (== for same_bits): {bad} of {ran} chain runs caught")
    assert bad > 0


def _eval_teeth(h, families, forms_like):
    bad = ran = 0
    for fam in families:
        for cs in rv.EVAL_FAMILIES[fam]():
            for form in rv.eval_forms(cs.scene):
                if form[0].startswith(forms_like):
                    bad += int(eval_mismatches(h, cs, form)[0].sum())
                    ran += len(cs)
    return bad, ran


def test_teeth_argmin_without_tie_break(built):
    """Wrong build 2: among equal t the speculative evaluator's arg-min lets the highest index win."""
    h = _wrong(2)
    bad, ran = _eval_teeth(h, ["tie"], "spec")
    h.close()
    print(f"[gpu_resolve] teeth 2 (arg-min tie-break): {bad} of {ran} cases caught")
    assert bad > 0


def test_teeth_skip_kept_after_a_miss(built):
    """Wrong build 3: S keeps the last hit shape after a missed level."""
    h = _wrong(3)
    bad, ran = _eval_teeth(h, ["scan", "creep", "pattern", "skip"], "spec")
    h.close()
    print(f"[gpu_resolve] teeth 3 (S after a miss): {bad} of {ran} cases caught")
    assert bad > 0


def test_teeth_guess_one_ulp_off(built):
    """Wrong build 4: the predictive step accepts a guess one float step from the exact carry."""
    h = _wrong(4)
    bad = ran = 0
    sub, hists = dense_histories(rv.dense_chains())
    for chains, hh, mode, G in ((rv.dense_chains(), None, -1, 4), (rv.dense_chains(), None, -1, 8),
                                (rv.dense_chains(), None, 1, 8), (sub, hists, 1, 8), (rv.natural_chains(), None, -1, 8)):
        r, b, first, _, _ = run_chains(h, chains, mode, G, WAVE_K if mode < 0 else RESOLVE_K, hists=hh)
        ran, bad = ran + r, bad + b
    h.close()
    print(f"[gpu_resolve] teeth 4 (guess one ulp off): {bad} of {ran} chain runs caught")
    assert bad > 0
