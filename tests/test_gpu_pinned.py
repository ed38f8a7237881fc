"""Phase C's carry-point table (rc_device.hpp pin_build / shade_dep_cont_pin / shade_dep_wave,
rc_tuning.pin): a wave of k_dep_chunks whose carry-ins all have the same bits
computes what depends on the carry point alone once.  Every result must keep every bit.

Wave level: tests/tools/pin_check.hip (make pincheck) runs one wave per 64 entries through the
product's shade_dep_wave; colour (every bit of the three floats before quantisation, one NaN equal
to another) and zero-normalize events per entry against the CPU oracle's o_shoot, and the number of
waves that took the table against what the carry-ins dictate.  The table covers phase C only (the
resolver's LANE windows do not use it), so there is no carry-out or hit flag to compare here.

Image level: whole frames under rc_tuning.pin 0..3, lone (phase C after the resolver, side=0, which
is k_dep_chunks; and the default side=3, which shades inside the resolver and has no table) and two
frames in flight, against the golden md5s where one exists and the CPU oracle elsewhere, with the
zero-normalize event counts."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import prim_cases as pc
import shade_cases as sc
from helpers import ROOT, golden_key, golden_table, oracle_render, p3_md5, rc, scene_path
from pinned_cases import IMAGES, LIGHT_ROWS, SHAPE_ROWS, big_scene, lit_phantom_scene, text_scene
from test_gpu_prims import _ok, _p, same_bits32

pytestmark = pytest.mark.gpu

F32, I32 = np.float32, np.int32
MAXREC = 7   # depth 6


class PinHarness:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.pn_scene_create.restype = ctypes.c_void_p
        self.lib.pn_scene_create.argtypes = [ctypes.c_void_p]
        self.lib.pn_scene_destroy.argtypes = [ctypes.c_void_p]
        self.lib.pn_scene_info.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int)] * 4
        self.lib.pn_dep_wave.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 6
        self._scenes = {}

    def scene(self, js):
        key = ctypes.addressof(js)
        if key not in self._scenes:
            h = self.lib.pn_scene_create(ctypes.addressof(js))
            assert h, "pn_scene_create failed"
            self._scenes[key] = h
        return self._scenes[key]

    def info(self, js):
        v = [ctypes.c_int() for _ in range(4)]
        self.lib.pn_scene_info(self.scene(js), *v)
        return dict(zip(("n", "m", "dep_fast", "fits"), (x.value for x in v)))

    def dep_wave(self, js, pin, d, carry, maxrec=MAXREC):
        d, carry = np.ascontiguousarray(d, F32), np.ascontiguousarray(carry, F32)
        n = len(d)
        rgb, zero, flag = np.zeros((n, 3), F32), np.zeros(n, I32), np.zeros(n, I32)
        waves = np.zeros(2, I32)
        _ok(self.lib.pn_dep_wave(self.scene(js), pin, n, maxrec, _p(d), _p(carry), _p(rgb), _p(zero),
                                 _p(flag), _p(waves)), "pn_dep_wave")
        return rgb, zero, flag, (int(waves[0]), int(waves[1]))

    def close(self):
        for h in self._scenes.values():
            self.lib.pn_scene_destroy(h)
        self._scenes = {}


@pytest.fixture(scope="module")
def hw():
    """The harness library; built here (no build, no pass)."""
    subprocess.run(["make", "-s", "pincheck"], cwd=ROOT, check=True, capture_output=True)
    rc.hip_lib()   # first: it settles which HIP runtime the process has (torch's, where torch is)
    h = PinHarness(os.path.join(ROOT, "tests", "build", "libpincheck.so"))
    yield h
    h.close()


def _hex32(a):
    return " ".join(f"{v:08x}" for v in pc.bits32(np.atleast_1d(a)))


class Base:
    """The quadric example's 64 x 48 camera: the first-bounce-miss (DEP) rays and the carry-ins
    the oracle's own scan gives them, most frequent first (`carries`); `pinning`: those
    from which at least a quarter of the first 64 rays hit and land on the carry point
    again, bit for bit (by the oracle's carry-out) — the hits that read the table."""

    def __init__(self, scene):
        self.scene, self.js = scene, scene.js
        d = sc.camera_dirs(self.js)
        _, cls, _, _, _ = sc.ref_shoot(self.js, d, MAXREC, "parity", np.zeros_like(d))
        _, _, cin = oracle_render(scene, 64, 48, MAXREC - 1, "parity", with_carry=True)
        dep = cls >= 2
        self.d, cin = d[dep], cin.reshape(-1, 3)[dep]
        rows, counts = np.unique(cin.view(np.uint32), axis=0, return_counts=True)
        self.carries = rows[np.argsort(-counts)].view(F32)
        assert len(self.d) >= 128 and len(self.carries) >= 3
        self.pinning = []
        for c in self.carries:
            tiled = np.tile(c, (64, 1))
            _, cl, cout, _, _ = sc.ref_shoot(self.js, self.d[:64], MAXREC, "parity", tiled)
            back = ((cl & 1) != 0) & same_bits32(cout, tiled).all(1)
            if back.sum() >= 16:
                self.pinning.append(c)
        assert len(self.pinning) >= 2, len(self.pinning)


@pytest.fixture(scope="module")
def base():
    return Base(rc.Scene.from_file(scene_path("quadric")))


def run_case(hw, js, d, carry, pin, want_took, label):
    """One harness call against o_shoot: every DEP entry's colour and events; the waves' ways."""
    d, carry = np.ascontiguousarray(d, F32), np.ascontiguousarray(carry, F32)
    w_rgb, w_cls, _, w_zero, _ = sc.ref_shoot(js, d, MAXREC, "parity", carry)
    rgb, zero, flag, waves = hw.dep_wave(js, pin, d, carry)
    info = hw.info(js)
    dep = (w_cls >= 2) & bool(info["dep_fast"])
    bad = (flag != 0) != dep
    bad |= dep & (~same_bits32(rgb, w_rgb).all(1) | (zero != w_zero))
    print(f"[gpu_pinned] {label} pin {pin}: {len(d)} entries, {int(dep.sum())} DEP, waves table/plain "
          f"{waves}, {int(bad.sum())} mismatches")
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        pytest.fail(f"{label} pin {pin}: entry {i} of {len(d)}: d {_hex32(d[i])} carry {_hex32(carry[i])} | "
                    f"device rgb {_hex32(rgb[i])} zero {zero[i]} flag {flag[i]} | reference rgb "
                    f"{_hex32(w_rgb[i])} zero {w_zero[i]} cls {w_cls[i]}")
    if want_took is not None:
        assert waves == want_took, (label, pin, waves, want_took)
    return int(dep.sum()), w_zero


def both(hw, js, d, carry, took, label):
    """The case with the table (the waves must go the way `took` says) and with pin = 0 (none may)."""
    n_dep, w_zero = run_case(hw, js, d, carry, 1, took, label)
    run_case(hw, js, d, carry, 0, (0, sum(took)), label)
    return n_dep, w_zero


def test_uniform_and_mixed_waves(hw, base):
    """All lanes on one carry (the three most frequent real carry-ins, and each entry's own);
    lane 0 differing from the rest; two carries alternating; partial waves of 1, 37 and 63."""
    d, cs = base.d[:64], base.carries
    for k in range(3):
        n, _ = both(hw, base.js, d, np.tile(cs[k], (64, 1)), (1, 0), f"uniform/{k}")
        assert n == 64
    for k, c in enumerate(base.pinning[:3]):
        both(hw, base.js, d, np.tile(c, (64, 1)), (1, 0), f"uniform/pinning {k}")
    cs = np.concatenate([base.pinning[:1], cs])   # the mixed waves below: a pinning carry and others
    c = np.tile(cs[0], (64, 1))
    c[0] = cs[1]
    both(hw, base.js, d, c, (0, 1), "lane 0 differs")
    c[0], c[63] = cs[0], cs[2]
    both(hw, base.js, d, c, (0, 1), "lane 63 differs")
    c = np.tile(cs[0], (64, 1))
    c[1::2] = cs[1]
    both(hw, base.js, d, c, (0, 1), "alternating")
    for n in (1, 37, 63):
        both(hw, base.js, base.d[64:64 + n], np.tile(cs[0], (n, 1)), (1, 0), f"partial/{n}")
    # two waves in one call: a uniform one and a mixed one
    c = np.tile(cs[1], (128, 1))
    c[100] = cs[0]
    both(hw, base.js, base.d[:128], c, (1, 1), "two waves")


def test_equal_numbers_different_bits(hw, base):
    """-0 against +0 in one component, two NaN payloads, and inf: `same point` is the bits."""
    d = base.d[:64]
    pos = base.pinning[0].copy()
    pos[1] = 0.0
    neg = pos.copy()
    neg[1] = -0.0
    assert (pos == neg).all() and not same_bits32(pos, neg).all()
    both(hw, base.js, d, np.tile(pos, (64, 1)), (1, 0), "+0 uniform")
    both(hw, base.js, d, np.tile(neg, (64, 1)), (1, 0), "-0 uniform")
    c = np.tile(pos, (64, 1))
    c[5] = neg
    both(hw, base.js, d, c, (0, 1), "-0 in lane 5")
    c[0], c[5] = neg, pos
    both(hw, base.js, d, c, (0, 1), "-0 in lane 0")
    nan_a = np.array([0x7fc00000, 0x3f800000, 0xc0a00000], np.uint32).view(F32)
    nan_b = np.array([0x7fc00001, 0x3f800000, 0xc0a00000], np.uint32).view(F32)
    both(hw, base.js, d, np.tile(nan_a, (64, 1)), (1, 0), "NaN uniform")
    c = np.tile(nan_a, (64, 1))
    c[9] = nan_b
    both(hw, base.js, d, c, (0, 1), "two NaN payloads")
    for v in (np.inf, -np.inf):
        inf = base.pinning[0].copy()
        inf[2] = v
        both(hw, base.js, d, np.tile(inf, (64, 1)), (1, 0), f"inf uniform {v}")
    both(hw, base.js, d, np.full((64, 3), np.inf, F32), (1, 0), "all inf")


def test_carry_on_a_light(hw, base):
    """The quadric example with a point light and a spot light put exactly on two pinning
    carry-ins: hits that land on the carry point then have dist == 0 (one counted event for the
    point light, two for the spot light when it is not shadowed)."""
    a, b = base.pinning[0], base.pinning[1]
    s = text_scene("on_light", LIGHT_ROWS(a, b))
    info = hw.info(s.js)
    assert info["dep_fast"] and info["fits"], info
    d = base.d[:64]
    assert not same_bits32(base.carries[0], a).all() and not same_bits32(base.carries[0], b).all()
    _, plain = both(hw, s.js, d, np.tile(base.carries[0], (64, 1)), (1, 0), "on light/elsewhere")
    fired = 0
    for name, c in (("point", a), ("spot", b)):
        _, w_zero = both(hw, s.js, d, np.tile(c, (64, 1)), (1, 0), f"on light/{name}")
        fired += int((w_zero > plain).sum())
    print(f"[gpu_pinned] entries with dist == 0 events: {fired}")
    assert fired > 0, "no entry of the case has a hit on the light"


def test_zero_normals(hw, base):
    """Carries where a shape's normal is the zero vector (a sphere's centre; the point where a
    quadric's gradient vanishes): the table's row is built through normalize's zero-length branch
    (and holds its event for any hit that lands there); the entries' results stand."""
    s = text_scene("zero_normal", SHAPE_ROWS)
    info = hw.info(s.js)
    assert info["dep_fast"] and info["fits"], info
    d = sc.camera_dirs(s.js)
    _, cls, _, _, _ = sc.ref_shoot(s.js, d, MAXREC, "parity", np.zeros_like(d))
    d = d[cls >= 2][:64]
    assert len(d) == 64
    for name, c in (("sphere centre", (0.0, 0.0, -5.0)), ("quadric centre", (2.0, 0.5, -6.0))):
        both(hw, s.js, d, np.tile(np.array(c, F32), (64, 1)), (1, 0), f"zero normal/{name}")


def test_scenes_beyond_the_table(hw):
    """n * m > 64 with n and m inside the table's rows, and n above its shape rows: no wave may
    take the table (the harness counts them), and the per-lane code's results stand."""
    for label, (n, m) in (("pairs", (8, 9)), ("shapes", (9, 2))):
        s = big_scene(label, n, m)
        info = hw.info(s.js)
        assert (info["n"], info["m"], info["fits"]) == (n, m, 0), info
        assert info["dep_fast"], info
        d = sc.camera_dirs(s.js)
        _, cls, _, _, _ = sc.ref_shoot(s.js, d, MAXREC, "parity", np.zeros_like(d))
        d = d[cls >= 2][:64]
        assert len(d) >= 16, (label, len(d))
        n_dep, _ = run_case(hw, s.js, d, np.tile(np.array((0.5, -1.0, -4.0), F32), (len(d), 1)), 1, (0, 1),
                            f"beyond/{label}")
        assert n_dep == len(d)


# ------------------------------------------------------------------------ image level --
@pytest.fixture(scope="module")
def table():
    return golden_table()


@pytest.fixture(scope="module")
def references(table):
    """(scene, reference image or None where the golden md5 serves, oracle's zero-normalize count)."""
    out = {}
    for name, w, h in IMAGES:
        s = rc.Scene.from_file(scene_path(name))
        img, st = oracle_render(s, w, h, 6, "parity")
        out[(name, w, h)] = (s, img, st["zero_normalize"])
    return out


def _check_image(got, tim, ref, table, key, what):
    s, img, zero = ref
    np.testing.assert_array_equal(got, img, err_msg=f"{what} {key}")
    gk = golden_key(key[0], key[1], key[2], 6, "parity")
    if gk in table:
        assert p3_md5(got) == table[gk]["md5"], (what, gk)
    if tim is not None:
        assert tim["zero_normalize"] == zero, (what, key, tim["zero_normalize"], zero)


@pytest.mark.parametrize("pin", [0, 1, 2, 3])
def test_images_lone(pin, references, table):
    """Lone frames: side = 0 (k_dep_chunks shades every DEP entry) and side = 3 (the resolver does)."""
    for side in (0, 3):
        with rc.tuned(pin=pin, side=side):
            for key, ref in references.items():
                tim = {}
                got = rc.render(ref[0], key[1], key[2], depth=6, mode="parity", timing=tim)
                _check_image(got, tim, ref, table, key, f"pin {pin} side {side}")


@pytest.mark.parametrize("pin", [0, 1, 2, 3])
def test_images_in_flight(pin, references, table):
    """Two frames in flight (k_dep_chunks on the pixel partition), every image twice in a row."""
    torch = pytest.importorskip("torch")
    with rc.tuned(pin=pin):
        jobs = [(key, ref, torch.zeros((key[2], key[1], 3), dtype=torch.uint8, device="cuda"))
                for key, ref in references.items() for _ in range(2)]
        torch.cuda.synchronize()
        for key, ref, buf in jobs:
            rc.frame_submit(ref[0], key[1], key[2], buf.data_ptr(), depth=6, mode="parity")
        tim = {}
        rc.frames_wait(tim)
        assert tim["frames_failed"] == 0, tim
        for key, ref, buf in jobs:
            _check_image(buf.cpu().numpy(), None, ref, table, key, f"in flight pin {pin}")


def test_not_dep_fast_scene():
    """A scene that is not dep_fast (a lit phantom), and the quadric example with rc_tuning.dep_fast
    = 0, keep the whole-pixel phase C whatever rc_tuning.pin says."""
    for s, extra in ((lit_phantom_scene(), {}), (rc.Scene.from_file(scene_path("quadric")), dict(dep_fast=0))):
        want, st = oracle_render(s, 256, 256, 6, "parity")
        for pin in (0, 3):
            for side in (0, 3):
                with rc.tuned(pin=pin, side=side, **extra):
                    tim = {}
                    got = rc.render(s, 256, 256, depth=6, mode="parity", timing=tim)
                    np.testing.assert_array_equal(got, want)
                    assert tim["zero_normalize"] == st["zero_normalize"]


def test_tuning_field():
    assert rc.get_tuning(default=True)["pin"] == 1
    for bad in (-1, 4):
        with pytest.raises(ValueError):
            rc.set_tuning(pin=bad)
    assert ctypes.sizeof(rc.RcTuning) == 4 * (len(rc.TUNING_FIELDS) + len(rc.TUNING_TAIL))
