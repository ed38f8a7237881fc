"""GPU parity tests: libraycast_hip.so (HIP path, called through its C-ABI) against the golden
md5s of the reference's own output and against the CPU oracle.  Bit-exact: every byte of
the PPM must match."""
import os
import subprocess

import numpy as np
import pytest

from helpers import (GOLDEN, ROOT, cross_nan_scene_text, file_md5, golden_key, golden_table,
                     oracle_lib, oracle_render, p3_md5, random_scene, rc, scene_path)

pytestmark = pytest.mark.gpu

SMALL = ["simple", "reflection", "quadric", "example2", "example3", "quadric2"]


@pytest.fixture(scope="module")
def table():
    return golden_table()


@pytest.fixture(scope="module")
def scenes():
    return {n: rc.Scene.from_file(scene_path(n)) for n in SMALL}


@pytest.mark.parametrize("scene", SMALL)
@pytest.mark.parametrize("mode", ["parity", "fast"])
def test_small_goldens(scene, mode, scenes, table):
    small = np.load(os.path.join(GOLDEN, "small.npz"))
    for n in (64, 256):
        for d in (0, 4, 6):
            img = rc.render(scenes[scene], n, n, depth=d, mode=mode)
            key = golden_key(scene, n, n, d, mode)
            if n == 64:
                np.testing.assert_array_equal(img, small[key], err_msg=key)
            assert p3_md5(img) == table[key]["md5"], key


@pytest.mark.parametrize("key", [
    "simple:256x256:d6:parity",             # C1
    "simple:1024x1024:d0:parity",           # C2
    "reflection:2048x2048:d4:parity",       # C3
    "reflection:2048x2048:d4:fast",
    "quadric:4096x4096:d6:parity",          # C4
    "quadric:4096x4096:d6:fast",
    "simple:1024x1024:d6:parity", "simple:1024x1024:d6:fast",
    "reflection:2048x2048:d6:parity", "reflection:2048x2048:d6:fast",
    "quadric:1024x1024:d6:parity", "quadric:1024x1024:d6:fast",
    "quadric:512x384:d6:parity", "quadric:333x517:d6:parity", "reflection:1x1:d6:parity",
    "quadric:7x3:d6:parity", "quadric:1x4096:d6:parity"])
def test_configs(key, scenes, table):
    scene, size, d, mode = key.split(":")
    w, h = map(int, size.split("x"))
    img = rc.render(scenes[scene], w, h, depth=int(d[1:]), mode=mode)
    assert p3_md5(img) == table[key]["md5"], key


SCHEDULES = {"no-side": dict(side=0), "side-always": dict(side=1), "side-by-size": dict(side=2),
             "in-resolver+no-dep-fast": dict(side=3, dep_fast=0),
             "in-resolver+no-helpers": dict(side=3, helpers=0),
             "in-resolver-until-done": dict(side=4),
             "no-block-segments": dict(block_min=0),
             "block-segments-256": dict(block_min=256),
             "split-shade": dict(split_shade=1, side=1),
             "resolve-shared": dict(resolve_shared=1), "no-dep-fast": dict(dep_fast=0),
             "no-side+no-dep-fast": dict(side=0, dep_fast=0),
             "no-side+phase-c-finish": dict(side=0, phase_c_finish=1), "no-o0": dict(o0=0),
             "no-x0": dict(x0=0),
             "hand-run-1": dict(hand_run=1), "helpers-1": dict(helpers=1),
             "no-helpers": dict(helpers=0), "no-coop": dict(coop=0),
             "small-grid": dict(resolve_grid=64, team_blocks=16),
             "serial-plain-d2h": dict(overlap_d2h=0, staged_d2h=0, prefault=0),
             "device-patch": dict(patch_host=0),
             "mapped-patch-after-frame": dict(patch_host=1),
             "helpers-8-hand-run-512": dict(helpers=8, hand_run=512),
             "no-headb-first": dict(headb_first=0)}


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_parity_schedules(sched, scenes, table):
    """The parity pipeline's alternative schedules (rc_set_tuning) give the same bytes:
    phase C after the resolver only (side=0: clean entries, then full waves of the rest —
    k_dep_chunks; with phase_c_finish through k_finish's batch claims), phase C beside the
    resolver at every size (side=1; by default only from 8 Mpixel), colours shaded beside
    the resolver (split_shade), no one-workgroup-per-CU reservation (resolve_shared, which
    also disables the side stream), every first-bounce-miss pixel recomputed in phase C
    (dep_fast=0), primary rays through the general intersection tests instead of the origin-
    zero forms (o0=0), the quadric tests with their cross terms although they are zero (x0=0),
    a hand-off to the helper blocks after every change (hand_run=1: the
    queue overflows), a single helper block, none, the lane-only evaluator (coop=0), a small
    resolver grid, the plain serial copy to the host, the colour patch through a device buffer
    (patch_host=0: a device buffer copied after phase C), the mapped patch scattered after the
    frame instead of entry by entry during it (patch_host=1: its frames leave the mapped array
    marked, so the next schedule's default frames also check that it is cleared before use) and
    the round-3 helper settings."""
    with rc.tuned(**SCHEDULES[sched]):
        for key in ("quadric:4096x4096:d6:parity", "reflection:2048x2048:d4:parity",
                    "quadric:333x517:d6:parity"):
            scene, size, d, mode = key.split(":")
            w, h = map(int, size.split("x"))
            img = rc.render(scenes[scene], w, h, depth=int(d[1:]), mode=mode)
            assert p3_md5(img) == table[key]["md5"], (sched, key)


@pytest.mark.parametrize("n_shapes", [20, 33, 64, 65, 90])
def test_many_shapes_vs_oracle(n_shapes, tmp_path):
    """Scenes beyond the examples' sizes: 32-lane groups, the non-speculative cooperative
    evaluator (64 lanes per entry), the resolver without LDS-staged shapes (> 64) and the
    reflectivity test without the bitmask — against the CPU oracle, every depth class."""
    rng = np.random.default_rng(1000 + n_shapes)
    path = str(tmp_path / f"m{n_shapes}.scene")
    random_scene(rng, path, n_shapes, 2)
    s = rc.Scene.from_file(path)
    for mode in ("parity", "fast"):
        for d in (1, 4, 6):
            want, st = oracle_render(s, 96, 72, d, mode)
            if not st["parity_defined"]:
                continue
            np.testing.assert_array_equal(rc.render(s, 96, 72, depth=d, mode=mode), want,
                                          err_msg=f"{n_shapes} shapes {mode} d{d}")


ZERO_EVENT_PLANES = [((0, 0, 1), 0.5, ""), ((0, 0.6, 0.8), 0.5, ""), ((0, 0.28, 0.96), 0.5, ""),
                     ((0.6, 0, 0.8), 0.4, "sphere, radius: 1.0, diffuse_color: [1, 0, 0], "
                      "specular_color: [1, 1, 1], position: [0, 3, -2], reflectivity: 0.5, "
                      "refractivity: 0.0, ior: 1.0\n")]


@pytest.mark.parametrize("x0", [1, 0])
@pytest.mark.parametrize("cross", [False, True])
def test_quadric_cross_terms_vs_oracle(cross, x0, tmp_path):
    """Quadrics with and without cross coefficients d, e, f (C/raycast.c:614-656).  Without
    them (every example scene) the kernels drop the cross terms (rc_device.hpp quad_abc,
    rc_tuning.x0); with them, or with x0 = 0, the full accumulations run.  Against the CPU
    oracle, both modes, every depth class, one frame at a time."""
    rng = np.random.default_rng(77 + int(cross))
    path = str(tmp_path / f"q{int(cross)}.scene")
    random_scene(rng, path, 14, 2, cross=cross)
    s = rc.Scene.from_file(path)
    with rc.tuned(x0=x0):
        for mode in ("parity", "fast"):
            for d in (1, 4, 6):
                want, st = oracle_render(s, 96, 72, d, mode)
                if not st["parity_defined"]:
                    continue
                np.testing.assert_array_equal(rc.render(s, 96, 72, depth=d, mode=mode), want,
                                              err_msg=f"cross={cross} x0={x0} {mode} d{d}")


@pytest.mark.parametrize("cam,y", [(20, "1.2e38"), (2000, "1.5e38")])
def test_cross_term_nan_rejection(cam, y, tmp_path):
    """Hit points beyond float range: two mirror planes at y = -+1.2e38 (or 1.5e38) send the
    second bounce's hit point to +-inf, where the reference's zero cross terms of a quadric
    test become NaN (0 * inf) and reject the quadric.  The kernels' cross-term-free form
    reproduces that through x0_reject (rc_device.hpp); the oracle's diagnostic counter shows
    the case is exercised.  Parity and fast mode, x0 on and off, against the oracle."""
    path = tmp_path / "xnan.scene"
    path.write_text(cross_nan_scene_text(cam, y))
    s = rc.Scene.from_file(str(path))
    lib = oracle_lib()
    for x0 in (1, 0):
        with rc.tuned(x0=x0):
            for mode in ("parity", "fast"):
                for w, h, d in ((64, 48, 6), (7, 5, 4)):
                    lib.rco_cross_nan_events(1)
                    want, st = oracle_render(s, w, h, d, mode)
                    if w == 64:
                        assert lib.rco_cross_nan_events(1) > 0, "the NaN cross-term case is not hit"
                    if not st["parity_defined"]:
                        continue
                    np.testing.assert_array_equal(rc.render(s, w, h, depth=d, mode=mode), want,
                                                  err_msg=f"x0={x0} {mode} {w}x{h} d{d}")


@pytest.mark.parametrize("case", range(len(ZERO_EVENT_PLANES)))
@pytest.mark.parametrize("fast_dep", [True, False])
@pytest.mark.parametrize("side", [0, 1, 3])
def test_zero_normalize_events(case, fast_dep, side, tmp_path):
    """Zero-length normalize events (C/v3math.c:183-187; raycast() prints one stderr line per
    event): a point light exactly on the hit point of the 1x1 image's ray.  The pixel is a
    first-bounce miss; phase A counts its primary part and phase C the rest, with the clean-
    entry path (Scene::dep_fast) on or off.  Counts and bytes against the CPU oracle."""
    nrm, refl, extra = ZERO_EVENT_PLANES[case]
    path = tmp_path / "z.scene"
    path.write_text("camera, width: 2.0, height: 2.0\n"
                    f"plane, normal: [{nrm[0]}, {nrm[1]}, {nrm[2]}], diffuse_color: [0.3, 0.5, 0.7], "
                    f"specular_color: [1, 1, 1], position: [0, 0, -5], reflectivity: {refl}\n"
                    + extra +
                    "light, color: [4, 4, 4], radial-a2: 0.01, radial-a1: 0.0125, "
                    "radial-a0: 0.0125, position: [0, 0, -5]\n")
    s = rc.Scene.from_file(str(path))
    # side=0: phase C after the resolver (k_dep_chunks); 1: k_side; 3: the resolver's waves
    with rc.tuned(dep_fast=int(fast_dep), side=side):
        for w, h in ((1, 1), (2, 1), (3, 1), (1, 3)):
            want, st = oracle_render(s, w, h, 6, "parity")
            tim = {}
            got = rc.render(s, w, h, depth=6, mode="parity", timing=tim)
            np.testing.assert_array_equal(got, want, err_msg=f"{w}x{h}")
            assert tim["zero_normalize"] == st["zero_normalize"], (w, h, tim, st["zero_normalize"])
    assert oracle_render(s, 1, 1, 6, "parity")[1]["zero_normalize"] > 0


def test_c5_8192(scenes, table):
    """C5 image (quadric 8192x8192 d6) on one GPU, both modes."""
    for mode in ("parity", "fast"):
        img = rc.render(scenes["quadric"], 8192, 8192, depth=6, mode=mode)
        key = golden_key("quadric", 8192, 8192, 6, mode)
        assert p3_md5(img) == table[key]["md5"], key


def test_oracle_random_sizes(scenes):
    """GPU == oracle on odd sizes and depths (covers partial tiles and every depth)."""
    rng = np.random.default_rng(7)
    for _ in range(6):
        name = SMALL[int(rng.integers(0, len(SMALL)))]
        w, h = int(rng.integers(1, 130)), int(rng.integers(1, 130))
        d = int(rng.integers(0, 8))
        for mode in ("parity", "fast"):
            ref, _ = oracle_render(scenes[name], w, h, d, mode)
            img = rc.render(scenes[name], w, h, depth=d, mode=mode)
            np.testing.assert_array_equal(img, ref, err_msg=f"{name} {w}x{h} d{d} {mode}")


def test_repeat_deterministic(scenes):
    """The carry resets per call: two renders in one process are identical."""
    a = rc.render(scenes["quadric"], 300, 200, depth=6)
    b = rc.render(scenes["quadric"], 300, 200, depth=6)
    np.testing.assert_array_equal(a, b)


def test_cli_dropin(tmp_path, table):
    """bin/raytrace: same CLI, same P3 bytes, same timing line as C/raycast.c:19-69."""
    exe = os.path.join(ROOT, "raytracing-programs_amd", "bin", "raytrace")
    out = tmp_path / "q.ppm"
    r = subprocess.run([exe, "256", "256", scene_path("quadric"), str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("Time (sec) to create a 256x256 image with 5 shape(s) and "
                               "2 light(s): ")
    assert file_md5(str(out)) == table["quadric:256x256:d6:parity"]["md5"]
    env = dict(os.environ, RAYCAST_DEPTH="4", RAYCAST_MODE="fast")
    r = subprocess.run([exe, "256", "256", scene_path("quadric"), str(out)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert file_md5(str(out)) == table["quadric:256x256:d4:fast"]["md5"]


OPTB = os.path.join(ROOT, "oracle", "_ref", "raytrace_optb")


@pytest.mark.skipif(not os.path.exists(OPTB), reason="oracle/_ref not built (make ref)")
def test_option_b_reference_main(tmp_path, table):
    """INTEGRATION.md Option B: the reference's own program (C/raycast.c:19-69 main, its own
    parse.c / ppm.c) with its raycast() fenced off by #ifndef RAYCAST_HIP (oracle/Makefile),
    linked against libraycast_hip.so: C1 and C4 files md5-equal to the reference's."""
    for scene, n, key, counts in [("simple", 256, "simple:256x256:d6:parity", (4, 1)),
                                  ("quadric", 4096, "quadric:4096x4096:d6:parity", (5, 2))]:
        out = tmp_path / f"{scene}.ppm"
        r = subprocess.run([OPTB, str(n), str(n), scene_path(scene), str(out)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        # main's own report; its num_lights starts uninitialised (C/raycast.c:41-44)
        assert f"image with {counts[0]} shape(s) and {counts[1]} light(s)" in r.stdout, r.stdout
        assert file_md5(str(out)) == table[key]["md5"], key


def test_device_render_matches_host(scenes, table):
    """rc_render_device (device-resident output, the bench path) writes the same bytes."""
    torch = pytest.importorskip("torch")
    out = torch.empty((512, 512, 3), dtype=torch.uint8, device="cuda")
    rc.render_device(scenes["quadric"], 512, 512, out.data_ptr(),
                     torch.cuda.current_stream().cuda_stream, depth=6, mode="parity")
    torch.cuda.synchronize()
    ref = rc.render(scenes["quadric"], 512, 512, depth=6, mode="parity")
    np.testing.assert_array_equal(out.cpu().numpy(), ref)
    # row-cyclic shard (fast mode): rows 1, 4, 7, ... of a 512x512 image
    rows = (512 - 1 + 2) // 3
    sh = torch.empty((rows, 512, 3), dtype=torch.uint8, device="cuda")
    rc.render_device(scenes["quadric"], 512, 512, sh.data_ptr(),
                     torch.cuda.current_stream().cuda_stream, depth=6, mode="fast", row0=1,
                     row_step=3, nrows=rows)
    torch.cuda.synchronize()
    full = rc.render(scenes["quadric"], 512, 512, depth=6, mode="fast")
    np.testing.assert_array_equal(sh.cpu().numpy(), full[1::3])


PIPES = {"default": {},
         "slot-streams": dict(pipe_slotstreams=1),
         "three-lanes": dict(pipe_resolvers=3, pipe_res_cus=144, pipe_slots=6),
         "one-lane-small-a": dict(pipe_resolvers=1, pipe_res_cus=32, pipe_timing=0),
         "one-wg-per-cu": dict(resolve_lds_kb=96, team_blocks=24),
         "phase-c-in-lanes": dict(pipe_inres=1),
         "phase-c-in-lanes-until-done": dict(pipe_inres=2, pipe_slotstreams=1),
         "no-lane-helpers": dict(pipe_helpers=0),
         "lane-helpers-every-run": dict(pipe_helpers=8, hand_run=2),
         "stream-order-1": dict(pipe_order=1),
         "queue-per-lane": dict(pipe_order=3),
         "one-phase-c-stream": dict(pipe_order=4),
         "last-phase-c-on-partition": dict(pipe_last_whole=0)}


@pytest.mark.parametrize("pipe", list(PIPES))
def test_frames_in_flight(pipe, scenes, table):
    """rc_frame_submit: consecutive frames overlap on two CU partitions (the resolver of one
    beside the pixel phases of the next); every frame is still byte-identical.  Mixed scenes,
    sizes and modes exercise the slot workspaces' re-use and re-upload; the pipeline is
    rebuilt (rc_pipe_reset) under each partition / stream layout."""
    torch = pytest.importorskip("torch")
    saved = rc.get_tuning()
    rc.set_tuning(**PIPES[pipe])
    rc.pipe_reset()
    seq = ["quadric:4096x4096:d6:parity", "reflection:2048x2048:d4:parity",
           "quadric:4096x4096:d6:parity", "simple:1024x1024:d6:parity",
           "quadric:1024x1024:d6:fast", "quadric:512x384:d6:parity",
           "quadric:4096x4096:d6:parity", "quadric:4096x4096:d6:parity"]
    jobs = []
    for key in seq:
        scene, size, d, mode = key.split(":")
        w, h = map(int, size.split("x"))
        jobs.append((key, scene, w, h, int(d[1:]), mode,
                     torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")))
    torch.cuda.synchronize()
    for _ in range(2):   # a second round re-uses both slots' workspaces
        for key, scene, w, h, d, mode, buf in jobs:
            buf.zero_()
        torch.cuda.synchronize()
        for key, scene, w, h, d, mode, buf in jobs:
            rc.frame_submit(scenes[scene], w, h, buf.data_ptr(), depth=d, mode=mode)
        tim = {}
        rc.frames_wait(tim)
        assert tim["resolve_ms"] > 0.0 or PIPES[pipe].get("pipe_timing") == 0
        # every parity frame's hand-off words read back (the fast-mode frame has none)
        assert (tim["frames_checked"], tim["frames_failed"]) == (7, 0), tim
        for key, scene, w, h, d, mode, buf in jobs:
            assert p3_md5(buf.cpu().numpy()) == table[key]["md5"], (pipe, key)
    rc.set_tuning(**saved)
    rc.pipe_reset()   # later tests get the default pipeline


def test_random_scene_sweep_vs_oracle(tmp_path):
    """Sixteen random phantom-safe scenes (2-12 shapes, one or two lights, odd sizes, depths
    2-7) against the CPU oracle: one frame at a time (rc_render) and as one window of frames
    in flight (rc_frame_submit, every scene's frame in one window, the last one's phase C on
    every CU in rc_frames_wait).  Parity mode, where the scan-order carry chains are."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(2025)
    cases = []
    for seed in range(16):
        path = str(tmp_path / f"r{seed}.scene")
        random_scene(rng, path, int(rng.integers(2, 13)), int(rng.integers(1, 3)))
        s = rc.Scene.from_file(path)
        w, h, d = int(rng.integers(96, 320)), int(rng.integers(64, 256)), int(rng.integers(2, 8))
        want, st = oracle_render(s, w, h, d, "parity")
        if not st["parity_defined"]:
            continue
        np.testing.assert_array_equal(rc.render(s, w, h, depth=d, mode="parity"), want,
                                      err_msg=f"scene {seed} {w}x{h} d{d}")
        cases.append((seed, s, w, h, d, want,
                      torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")))
    assert len(cases) >= 8
    torch.cuda.synchronize()
    for seed, s, w, h, d, want, buf in cases:
        rc.frame_submit(s, w, h, buf.data_ptr(), depth=d, mode="parity")
    tim = {}
    rc.frames_wait(tim)
    assert (tim["frames_checked"], tim["frames_failed"]) == (len(cases), 0), tim
    for seed, s, w, h, d, want, buf in cases:
        np.testing.assert_array_equal(buf.cpu().numpy(), want, err_msg=f"in flight: scene {seed}")


LIGHT = ("light, color: [1.5, 1.2, 1.0], radial-a2: 0.01, radial-a1: 0.0125, radial-a0: 0.0125, "
         "position: [3, 6, 1]\n")
DEGENERATE = {
    "no-shapes": LIGHT,
    "no-lights": "sphere, radius: 1.0, diffuse_color: [1, 0, 0], specular_color: [1, 1, 1], "
                 "position: [0, 0, -5], reflectivity: 0.5, refractivity: 0, ior: 1\n",
    "matte-only": "sphere, radius: 1.0, diffuse_color: [1, 0, 0], specular_color: [1, 1, 1], "
                  "position: [0, 0, -5], reflectivity: 0, refractivity: 0, ior: 1\n"
                  "plane, normal: [0, 1, 0], diffuse_color: [0.3, 0.3, 0.3], "
                  "position: [0, -1, 0], reflectivity: 0\n" + LIGHT,
    "mirror-box": "".join(
        f"plane, normal: [{n}], diffuse_color: [0.4, 0.5, 0.6], specular_color: [1, 1, 1], "
        f"position: [{p}], reflectivity: 0.9\n"
        for n, p in (("0, 1, 0", "0, -2, 0"), ("0, -1, 0", "0, 2, 0"), ("1, 0, 0", "-2, 0, 0"),
                     ("-1, 0, 0", "2, 0, 0"), ("0, 0, 1", "0, 0, -8"))) + LIGHT,
    "lone-mirror-plane": "plane, normal: [0, 0.6, 0.8], diffuse_color: [0.2, 0.7, 0.3], "
                         "specular_color: [1, 1, 1], position: [0, 0, -6], reflectivity: 1.0\n"
                         + LIGHT,
    "full-reflect-sphere": "sphere, radius: 2.0, diffuse_color: [0, 0, 1], specular_color: "
                           "[1, 1, 1], position: [0, 0, -6], reflectivity: 1.0, refractivity: 0, "
                           "ior: 1\n" + LIGHT,
}


@pytest.mark.parametrize("case", list(DEGENERATE))
def test_degenerate_scenes(case, tmp_path):
    """Edge scenes against the oracle, every depth class and mode, one frame at a time and
    with frames in flight: no shapes, no lights, nothing reflective (no carry at all), a
    closed mirror box (deep bounce chains), a lone mirror plane and a perfect mirror sphere
    (every first bounce misses: the image is one long carry segment)."""
    torch = pytest.importorskip("torch")
    path = tmp_path / f"{case}.scene"
    path.write_text("camera, width: 2.0, height: 2.0\n" + DEGENERATE[case])
    s = rc.Scene.from_file(str(path))
    bufs = []
    for w, h in ((64, 48), (7, 5)):
        for d in (0, 1, 4, 6):
            for mode in ("parity", "fast"):
                want, st = oracle_render(s, w, h, d, mode)
                if not st["parity_defined"]:
                    continue
                np.testing.assert_array_equal(rc.render(s, w, h, depth=d, mode=mode), want,
                                              err_msg=f"{case} {w}x{h} d{d} {mode}")
                buf = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
                bufs.append((buf, want, f"{case} {w}x{h} d{d} {mode} in flight"))
    torch.cuda.synchronize()
    for buf, want, msg in bufs:
        h, w, _ = want.shape
        d = int(msg.split(" d")[1].split()[0])
        rc.frame_submit(s, w, h, buf.data_ptr(), depth=d, mode=msg.split()[3])
    rc.frames_wait()
    for buf, want, msg in bufs:
        np.testing.assert_array_equal(buf.cpu().numpy(), want, err_msg=msg)


PHANTOM_TABLE = os.path.join(GOLDEN, "phantom_md5.json")


def test_phantom_lit():
    """Scenes whose phantom record is lit (shapes_list[-1], C/raycast.c:87-89,382; SURVEY.md §8
    a15): four lights (light bytes [184, 288)) and two lights with L1.pos.y + L1.pos.z < 1
    (bytes [40, 144)).  Every reflection miss shades the phantom, so the device's phantom
    record and phase C without the clean-entry shortcut (Scene::dep_fast = 0) decide the
    bytes.  Parity: md5 of the reference's own output (tests/golden/make_phantom_golden.py) at
    depths 1/4/6, one frame at a time and with frames in flight; fast mode against the oracle."""
    import json
    torch = pytest.importorskip("torch")
    table = json.load(open(PHANTOM_TABLE))
    scenes = {n: rc.Scene.from_file(scene_path(n)) for n in ("phantom_four", "phantom_two")}
    jobs = []
    for key, want in sorted(table.items()):
        name, size, d, mode = key.split(":")
        w, h = map(int, size.split("x"))
        img = rc.render(scenes[name], w, h, depth=int(d[1:]), mode=mode)
        assert p3_md5(img) == want["md5"], key
        jobs.append((key, name, w, h, int(d[1:]),
                     torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")))
    torch.cuda.synchronize()
    for key, name, w, h, d, buf in jobs:
        rc.frame_submit(scenes[name], w, h, buf.data_ptr(), depth=d, mode="parity")
    rc.frames_wait()
    for key, name, w, h, d, buf in jobs:
        assert p3_md5(buf.cpu().numpy()) == table[key]["md5"], key + " in flight"
    for name, s in scenes.items():
        for d in (1, 4, 6):
            want, st = oracle_render(s, 200, 150, d, "fast")
            np.testing.assert_array_equal(rc.render(s, 200, 150, depth=d, mode="fast"), want,
                                          err_msg=f"{name} fast d{d}")


def test_bench_sequence_8192(table):
    """bench.py's order at the C5 image size (a lone frame issued after the frame
    pipeline once timed out): lone rc_render_device frames, then 22 frames in flight, then
    lone rc_render frames into host memory — every image md5-equal to the reference's (each
    in-flight frame has its own buffer: bytes equal to frame 0's on the device, frame 0's md5)
    and every frame's carry hand-offs read back."""
    torch = pytest.importorskip("torch")
    n = 8192
    want = table["quadric:8192x8192:d6:parity"]["md5"]
    s = rc.Scene.from_file(scene_path("quadric"))
    out = torch.empty((n, n, 3), dtype=torch.uint8, device="cuda")
    rc.lone_frames_check()
    for _ in range(2):
        rc.render_device(s, n, n, out.data_ptr(), depth=6, mode="parity")
    torch.cuda.synchronize()
    assert rc.lone_frames_check() == {"checked": 2, "failed": 0}
    assert p3_md5(out.cpu().numpy()) == want, "lone device frame"
    outs = [torch.empty((n, n, 3), dtype=torch.uint8, device="cuda") for _ in range(22)]
    torch.cuda.synchronize()
    rc.frames_wait()
    for o in outs:
        rc.frame_submit(s, n, n, o.data_ptr(), depth=6, mode="parity")
    tim = {}
    rc.frames_wait(tim)
    assert (tim["frames_checked"], tim["frames_failed"]) == (22, 0)
    assert p3_md5(outs[0].cpu().numpy()) == want, "in flight, frame 0"
    for i, o in enumerate(outs):
        assert torch.equal(o, outs[0]), f"in flight, frame {i}"
    del outs
    for i in range(2):
        assert p3_md5(rc.render(s, n, n, depth=6, mode="parity")) == want, f"lone rc_render {i}"


# ------------------------------------------------- CUDA-port semantics --
# RC_MODE_CUDA against its CPU restatement (oracle/rc_oracle_cuda.c): bit-exact.  The
# restatement itself is parity-unpinned against the CUDA binary (no nvcc).
CUDA_DEPTHS = (0, 1, 6, 50)


@pytest.mark.parametrize("scene", SMALL)
def test_cuda_mode_vs_oracle(scene, scenes):
    from helpers import oracle_render_cuda
    for d in CUDA_DEPTHS:
        want = oracle_render_cuda(scenes[scene], 96, 72, d)
        np.testing.assert_array_equal(rc.render(scenes[scene], 96, 72, depth=d, mode="cuda"),
                                      want, err_msg=f"{scene} d{d}")


@pytest.mark.parametrize("n_shapes", [7, 33, 65])
def test_cuda_mode_random_scenes(n_shapes, tmp_path):
    from helpers import oracle_render_cuda
    rng = np.random.default_rng(4000 + n_shapes)
    path = str(tmp_path / f"c{n_shapes}.scene")
    random_scene(rng, path, n_shapes, 2)
    s = rc.Scene.from_file(path)
    for d in (4, 50):
        w, h = int(rng.integers(1, 140)), int(rng.integers(1, 140))
        np.testing.assert_array_equal(rc.render(s, w, h, depth=d, mode="cuda"),
                                      oracle_render_cuda(s, w, h, d),
                                      err_msg=f"{n_shapes} shapes {w}x{h} d{d}")


def test_cuda_mode_cli_and_device(tmp_path, scenes):
    """RAYCAST_MODE=cuda through the drop-in CLI (50 bounces by default, MAX_ITER) and the
    device-resident entry point."""
    from helpers import oracle_render_cuda, read_p3
    want = oracle_render_cuda(scenes["reflection"], 200, 150, 50)
    exe = os.path.join(ROOT, "raytracing-programs_amd", "bin", "raytrace")
    out = tmp_path / "c.ppm"
    env = dict(os.environ, RAYCAST_MODE="cuda")
    env.pop("RAYCAST_DEPTH", None)
    r = subprocess.run([exe, "200", "150", scene_path("reflection"), str(out)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(read_p3(str(out)), want)
    torch = pytest.importorskip("torch")
    d = torch.empty((150, 200, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc.render_device(scenes["reflection"], 200, 150, d.data_ptr(), depth=50, mode="cuda")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d.cpu().numpy(), want)


@pytest.mark.parametrize("a0", [-2, -5, 2.5, 7.25])
def test_spot_exponents_beyond_references(a0, tmp_path):
    """Spot exponents no reference scene has (negative integers: pown_dd's reciprocal;
    non-integers: the device pow) against the oracle's glibc pow, both modes — image-level
    parity (scripts/spot_exp_probe.py covers more cases)."""
    base = open(scene_path("reflection")).read().rstrip("\n")
    path = tmp_path / "spot.scene"
    path.write_text(base + "\nlight, color: [1.5, 1.2, 1.0], radial-a2: 0.01, radial-a1: 0.0125, "
                    "radial-a0: 0.0125, position: [0, 2, 0], theta: 0.9, "
                    f"angular-a0: {a0}, direction: [0, -0.3, -1]\n")
    s = rc.Scene.from_file(str(path))
    for mode in ("fast", "parity"):
        want, st = oracle_render(s, 128, 128, 4, mode)
        assert st["parity_defined"]
        np.testing.assert_array_equal(rc.render(s, 128, 128, depth=4, mode=mode), want,
                                      err_msg=f"a0={a0} {mode}")


SPOT_ZERO_ALPHA_SCENE = (
    "camera, width: 2.0, height: 2.03125\n"
    "plane, normal: [0, 0, 1], diffuse_color: [0.6, 0.5, 0.4], position: [0, 0, -8], "
    "reflectivity: 0\n"
    "sphere, radius: 1.0, diffuse_color: [0.2, 0.7, 0.3], specular_color: [0.5, 0.5, 0.5], "
    "position: [1.5, 0.25, -6], reflectivity: 0.3, refractivity: 0, ior: 1\n"
    "light, color: [2e-5, 1.5e-5, 1e-5], radial-a2: 0.01, radial-a1: 0.0125, radial-a0: 0.0125, "
    "position: [0, 0, -3], theta: 1.05, angular-a0: -3, direction: [-0, -1, -0]\n"
    "light, color: [1.5, 1.2, 1.0], radial-a2: 0.01, radial-a1: 0.0125, radial-a0: 0.0125, "
    "position: [5, 5, 0]\n")


def test_spot_zero_alpha_negative_exponent(tmp_path):
    """alpha == +-0 under a negative odd spot exponent: the reference's pow gives +-inf there
    (white or black), which pown_dd has to give too.  The light sits at y = 0 and points straight
    down; its cone is wider than 90 degrees (cos_theta < 0), so alpha = +-0 passes the cone test.
    The camera's height is 65 / 32 and the image has 65 rows, so the middle row's rays have
    d.y = +0 exactly and every hit point of that row lies in the plane through the light
    perpendicular to its direction: v.y = P.y - L.y = +0 and alpha = (v.x * -0 + 0 * -1) + v.z * -0
    = +0 on either side of the light (v.z < 0), so pow(+0, -3) = +inf and the wall's middle row
    is white.  (L.y - P.y is +0 as well, not -0: negating a dot product with ld, the device's
    earlier shortcut, gives alpha = -0 and -inf — black — where v.x < 0.)  The second light
    gives the rest of the picture ordinary shades."""
    path = tmp_path / "zero_alpha.scene"
    path.write_text(SPOT_ZERO_ALPHA_SCENE)
    s = rc.Scene.from_file(str(path))
    light = s.js.lights_list.contents
    assert light.cos_theta < 0 and light.a0 == -3.0
    W, H = 64, 65
    for mode in ("fast", "parity"):
        want, st = oracle_render(s, W, H, 4, mode)
        assert st["parity_defined"]
        # the edge is in the picture: the wall's part of the middle row is saturated on both sides
        # of the light (x < W / 2 and x > W / 2), and hardly a pixel of any other row is
        white = (want[H // 2] == 255).all(1)
        assert white[: W // 2].sum() >= W // 4 and white[W // 2:].sum() >= W // 8
        assert (np.delete(want, H // 2, 0) == 255).all(2).sum() <= 4
        np.testing.assert_array_equal(rc.render(s, W, H, depth=4, mode=mode), want, err_msg=mode)


def test_concurrent_callers_one_device(scenes, table):
    """Host threads calling raycast()/rc_render on the same device at once (ctypes drops the
    GIL): the per-device lock serialises them on the shared workspace, the resolver's
    TeamState and the copy pool, so every image stays byte-identical."""
    import threading
    keys = ["quadric:1024x1024:d6:parity", "reflection:2048x2048:d4:parity",
            "simple:1024x1024:d6:fast", "quadric:512x384:d6:parity"] * 2
    got, errs = {}, []

    def worker(i, key):
        try:
            scene, size, d, mode = key.split(":")
            w, h = map(int, size.split("x"))
            for rep in range(3):
                img = rc.render(scenes[scene], w, h, depth=int(d[1:]), mode=mode)
                got[(i, rep)] = (key, p3_md5(img))
        except Exception as e:   # pragma: no cover - reported below
            errs.append(repr(e))

    ts = [threading.Thread(target=worker, args=(i, k)) for i, k in enumerate(keys)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(100)
    assert not errs, errs
    assert len(got) == 3 * len(keys)
    for (key, md5) in got.values():
        assert md5 == table[key]["md5"], key


def test_lone_renders_beside_frames_in_flight(scenes, table):
    """A caller's raycast()/rc_render issued while another thread's frames are still in
    flight (rc_frame_submit without rc_frames_wait): the lone frame's resolver waits for CUs
    the pipeline's resolvers hold (its team spins are bounded, the pipeline's resolvers never
    wait on it), and every image of both callers is byte-identical."""
    import threading
    torch = pytest.importorskip("torch")
    seq = ["quadric:4096x4096:d6:parity", "reflection:2048x2048:d4:parity"] * 4
    bufs = []
    for key in seq:
        _, size, _, _ = key.split(":")
        w, h = map(int, size.split("x"))
        bufs.append(torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    lone, errs = [], []

    def lone_caller():
        try:
            for key in ["quadric:4096x4096:d6:parity", "quadric:512x384:d6:parity"] * 2:
                scene, size, d, mode = key.split(":")
                w, h = map(int, size.split("x"))
                img = rc.render(scenes[scene], w, h, depth=int(d[1:]), mode=mode)
                lone.append((key, p3_md5(img)))
        except Exception as e:   # pragma: no cover - reported below
            errs.append(repr(e))

    t = threading.Thread(target=lone_caller)
    for i, (key, buf) in enumerate(zip(seq, bufs)):
        scene, size, d, mode = key.split(":")
        w, h = map(int, size.split("x"))
        rc.frame_submit(scenes[scene], w, h, buf.data_ptr(), depth=int(d[1:]), mode=mode)
        if i == 1:
            t.start()
    t.join(100)
    rc.frames_wait({})
    assert not errs, errs
    assert len(lone) == 4
    for key, md5 in lone:
        assert md5 == table[key]["md5"], ("lone", key)
    for key, buf in zip(seq, bufs):
        assert p3_md5(buf.cpu().numpy()) == table[key]["md5"], ("in flight", key)


def test_injected_hand_off_failure_in_flight(scenes, table):
    """a failed carry hand-off in frame 2 of 8 in flight
    (rc_debug_inject_error: its resolver raises the error word as a timed-out spin would) is
    caught although slot 2 is reused by frame 6 (which resets the TeamState): rc_frame_submit
    refuses new frames once the failure has arrived, rc_frames_wait raises and counts it, the
    other frames are byte-identical, and the pipeline then renders and verifies normally."""
    torch = pytest.importorskip("torch")
    n, key = 1024, "quadric:1024x1024:d6:parity"
    want = table[key]["md5"]
    s = scenes["quadric"]
    bufs = [torch.zeros((n, n, 3), dtype=torch.uint8, device="cuda") for _ in range(8)]
    torch.cuda.synchronize()
    rc.frames_wait()
    rc.inject_error(2)
    submitted = 0
    try:
        for b in bufs:
            rc.frame_submit(s, n, n, b.data_ptr(), depth=6)
            submitted += 1
    except RuntimeError:
        assert submitted > 2, "refused before the failing frame was submitted"
    with pytest.raises(RuntimeError, match=f"1 of {submitted} frames"):
        rc.frames_wait()
    for i in range(submitted):
        if i != 2:
            assert p3_md5(bufs[i].cpu().numpy()) == want, f"frame {i}"
    for b in bufs[:4]:
        rc.frame_submit(s, n, n, b.data_ptr(), depth=6)
    tim = {}
    rc.frames_wait(tim)
    assert (tim["frames_checked"], tim["frames_failed"]) == (4, 0)
    for b in bufs[:4]:
        assert p3_md5(b.cpu().numpy()) == want


def test_injected_hand_off_failure_lone(scenes, table):
    """One frame at a time: rc_render_device returns before its frame has run, so a failed
    hand-off is reported by the device's next call (once), or by rc_render_device with timing
    for its own frame, or by rc_lone_frames_check."""
    torch = pytest.importorskip("torch")
    n, key = 1024, "quadric:1024x1024:d6:parity"
    want = table[key]["md5"]
    s = scenes["quadric"]
    out = torch.empty((n, n, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc.lone_frames_check()
    rc.inject_error(0)
    rc.render_device(s, n, n, out.data_ptr(), depth=6)   # enqueued: returns at once
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        rc.render_device(s, n, n, out.data_ptr(), depth=6)   # reports the previous frame
    rc.render_device(s, n, n, out.data_ptr(), depth=6)
    torch.cuda.synchronize()
    assert p3_md5(out.cpu().numpy()) == want
    assert rc.lone_frames_check() == {"checked": 1, "failed": 0}
    rc.inject_error(0)
    with pytest.raises(RuntimeError):
        rc.render_device(s, n, n, out.data_ptr(), depth=6, timing={})
    rc.inject_error(0)
    rc.render_device(s, n, n, out.data_ptr(), depth=6)
    with pytest.raises(RuntimeError, match="1 of 1"):
        rc.lone_frames_check()
    tim = {}
    rc.render_device(s, n, n, out.data_ptr(), depth=6, timing=tim)
    assert tim["frames_checked"] == 1 and tim["frames_failed"] == 0
    assert p3_md5(out.cpu().numpy()) == want
    with pytest.raises(RuntimeError):   # rc_render (host pixmap) reports its own frame
        rc.inject_error(0)
        rc.render(s, n, n, depth=6)
    assert p3_md5(rc.render(s, n, n, depth=6)) == want


def test_render_device_two_streams(scenes, table):
    """rc_render_device returns before its frame has run; a second caller on
    another stream must not overwrite the shared one-frame workspace meanwhile (the workspace
    event orders the two streams).  Two threads, two torch streams, md5 of every image."""
    import threading
    torch = pytest.importorskip("torch")
    keys = [("quadric", 4096, 6), ("reflection", 2048, 4)]
    res, errs = {}, []

    def worker(i):
        try:
            name, n, d = keys[i]
            st = torch.cuda.Stream()
            bufs = [torch.empty((n, n, 3), dtype=torch.uint8, device="cuda") for _ in range(3)]
            torch.cuda.synchronize()
            for b in bufs:
                rc.render_device(scenes[name], n, n, b.data_ptr(), st.cuda_stream, depth=d)
            st.synchronize()
            res[i] = [p3_md5(b.cpu().numpy()) for b in bufs]
        except Exception as e:   # pragma: no cover - reported below
            errs.append(repr(e))

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errs, errs
    for i, (name, n, d) in enumerate(keys):
        want = table[f"{name}:{n}x{n}:d{d}:parity"]["md5"]
        assert res[i] == [want] * 3, name
    assert rc.lone_frames_check()["failed"] == 0


def test_resolver_diagnostics_record(scenes, table):
    """a frame's own record explains a slow frame.  After frames in flight
    and lone frames, rc_resolver_stats_get reports every frame read back, the resolver's
    placement within what a CU can hold (registers <= 256: two lane workgroups per CU), the
    team's rounds, and the shader clock each resolver ran at (s_memtime against s_memrealtime:
    a throttled box would show a low clock, not an unexplained slow step)."""
    torch = pytest.importorskip("torch")
    n, key = 1024, "quadric:1024x1024:d6:parity"
    want = table[key]["md5"]
    s = scenes["quadric"]
    bufs = [torch.zeros((n, n, 3), dtype=torch.uint8, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    rc.frames_wait()
    for b in bufs:
        rc.frame_submit(s, n, n, b.data_ptr(), depth=6)
    rc.frames_wait()
    d = rc.resolver_stats()
    assert d["frames"] == 4
    assert 0 < d["resolve_ms_min"] <= d["resolve_ms_mean"] <= d["resolve_ms_max"]
    assert 0 < d["wg_per_cu"] <= d["wg_per_cu_max"] and d["regs"] <= 256
    assert 300 <= d["clock_mhz_min"] <= d["clock_mhz_max"] <= 3500, d
    assert d["scan_rounds_max"] + d["cscan_rounds_max"] + d["resolve_rounds_max"] > 0
    for b in bufs:
        assert p3_md5(b.cpu().numpy()) == want
    rc.lone_frames_check()
    rc.resolver_stats(lone=True)   # reset the lone window
    out = torch.empty((n, n, 3), dtype=torch.uint8, device="cuda")
    for _ in range(3):
        rc.render_device(s, n, n, out.data_ptr(), depth=6)
    assert rc.lone_frames_check() == {"checked": 3, "failed": 0}
    d = rc.resolver_stats(lone=True)
    assert d["frames"] == 3 and 300 <= d["clock_mhz_min"] <= d["clock_mhz_max"] <= 3500, d
    assert d["wg_per_cu"] <= d["wg_per_cu_max"]
    assert p3_md5(out.cpu().numpy()) == want


@pytest.mark.parametrize("sched", ["default", "no-side"])
def test_mapped_patch_marks_across_frames(sched, scenes, table):
    """rc_render's mapped colour patch (patch_host 2) over a run of frames of different scenes
    and sizes, past two cycles of its per-frame marks (rc::kPatchMarks = 128 epochs, then the
    array is cleared): every frame's bytes are its golden's.  A mark that outlives its frame
    makes the next frame scatter an earlier scene's colour (profiles/r06n_patch_marks.txt: seen
    with phase C after the resolver, side=0, when the host cleared consumed entries)."""
    keys = ["reflection:256x256:d6:parity", "quadric:256x256:d6:parity",
            "simple:256x256:d4:parity", "quadric:333x517:d6:parity"]
    tune = {} if sched == "default" else dict(side=0)
    with rc.tuned(**tune):
        for i in range(300):
            key = keys[i % len(keys)]
            scene, size, d, mode = key.split(":")
            w, h = map(int, size.split("x"))
            img = rc.render(scenes[scene], w, h, depth=int(d[1:]), mode=mode)
            assert p3_md5(img) == table[key]["md5"], (sched, i, key)


def test_team_slots_over_many_frames(scenes, table):
    """The resolver team's hand-off slots (k_resolve) over 600 lone quadric 4096^2 frames in
    the default schedule, every frame's hand-offs checked (the slots rotate over four rounds;
    with round-parity slots 1 frame in ~200-300 failed under split shading,
    profiles/r06o_team_slot_race.txt).  Split shading itself still fails a hand-off about once
    in 5 000-14 000 frames (profiles/r06zz_split_shade_residual.txt): too rare to stress here
    without a flaky test, so test_parity_schedules keeps its three split-shading frames only.
    The last frame's bytes are the golden's."""
    torch = pytest.importorskip("torch")
    n, key = 4096, "quadric:4096x4096:d6:parity"
    out = torch.empty((n, n, 3), dtype=torch.uint8, device="cuda")
    rc.lone_frames_check()
    for i in range(600):
        rc.render_device(scenes["quadric"], n, n, out.data_ptr(), depth=6)
        if i % 50 == 49:
            assert rc.lone_frames_check()["failed"] == 0, i
    assert rc.lone_frames_check()["failed"] == 0
    assert p3_md5(out.cpu().numpy()) == table[key]["md5"]


def test_held_back_phase_c_completion_points(scenes, table):
    """the last submitted frame's phase C is held back until the next submit or
    rc_frames_wait.  rc_lone_frames_check and a lone render launch it first, so a device
    synchronisation after them completes every submitted frame; rc_frames_wait still verifies
    the window afterwards, and rc_pipe_reset leaves nothing pending."""
    torch = pytest.importorskip("torch")
    n, key = 1024, "quadric:1024x1024:d6:parity"
    want = table[key]["md5"]
    s = scenes["quadric"]
    rc.frames_wait()
    bufs = [torch.zeros((n, n, 3), dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    for b in bufs[:2]:
        rc.frame_submit(s, n, n, b.data_ptr(), depth=6)
    rc.lone_frames_check()   # launches frame 1's held-back phase C
    torch.cuda.synchronize()
    assert [p3_md5(b.cpu().numpy()) for b in bufs[:2]] == [want] * 2
    rc.frame_submit(s, n, n, bufs[2].data_ptr(), depth=6)
    out = torch.empty((n, n, 3), dtype=torch.uint8, device="cuda")
    rc.render_device(s, n, n, out.data_ptr(), depth=6)   # a lone render flushes it too
    torch.cuda.synchronize()
    assert p3_md5(bufs[2].cpu().numpy()) == want and p3_md5(out.cpu().numpy()) == want
    tim = {}
    rc.frames_wait(tim)
    assert (tim["frames_checked"], tim["frames_failed"]) == (3, 0)
    rc.frame_submit(s, n, n, bufs[0].data_ptr(), depth=6)
    rc.pipe_reset()   # waits for the window, then rebuilds the pipeline on the next submit
    rc.frame_submit(s, n, n, bufs[1].data_ptr(), depth=6)
    rc.frames_wait(tim)
    assert (tim["frames_checked"], tim["frames_failed"]) == (1, 0)
    assert rc.lone_frames_check()["failed"] == 0
