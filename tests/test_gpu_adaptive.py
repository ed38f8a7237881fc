"""Adaptive supersampling on the GPU (rc_options.ssaa = RC_SSAA_ADAPTIVE(s, t)): every output
byte is rc.adaptive_compose of two images of the CPU oracle, its W x H image A and the box filter
F of its s*W x s*H image: no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

from helpers import (ROOT, oracle_render, oracle_render_cuda, random_scene, rc, read_p3,
                     scene_path)

pytestmark = pytest.mark.gpu

SCENES = ["simple", "reflection", "quadric"]
SIZES = [(1, 1), (7, 3), (33, 17), (64, 48)]   # one pixel; partial tiles; a partly filled wave
THRESHOLDS = [1, 16, 64, 255]


@pytest.fixture(scope="module")
def scenes():
    return {n: rc.Scene.from_file(scene_path(n)) for n in SCENES}


_oracle = {}


def oracle_image(sc, key, w, h, depth, mode):
    """The oracle's w x h image and its zero-normalize count (None in cuda mode, whose oracle
    keeps none): computed once per key, read-only."""
    key = (key, w, h, depth, mode)
    if key not in _oracle:
        if mode == "cuda":
            img, zn = oracle_render_cuda(sc, w, h, depth), None
        else:
            img, stats = oracle_render(sc, w, h, depth, mode)
            assert stats["parity_defined"] == 1, key   # the example scenes are all defined
            zn = stats["zero_normalize"]
        img.setflags(write=False)
        _oracle[key] = (img, zn)
    return _oracle[key]


_af = {}


def images(scenes, name, w, h, s, depth, mode):
    """(A, F, zero-normalize events of A, of B) from the oracle."""
    key = (name, w, h, s, depth, mode)
    if key not in _af:
        a, za = oracle_image(scenes[name], name, w, h, depth, mode)
        big, zb = oracle_image(scenes[name], name, s * w, s * h, depth, mode)
        f = rc.box_downsample(big, s)
        f.setflags(write=False)
        _af[key] = (a, f, za, zb)
    return _af[key]


def check_fast(scenes, name, w, h, s, t, depth):
    a, f, za, zb = images(scenes, name, w, h, s, depth, "fast")
    want = rc.adaptive_compose(a, f, t)
    tim = {}
    got = rc.render(scenes[name], w, h, depth=depth, mode="fast", ssaa=s, adaptive=t, timing=tim)
    tag = f"{name} {w}x{h} s{s} t{t} d{depth}"
    np.testing.assert_array_equal(got, want, err_msg=tag)
    st = rc.adaptive_stats()
    flagged = int(rc.edge_mask(a, t).sum())
    assert st["refined_pixels"] == flagged, tag
    assert st["rays"] == w * h + s * s * flagged, tag
    assert za <= tim["zero_normalize"] <= za + zb, tag
    return a, f, want, flagged


@pytest.mark.parametrize("s", [2, 4, 8])
@pytest.mark.parametrize("scene", SCENES)
def test_fast_vs_oracle(scene, s, scenes):
    for w, h in SIZES:
        for t in THRESHOLDS:
            a, f, want, flagged = check_fast(scenes, scene, w, h, s, t, 6)
            if (w, h) == (1, 1):
                # nothing is flagged: the one-ray image, which is not the supersampled one
                assert flagged == 0 and (want == a).all() and (want != f).any()
            if t == 64 and (w, h) in ((33, 17), (64, 48)):
                # a build that returns either image fails
                assert (want != a).any() and (want != f).any(), (scene, w, h, s)
            if t == 1 and (w, h) == (64, 48):
                # many pixels, and not a whole number of waves' worth
                assert flagged > 1000 and flagged % 16 != 0, (scene, s, flagged)


@pytest.mark.parametrize("scene", SCENES)
def test_fast_depth0_vs_oracle(scene, scenes):
    for w, h in SIZES:
        check_fast(scenes, scene, w, h, 4, 16, 0)


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("scene", SCENES)
def test_cuda_vs_oracle(scene, s, scenes):
    for w, h in ((7, 3), (64, 48)):
        a, f, _, _ = images(scenes, scene, w, h, s, 50, "cuda")
        for t in (16, 64):
            got = rc.render(scenes[scene], w, h, depth=50, mode="cuda", ssaa=s, adaptive=t)
            np.testing.assert_array_equal(got, rc.adaptive_compose(a, f, t),
                                          err_msg=f"{scene} {w}x{h} s{s} t{t}")
            st = rc.adaptive_stats()
            assert st["refined_pixels"] == int(rc.edge_mask(a, t).sum())


def test_random_cross_term_scene(tmp_path):
    """14 shapes with cross-term quadrics: the general quadric form and a scene other than the
    examples."""
    rng = np.random.default_rng(1407)
    path = str(tmp_path / "r14.scene")
    random_scene(rng, path, 14, 2, cross=True)
    sc = rc.Scene.from_file(path)
    w, h = 33, 17
    a, stats = oracle_render(sc, w, h, 6, "fast")
    if stats["parity_defined"] == 0:
        pytest.skip("the reference reads undefined memory for this scene")
    for s in (2, 8):
        big, _ = oracle_render(sc, s * w, s * h, 6, "fast")
        want = rc.adaptive_compose(a, rc.box_downsample(big, s), 16)
        np.testing.assert_array_equal(
            rc.render(sc, w, h, depth=6, mode="fast", ssaa=s, adaptive=16), want,
            err_msg=f"s{s}")


@pytest.mark.parametrize("s", [2, 8])
def test_larger_image(s, scenes):
    """Many tiles, and with one workgroup-pass of a small grid a list longer than the grid."""
    w, h, t = 257, 129, 16
    a, f, want, flagged = check_fast(scenes, "quadric", w, h, s, t, 6)
    assert flagged > 64
    with rc.tuned(adaptive_blocks=2):   # 8 waves stride over the whole list
        got = rc.render(scenes["quadric"], w, h, depth=6, mode="fast", ssaa=s, adaptive=t)
    np.testing.assert_array_equal(got, want)


def test_stride_loop_one_workgroup(scenes):
    a, f, _, _ = images(scenes, "quadric", 64, 48, 2, 6, "fast")
    want = rc.adaptive_compose(a, f, 1)
    default = rc.render(scenes["quadric"], 64, 48, depth=6, mode="fast", ssaa=2, adaptive=1)
    with rc.tuned(adaptive_blocks=1):
        one = rc.render(scenes["quadric"], 64, 48, depth=6, mode="fast", ssaa=2, adaptive=1)
        assert rc.adaptive_stats()["refined_pixels"] == int(rc.edge_mask(a, 1).sum())
    np.testing.assert_array_equal(one, default)
    np.testing.assert_array_equal(one, want)


@pytest.mark.parametrize("mode,depth", [("fast", 6), ("cuda", 50)])
def test_order_independence_and_gpu_composition(mode, depth, scenes):
    """The list's order differs from run to run; the bytes do not.  And on the GPU alone: the
    adaptive image is the composition of the GPU's own A and F."""
    sc = scenes["reflection"]
    for s, t in ((2, 16), (4, 1)):
        one = rc.render(sc, 64, 48, depth=depth, mode=mode, ssaa=s, adaptive=t)
        two = rc.render(sc, 64, 48, depth=depth, mode=mode, ssaa=s, adaptive=t)
        np.testing.assert_array_equal(one, two)
        a = rc.render(sc, 64, 48, depth=depth, mode=mode)
        f = rc.render(sc, 64, 48, depth=depth, mode=mode, ssaa=s)
        np.testing.assert_array_equal(one, rc.adaptive_compose(a, f, t))


def test_adaptive_off_is_plain_ssaa(scenes):
    _, f, _, zb = images(scenes, "quadric", 33, 17, 4, 6, "fast")
    tim = {}
    got = rc.render(scenes["quadric"], 33, 17, depth=6, mode="fast", ssaa=4, adaptive=0,
                    timing=tim)
    np.testing.assert_array_equal(got, f)
    assert tim["zero_normalize"] == zb
    np.testing.assert_array_equal(
        got, rc.render(scenes["quadric"], 33, 17, depth=6, mode="fast", ssaa=4))


def test_device_render_whole_image(scenes):
    torch = pytest.importorskip("torch")
    a, f, _, _ = images(scenes, "quadric", 64, 48, 2, 6, "fast")
    out = torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tim = {}
    rc.render_device(scenes["quadric"], 64, 48, out.data_ptr(), depth=6, mode="fast", ssaa=2,
                     adaptive=16, timing=tim)
    np.testing.assert_array_equal(out.cpu().numpy(), rc.adaptive_compose(a, f, 16))
    ms = rc.adaptive_phase_ms()
    assert all(ms[k] > 0.0 for k in ("render", "mark", "refine"))
    assert ms["render"] + ms["mark"] + ms["refine"] == pytest.approx(tim["kernel_ms"], rel=1e-3)


def test_frames_in_flight(scenes):
    torch = pytest.importorskip("torch")
    a, f, _, _ = images(scenes, "quadric", 64, 48, 2, 6, "fast")
    want = rc.adaptive_compose(a, f, 16)
    outs = [torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    for o in outs:
        rc.frame_submit(scenes["quadric"], 64, 48, o.data_ptr(), depth=6, mode="fast", ssaa=2,
                        adaptive=16)
    rc.frames_wait()
    for o in outs:
        np.testing.assert_array_equal(o.cpu().numpy(), want)
    assert rc.adaptive_stats()["refined_pixels"] == int(rc.edge_mask(a, 16).sum())


def test_refusals(scenes):
    torch = pytest.importorskip("torch")
    sc = scenes["simple"]
    out = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):   # parity mode
        rc.render(sc, 8, 8, mode="parity", ssaa=2, adaptive=16)
    with pytest.raises(RuntimeError):
        rc.render_device(sc, 8, 8, out.data_ptr(), mode="parity", ssaa=2, adaptive=16)
    with pytest.raises(RuntimeError):
        rc.frame_submit(sc, 8, 8, out.data_ptr(), mode="parity", ssaa=2, adaptive=16)
    rc.frames_wait()
    for rows in (dict(row0=0, row_step=1, nrows=4), dict(row0=1, row_step=1, nrows=7),
                 dict(row0=0, row_step=2, nrows=4)):   # a row subset
        with pytest.raises(RuntimeError):
            rc.render_device(sc, 8, 8, out.data_ptr(), mode="fast", ssaa=2, adaptive=16, **rows)
    for s in (1, 0):   # a threshold without a factor
        with pytest.raises(RuntimeError):
            rc.render(sc, 8, 8, mode="fast", ssaa=s, adaptive=16)
    for bad in (256, -1, 1 << 16):
        with pytest.raises(RuntimeError):
            rc.render(sc, 8, 8, mode="fast", ssaa=2, adaptive=bad)
    with pytest.raises(RuntimeError):   # a factor that is none, with a threshold
        rc.render(sc, 8, 8, mode="fast", ssaa=3, adaptive=16)
    with pytest.raises(RuntimeError):
        rc.frame_submit(sc, 8, 8, out.data_ptr(), mode="fast", ssaa=1, adaptive=16)
    with pytest.raises(RuntimeError):   # the row shards do not supersample
        rc.render(sc, 8, 8, mode="fast", gpus=2, ssaa=2, adaptive=16)
    with rc.tuned(share_device=1):   # two ranks on this device: still refused
        with pytest.raises(RuntimeError):
            rc.render(sc, 8, 8, mode="fast", gpus=2, ssaa=2, adaptive=16)
    # a refusal leaves the device usable
    a = rc.render(sc, 8, 8, mode="fast")
    f = rc.render(sc, 8, 8, mode="fast", ssaa=2)
    np.testing.assert_array_equal(rc.render(sc, 8, 8, mode="fast", ssaa=2, adaptive=16),
                                  rc.adaptive_compose(a, f, 16))
    np.testing.assert_array_equal(a, oracle_render(sc, 8, 8, 6, "fast")[0])


def test_cli_env(tmp_path, scenes):
    """RAYCAST_SSAA_ADAPTIVE reaches the kernels through raycast(): the drop-in CLI's file is the
    adaptive image and its timing line keeps its form."""
    a, f, _, _ = images(scenes, "quadric", 64, 48, 2, 6, "fast")
    exe = os.path.join(ROOT, "raytracing-programs_amd", "bin", "raytrace")
    out = tmp_path / "aa.ppm"
    env = dict(os.environ, RAYCAST_SSAA="2", RAYCAST_SSAA_ADAPTIVE="16", RAYCAST_MODE="fast")
    env.pop("RAYCAST_DEPTH", None)
    r = subprocess.run([exe, "64", "48", scene_path("quadric"), str(out)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(read_p3(str(out)), rc.adaptive_compose(a, f, 16))
    assert r.stdout.startswith("Time (sec) to create a 64x48 image with 5 shape(s) and "
                               "2 light(s): ")
    assert r.stdout.count("\n") == 1
