"""Sparse sample patterns on the GPU (rc_render_pattern): every output byte is
rc.pattern_downsample of the CPU oracle's own g*W x g*H image, composed with its W x H image by
rc.adaptive_compose when a threshold is given: no tolerance anywhere."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, oracle_render, oracle_render_cuda, rc, read_p3, scene_path

pytestmark = pytest.mark.gpu

SCENES = ["simple", "reflection", "quadric"]
SIZES = [(1, 1), (7, 3), (33, 17), (64, 48)]   # partial tiles; at n = 16 a pixel is a quarter wave
CUSTOM = {"asym2": (8, [(7, 0), (1, 3)]),
          "cust16": (8, [((5 * k + 3) % 8, k // 2) for k in range(16)])}
PATTERNS = dict(rc.PATTERNS, **CUSTOM)
# transpose-symmetric by construction: exempt from the transpose assertion only
SYMMETRIC = ("diag2", "checker8")


@pytest.fixture(scope="module")
def scenes():
    return {n: rc.Scene.from_file(scene_path(n)) for n in SCENES}


_oracle = {}


def oracle_image(scenes, name, w, h, depth, mode):
    """The oracle's w x h image and its zero-normalize count (None in cuda mode, whose oracle
    keeps none): computed once per key, read-only."""
    key = (name, w, h, depth, mode)
    if key not in _oracle:
        if mode == "cuda":
            img, zn = oracle_render_cuda(scenes[name], w, h, depth), None
        else:
            img, stats = oracle_render(scenes[name], w, h, depth, mode)
            assert stats["parity_defined"] == 1, key   # the example scenes are all defined
            zn = stats["zero_normalize"]
        img.setflags(write=False)
        _oracle[key] = (img, zn)
    return _oracle[key]


_expected = {}


def expected(scenes, name, pat, w, h, depth, mode):
    """(A, P, zero-normalize events of A, of B_g) from the oracle for the pattern named `pat`.
    Before anything touches the GPU: P is not what a swapped x / y, the full grid or one ray
    would give (sizes of more than one pixel a side)."""
    key = (name, pat, w, h, depth, mode)
    if key not in _expected:
        g, pts = PATTERNS[pat]
        a, za = oracle_image(scenes, name, w, h, depth, mode)
        big, zb = oracle_image(scenes, name, g * w, g * h, depth, mode)
        p = rc.pattern_downsample(big, g, pts)
        p.setflags(write=False)
        if min(w, h) > 1:
            if pat not in SYMMETRIC:
                swapped = rc.pattern_downsample(big, g, [(y, x) for x, y in pts])
                assert (p != swapped).any(), key
            assert (p != rc.box_downsample(big, g)).any(), key
            assert (p != a).any(), key
        _expected[key] = (a, p, za, zb)
    return _expected[key]


@pytest.mark.parametrize("depth", [0, 6])
@pytest.mark.parametrize("scene", SCENES)
def test_dense_fast_vs_oracle(scene, depth, scenes):
    for w, h in SIZES:
        for pat in PATTERNS:
            _, want, _, zb = expected(scenes, scene, pat, w, h, depth, "fast")
            tim = {}
            got = rc.render_pattern(scenes[scene], w, h, PATTERNS[pat], depth=depth, mode="fast",
                                    timing=tim)
            tag = f"{scene} {pat} {w}x{h} d{depth}"
            np.testing.assert_array_equal(got, want, err_msg=tag)
            n = len(PATTERNS[pat][1])
            assert rc.pattern_stats() == {"refined_pixels": w * h, "rays": n * w * h}, tag
            assert 0 <= tim["zero_normalize"] <= zb, tag   # the rays shot are some of B_g's
            assert tim["kernel_ms"] > 0.0, tag


@pytest.mark.parametrize("scene", SCENES)
def test_dense_cuda_vs_oracle(scene, scenes):
    for w, h in ((7, 3), (64, 48)):
        for pat in ("rgss4", "queens8", "asym2"):
            _, want, _, _ = expected(scenes, scene, pat, w, h, 50, "cuda")
            got = rc.render_pattern(scenes[scene], w, h, PATTERNS[pat], depth=50, mode="cuda")
            np.testing.assert_array_equal(got, want, err_msg=f"{scene} {pat} {w}x{h}")


@pytest.mark.parametrize("g", [2, 4])
def test_full_pattern_is_plain_ssaa(g, scenes):
    """On the GPU alone: every lattice point once is rc_options.ssaa = g, bytes and counts."""
    full = (g, [(i, j) for j in range(g) for i in range(g)])
    for name in SCENES:
        for w, h in SIZES:
            ts, tp = {}, {}
            want = rc.render(scenes[name], w, h, depth=6, mode="fast", ssaa=g, timing=ts)
            got = rc.render_pattern(scenes[name], w, h, full, depth=6, mode="fast", timing=tp)
            np.testing.assert_array_equal(got, want, err_msg=f"{name} {w}x{h} g{g}")
            assert tp["zero_normalize"] == ts["zero_normalize"], (name, w, h, g)
    want = rc.render(scenes["quadric"], 33, 17, depth=50, mode="cuda", ssaa=g)
    got = rc.render_pattern(scenes["quadric"], 33, 17, full, depth=50, mode="cuda")
    np.testing.assert_array_equal(got, want)


def check_adaptive(scenes, name, pat, w, h, t, depth, mode):
    a, p, za, zb = expected(scenes, name, pat, w, h, depth, mode)
    want = rc.adaptive_compose(a, p, t)
    tim = {}
    got = rc.render_pattern(scenes[name], w, h, PATTERNS[pat], threshold=t, depth=depth,
                            mode=mode, timing=tim)
    tag = f"{name} {pat} {w}x{h} t{t} {mode}"
    np.testing.assert_array_equal(got, want, err_msg=tag)
    st = rc.pattern_stats()
    flagged = int(rc.edge_mask(a, t).sum())
    assert st["refined_pixels"] == flagged, tag
    assert st["rays"] == w * h + len(PATTERNS[pat][1]) * flagged, tag
    if mode == "fast":
        assert za <= tim["zero_normalize"] <= za + zb, tag
    return a, p, want, flagged


def check_adaptive_first(scenes, name, pat, w, h, t, depth, mode):
    """check_adaptive after asserting, on the oracle's images, that the composed image is neither
    A nor P: a build that returns either fails."""
    a, p, _, _ = expected(scenes, name, pat, w, h, depth, mode)
    want = rc.adaptive_compose(a, p, t)
    assert (want != a).any() and (want != p).any(), (name, pat, w, h, t, mode)
    return check_adaptive(scenes, name, pat, w, h, t, depth, mode)


@pytest.mark.parametrize("scene", SCENES)
def test_adaptive_vs_oracle(scene, scenes):
    for w, h in ((33, 17), (64, 48)):
        for pat in ("rgss4", "queens8", "asym2"):
            check_adaptive_first(scenes, scene, pat, w, h, 32, 6, "fast")
    for pat in ("rgss4", "queens8", "asym2"):
        check_adaptive_first(scenes, scene, pat, 64, 48, 32, 50, "cuda")


def test_adaptive_list_ends(scenes):
    # an empty list: the one-ray image
    a, p, want, flagged = check_adaptive(scenes, "simple", "rgss4", 7, 3, 255, 6, "fast")
    assert flagged == 0 and (want == a).all() and (want != p).any()
    # every pixel listed: the pattern image
    a, p, want, flagged = check_adaptive(scenes, "quadric", "rgss4", 7, 3, 1, 6, "fast")
    assert flagged == 21 and (want == p).all() and (want != a).any()
    for pat in ("diag2", "cust16"):   # 32 and 4 pixels a wave step: 21 is a partly filled step
        check_adaptive(scenes, "quadric", pat, 7, 3, 1, 6, "fast")


def test_adaptive_stride_loop_and_repeat(scenes):
    sc = scenes["quadric"]
    for pat in ("rgss4", "queens8", "cust16"):
        _, _, want, flagged = check_adaptive(scenes, "quadric", pat, 64, 48, 32, 6, "fast")
        assert flagged > 64   # more than one wave step of one workgroup at any n
        with rc.tuned(adaptive_blocks=1):   # four waves stride over the whole list
            one = rc.render_pattern(sc, 64, 48, PATTERNS[pat], threshold=32, depth=6, mode="fast")
            assert rc.pattern_stats()["refined_pixels"] == flagged
        np.testing.assert_array_equal(one, want)
        again = rc.render_pattern(sc, 64, 48, PATTERNS[pat], threshold=32, depth=6, mode="fast")
        np.testing.assert_array_equal(again, want)   # the list's order differs, the bytes do not


@pytest.mark.parametrize("pat", ["diag2", "rgss4", "cust16"])
def test_larger_image(pat, scenes):
    """Hundreds of tiles (more than 64, where a build with the XCD-chunked tile order starts to
    permute them) and odd sizes; with two workgroups a list much longer than the grid."""
    w, h, t = 257, 129, 16
    _, want, _, _ = expected(scenes, "quadric", pat, w, h, 6, "fast")
    got = rc.render_pattern(scenes["quadric"], w, h, PATTERNS[pat], depth=6, mode="fast")
    np.testing.assert_array_equal(got, want)
    _, _, composed, flagged = check_adaptive(scenes, "quadric", pat, w, h, t, 6, "fast")
    assert flagged > 1024
    with rc.tuned(adaptive_blocks=2):   # 8 waves stride over the whole list
        got = rc.render_pattern(scenes["quadric"], w, h, PATTERNS[pat], threshold=t, depth=6,
                                mode="fast")
    np.testing.assert_array_equal(got, composed)


def test_device_entry_on_a_torch_stream(scenes):
    torch = pytest.importorskip("torch")
    sc = scenes["quadric"]
    a, p, _, _ = expected(scenes, "quadric", "queens8", 64, 48, 6, "fast")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dense = torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda")
        listed = torch.zeros((48, 64, 3), dtype=torch.uint8, device="cuda")
        rc.render_pattern_device(sc, 64, 48, "queens8", dense.data_ptr(),
                                 stream_ptr=stream.cuda_stream, depth=6, mode="fast")
        rc.render_pattern_device(sc, 64, 48, "queens8", listed.data_ptr(), threshold=32,
                                 stream_ptr=stream.cuda_stream, depth=6, mode="fast")
    stream.synchronize()
    np.testing.assert_array_equal(dense.cpu().numpy(), p)
    np.testing.assert_array_equal(listed.cpu().numpy(), rc.adaptive_compose(a, p, 32))
    # with a timing record the call waits, and the spans add up to its kernel time
    tim = {}
    rc.render_pattern_device(sc, 64, 48, "queens8", dense.data_ptr(), depth=6, mode="fast",
                             timing=tim)
    ms = rc.pattern_phase_ms()
    assert sorted(ms) == ["mark", "refine", "render"]
    assert ms["render"] > 0.0 and ms["mark"] == 0.0 and ms["refine"] == 0.0
    assert ms["render"] == pytest.approx(tim["kernel_ms"], rel=1e-3)
    rc.render_pattern_device(sc, 64, 48, "queens8", listed.data_ptr(), threshold=32, depth=6,
                             mode="fast", timing=tim)
    ms = rc.pattern_phase_ms()
    assert all(ms[k] > 0.0 for k in ("render", "mark", "refine"))
    assert ms["render"] + ms["mark"] + ms["refine"] == pytest.approx(tim["kernel_ms"], rel=1e-3)
    np.testing.assert_array_equal(listed.cpu().numpy(), rc.adaptive_compose(a, p, 32))


def test_refusals_leave_the_device_usable(scenes):
    torch = pytest.importorskip("torch")
    sc = scenes["simple"]
    out = torch.zeros((8, 8, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    host = np.zeros((8, 8, 3), dtype=np.uint8)
    refused = [dict(mode="parity"),                                   # parity mode
               dict(pat=(4, [(1, 0), (3, 1), (1, 0), (2, 3)])),      # fails the check
               dict(threshold=256), dict(threshold=-1),              # the threshold
               dict(w=(1 << 26) + 1), dict(h=(1 << 26) + 1),         # above 2^28 / g
               dict(w=1 << 16, h=1 << 16, threshold=16)]             # W * H >= 2^32 with t > 0
    for kw in refused:
        w, h = kw.get("w", 8), kw.get("h", 8)
        p = rc.RcPattern()
        g, pts = kw.get("pat", rc.PATTERNS["rgss4"])
        p.grid, p.nsamples = g, len(pts)
        for k, (x, y) in enumerate(pts):
            p.x[k], p.y[k] = x, y
        opt = rc.options(6, kw.get("mode", "fast"))
        assert rc.hip_lib().rc_render_pattern_device(
            sc.packed(), w, h, ctypes.byref(opt), ctypes.byref(p), kw.get("threshold", 0),
            out.data_ptr(), None, None) == -1, kw
        assert rc.hip_lib().rc_render_pattern(
            sc.packed(), w, h, ctypes.byref(opt), ctypes.byref(p), kw.get("threshold", 0),
            host.ctypes.data_as(ctypes.c_void_p), None) == -1, kw
    for bad in (dict(ssaa=2), dict(ssaa=4, adaptive=16), dict(gpus=2)):   # the options
        opt = rc.options(6, "fast", **bad)
        p = rc.RcPattern()
        assert rc.hip_lib().rc_pattern_builtin(b"rgss4", ctypes.byref(p)) == 0
        assert rc.hip_lib().rc_render_pattern_device(
            sc.packed(), 8, 8, ctypes.byref(opt), ctypes.byref(p), 0, out.data_ptr(), None,
            None) == -1, bad
    assert not host.any() and not out.cpu().numpy().any()
    # a refusal leaves the device usable
    a, p, _, _ = expected(scenes, "simple", "rgss4", 8, 8, 6, "fast")
    np.testing.assert_array_equal(rc.render_pattern(sc, 8, 8, "rgss4", depth=6, mode="fast"), p)
    np.testing.assert_array_equal(
        rc.render_pattern(sc, 8, 8, "rgss4", threshold=16, depth=6, mode="fast"),
        rc.adaptive_compose(a, p, 16))
    np.testing.assert_array_equal(rc.render(sc, 8, 8, mode="fast"), a)


def test_cli_env(tmp_path, scenes):
    """RAYCAST_PATTERN reaches the kernels through raycast(): the drop-in CLI's file is the
    pattern image and its timing line keeps its form."""
    a, p, _, _ = expected(scenes, "quadric", "rgss4", 64, 48, 6, "fast")
    exe = os.path.join(ROOT, "raytracing-programs_amd", "bin", "raytrace")
    out = tmp_path / "pat.ppm"
    env = dict(os.environ, RAYCAST_PATTERN="rgss4:32", RAYCAST_MODE="fast")
    for name in ("RAYCAST_DEPTH", "RAYCAST_SSAA", "RAYCAST_SSAA_ADAPTIVE", "RAYCAST_FILTER"):
        env.pop(name, None)
    r = subprocess.run([exe, "64", "48", scene_path("quadric"), str(out)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(read_p3(str(out)), rc.adaptive_compose(a, p, 32))
    assert r.stdout.startswith("Time (sec) to create a 64x48 image with 5 shape(s) and "
                               "2 light(s): ")
    assert r.stdout.count("\n") == 1
