"""Accumulation through a free camera: the inputs and the expectation that tests/test_camera_accum.py
(no GPU) and tests/test_gpu_camera_accum.py share.  A sample of a pass is a pixel of
the image rc_render_camera defines, so the expectation is ray_cases.camera_samples, sliced at the
lattice point, and the pass itself is rc.accum_add.  References are computed once per key
(camera_samples keeps them) and are read-only."""
import numpy as np

import ray_cases as rcs
from helpers import rc

DEPTH = rcs.DEPTH
FULL = rcs.SIZE                                   # 64 x 48
WINDOW, SIZE = (*FULL, 5, 3), (33, 17)            # odd origin; crosses tile and wave edges
CORNER, CORNER_SIZE = (*FULL, FULL[0] - 7, FULL[1] - 3), (7, 3)   # the image's bottom-right corner
G, HIER4 = rc.SAMPLE_SEQS["hier4"]
PREFIXES = (1, 3, 5, 16)                          # hier4[0..1), [0..3), [0..5), [0..16)

# ray_cases.CAMERAS: the eye inside a sphere, the turned eye inside the quadric, the eye -0
DENSE = [rcs.CAMERAS[1], rcs.CAMERAS[11], rcs.CAMERAS[7]]
assert DENSE[0][1] == (0.0, -4.0, -12.5) and DENSE[1][1] == (2.0, 3.0, -8.0)
assert all(np.signbit(v) for v in DENSE[2][1])

# the lens: 16 points of a disc, the centre first, then a sunflower spiral out to the radius
LENS_SCENE, LENS_EYE, LENS_RADIUS, LENS_FOCUS = "quadric", (0.5, 0.25, 1.0), 0.3, 8.0


def lens_points(n, radius=LENS_RADIUS):
    k = np.arange(n, dtype=np.float64)
    r = radius * np.sqrt(k / max(n - 1, 1))
    a = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1)


LENS = rc.thin_lens(LENS_EYE, None, LENS_FOCUS, lens_points(16))
MASKED = rcs.CAMERAS[8]                           # quadric, eye (0.5, 0.25, 1.0): the masked pass's
MASK_T = 16


def lit_unstaged_scene():
    """"quadric40": the quadric example's shapes and lights with 35 small spheres in front of them,
    40 shapes, more than the kernels stage in LDS.  The 65-shape scene of tests/test_gpu_camera.py
    is black from every eye (its two lights reach nothing), so a masked pass over it lists nothing;
    this one has edges.  Registered with ray_cases.scene."""
    name = "quadric40"
    if name not in rcs._scenes:
        import shade_cases as shc
        from helpers import scene_path
        rng = np.random.default_rng(40)
        lines = open(scene_path("quadric")).read().splitlines()
        for _ in range(35):
            x, y, z = rng.uniform(-3, 3), rng.uniform(-0.5, 2.5), rng.uniform(-9, -5)
            r, gr, b = rng.uniform(0.2, 1.0, 3)
            lines.append(f"sphere, diffuse_color: [{r:.3f}, {gr:.3f}, {b:.3f}], specular_color: "
                         f"[0.5, 0.5, 0.5], position: [{x:.3f}, {y:.3f}, {z:.3f}], radius: "
                         f"{rng.uniform(0.1, 0.3):.3f}, reflectivity: {rng.uniform(0.0, 0.4):.2f}, refractivity: 0, ior: 2")
        rcs._scenes[name] = shc._text_scene(name, "\n".join(lines) + "\n")
    return name


def plane(name, eye, m, point, size=SIZE, window=WINDOW, g=G):
    """The [h, w, 3] plane of lattice point (x, y) through the camera (eye, m): that point's slice
    of the oracle's g*w x g*h samples of the window."""
    x, y = point
    return rcs.camera_samples(name, tuple(float(v) for v in eye), m, g, size, window)[0][y::g, x::g]


def planes(name, cams, points, size=SIZE, window=WINDOW, g=G):
    """[count, h, w, 3]: sample j of a pass takes lattice point points[j] through cams[j] (one
    camera: through it for every j)."""
    cams = list(cams) if len(cams) == len(points) else [cams[0]] * len(points)
    return np.stack([plane(name, e, m, p, size, window, g) for (e, m), p in zip(cams, points)])


def run_prefixes(name, eye, m, size=SIZE, window=WINDOW):
    """The states after the t = 0 passes hier4[0..1), [1..3), [3..5), [5..16), the first one
    resetting: [(first, count, acc, out), ...]."""
    h, w = size[1], size[0]
    acc, out = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8)
    states, first = [], 0
    for upto in PREFIXES:
        acc, out, _, _ = rc.accum_add(acc, out, planes(name, [(eye, m)], HIER4[first:upto], size,
                                                       window), 0, reset=first == 0)
        states.append((first, upto - first, acc, out))
        first = upto
    return states


def masked_pass():
    """The reset pass hier4[0..1) and the masked pass hier4[1..4) at MASK_T through MASKED:
    (acc0, out0, acc1, out1, active)."""
    name, eye, m = MASKED
    h, w = SIZE[1], SIZE[0]
    zero = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8)
    acc0, out0, _, _ = rc.accum_add(*zero, planes(name, [(eye, m)], HIER4[:1]), 0, reset=True)
    acc1, out1, active, sat = rc.accum_add(acc0, out0, planes(name, [(eye, m)], HIER4[1:4]),
                                           MASK_T)
    assert sat == 0
    return acc0, out0, acc1, out1, active
