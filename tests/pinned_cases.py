"""Scenes, images and the wave census shared by tests/test_pinned_cases.py (CPU) and
tests/test_gpu_pinned.py: phase C's carry-point table."""
import ctypes

import numpy as np

import prim_cases as pc
import shade_cases as sc
from helpers import PHANTOM_LIT, QUADRIC_POINT_LIGHT, oracle_render, rc, scene_path

F32 = np.float32
CHUNK = 1024          # k_dep_chunks' entries per workgroup trip (RC_CHUNK)
PIN_SHAPES, PIN_LIGHTS = 8, 16   # RC_PIN_SHAPES, RC_PIN_LIGHTS (rc_scene.h)

# the image-level cases: (scene, W, H), all at depth 6
IMAGES = [("quadric", 256, 256), ("quadric", 64, 64), ("quadric", 7, 3), ("quadric", 1, 4096),
          ("quadric", 333, 517), ("quadric2", 256, 256), ("simple", 256, 256),
          ("reflection", 256, 256)]


def text_scene(name, text):
    return sc._text_scene("pinned_" + name, text)


def _quadric_lines():
    lines = open(scene_path("quadric")).read().splitlines()
    return [ln for ln in lines if not ln.startswith("light")], [ln for ln in lines if ln.startswith("light")]


def _f(v):
    return repr(float(F32(v)))   # a decimal that reads back as the same float


def LIGHT_ROWS(a, b):
    """The quadric example with a point light exactly on a and a spot light exactly on b, ahead of
    its own two lights (the phantom is made of the last lights' bytes: it stays the example's)."""
    shapes, lights = _quadric_lines()
    new = [f"light, color: [3, 2, 1], radial-a2: 0.01, radial-a1: 0.0125, radial-a0: 0.0125, "
           f"position: [{_f(a[0])}, {_f(a[1])}, {_f(a[2])}]",
           f"light, color: [1, 2, 3], radial-a2: 0.01, radial-a1: 0.0125, radial-a0: 0.0125, "
           f"position: [{_f(b[0])}, {_f(b[1])}, {_f(b[2])}], theta: 80, angular-a0: 2, direction: [0, 0, -1]"]
    return "\n".join(shapes[:1] + new + shapes[1:] + lights) + "\n"


# a sphere whose centre and an ellipsoid whose centre (2, 0.5, -6: the gradient vanishes) serve as
# carry points with a zero-length normal; the quadric example's lights
SHAPE_ROWS = "\n".join([
    "camera, width: 2, height: 2",
    "sphere, diffuse_color: [0.25, 0.25, 1], specular_color: [1, 1, 1], position: [0, 0, -5], radius: 1.5, "
    "reflectivity: 0.3, refractivity: 0, ior: 2",
    "quadric, diffuse_color: [0, 0.5, 1.0], specular_color: [0.5, 0.5, 0.5], a: 1, b: 1, c: 1, d: 0, e: 0, "
    "f: 0, g: -4, h: -1, i: 12, j: 39.25, reflectivity: 0.4",
    "plane, normal: [0, 1, 0], diffuse_color: [0.3, 0.3, 0.3], position: [0, -3, 0], reflectivity: 0.0",
    _quadric_lines()[1][0], _quadric_lines()[1][1]]) + "\n"


def big_scene(label, n, m):
    """The quadric example grown to n shapes (small spheres behind the camera's view) and m lights
    (dim point lights ahead of its own two)."""
    shapes, lights = _quadric_lines()
    assert n >= len(shapes) - 1 and m >= len(lights)
    extra_s = [f"sphere, diffuse_color: [0.5, 0.5, 0.5], specular_color: [0.2, 0.2, 0.2], position: "
               f"[{30 + 3 * k}, 40, 30], radius: 1, reflectivity: 0.1, refractivity: 0, ior: 1.5"
               for k in range(n - (len(shapes) - 1))]
    extra_l = [f"light, color: [0.3, 0.2, 0.1], radial-a2: 0.01, radial-a1: 0.0125, radial-a0: 0.0125, "
               f"position: [{-6 + 2 * k}, 8, -3]" for k in range(m - len(lights))]
    return text_scene(f"big_{label}", "\n".join(shapes + extra_s + extra_l + lights) + "\n")


def lit_phantom_scene():
    """The quadric example with a lit phantom (helpers.PHANTOM_LIT): not dep_fast, since a clean
    entry's levels then shade to more than zero."""
    text = open(scene_path("quadric")).read().rstrip("\n")
    assert QUADRIC_POINT_LIGHT in text
    return text_scene("lit_phantom", text.replace(QUADRIC_POINT_LIGHT, PHANTOM_LIT["two-lights"]) + "\n")


class _Header(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("n", "m")] + [("cam_w", ctypes.c_float), ("cam_h", ctypes.c_float)] + \
               [(n, ctypes.c_int32) for n in ("off_shapes", "off_lights", "off_pairs", "bytes",
                                               "phantom_defined", "o0_ok")]


def scene_facts(scene):
    """(n, m, dep_fast, fits) of a scene as upload_scene (rc_api.hip) derives them from the packed
    image: rc_pack_scene on the host, no device."""
    lib = rc.hip_lib()
    lib.rc_pack_scene.restype = ctypes.c_void_p
    lib.rc_pack_scene.argtypes = [ctypes.c_void_p]
    p = lib.rc_pack_scene(ctypes.addressof(scene.js))
    assert p
    h = _Header.from_address(p)
    rec = np.ctypeslib.as_array((ctypes.c_float * (32 * (h.n + 1))).from_address(p + h.off_shapes))
    rec = rec.reshape(h.n + 1, 32)            # 128-byte shape records: refl at word 1, opacity at 2
    dep_fast = bool(not rec[h.n, 2] > 0.0) and bool((np.abs(rec[:h.n, 1]) < 1.0e5).all())
    fits = 1 <= h.n <= PIN_SHAPES and h.m <= PIN_LIGHTS and h.n * h.m <= 64
    out = (int(h.n), int(h.m), dep_fast, fits)
    ctypes.CDLL(None).free(ctypes.c_void_p(p))
    return out


def wave_census(scene, W, H, depth=6):
    """(uniform, mixed) waves of k_dep_chunks' second pass over the image: the DEP entries in scan
    order in chunks of CHUNK, each chunk's entries that hit at their carry-in compacted batch by
    batch (on the device the batches of a chunk may land in another order: the list order is
    free), the list cut into waves of 64; uniform = one carry-in, bit for bit, in every lane."""
    d = pc.primary_dirs(scene.js.camera_width, scene.js.camera_height, W, H)
    _, _, cin = oracle_render(scene, W, H, depth, "parity", with_carry=True)
    cin = np.ascontiguousarray(cin.reshape(-1, 3))
    _, cls, _, _, _ = sc.ref_shoot(scene.js, d, depth + 1, "parity", cin)
    dep = cls >= 2
    hit = (cls[dep] & 1) != 0
    bits = cin[dep].view(np.uint32)
    uniform = mixed = 0
    for c0 in range(0, len(bits), CHUNK):
        lst = bits[c0:c0 + CHUNK][hit[c0:c0 + CHUNK]]
        for w0 in range(0, len(lst), 64):
            wv = lst[w0:w0 + 64]
            if (wv == wv[0]).all():
                uniform += 1
            else:
                mixed += 1
    return uniform, mixed
