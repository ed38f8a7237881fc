"""Views, expected images and ray lists for tests/test_view.py, tests/test_gpu_view.py and
tests/test_gpu_rays.py.  Every expectation is the CPU oracle's own routine on the
directions of the numpy contract rc.view_dirs: rco_prim_shoot / rco_prim_shoot_cuda for colours,
rco_prim_quant for bytes, rco_prim_nearest for hits.  References are computed once per key and are
read-only."""
import os
import tempfile

import numpy as np

import prim_cases as pc
import shade_cases as sc
from helpers import rc, scene_path

F32 = np.float32
FULL = (97, 61)
DEPTH = 6                 # max_recursion 7 for rco_prim_shoot, max_iter 6 for the cuda export
DEG = np.pi / 180.0

VIEWS = {
    "identity": rc.view_identity(),
    "yaw10": rc.view_euler(10 * DEG, 0.0, 0.0),
    "yaw30": rc.view_euler(30 * DEG, 0.0, 0.0),
    "ypr": rc.view_euler(12 * DEG, -8 * DEG, 10 * DEG),
    "back": np.diag([-1.0, 1.0, -1.0]).astype(F32),      # looks backwards: exact, d.z > 0
    "swap": np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]], F32),
    "wide": np.diag([1.5, 1.0, 1.0]).astype(F32),        # anamorphic: not orthonormal
}
ROTATED = [v for v in VIEWS if v != "identity"]

_TMP = []


_LIGHT = "light, color: [{c}, {c}, {c}], radial-a2: 0.01, radial-a1: 0.0125, radial-a0: 0.0125, "
OWN_SCENES = {
    # A reflective plane at z = +1 facing -z BEHIND the eye, a sphere in front of it and a floor:
    # the backward view's primary rays hit the mirror and bounce forwards (the golden scenes have
    # nothing behind the eye, so their backward view runs no bounce at all).
    "mirror_behind":
        "camera, width: 2.0, height: 2.0\n"
        "plane, normal: [0, 0, -1], diffuse_color: [0.3, 0.5, 0.7], specular_color: [1, 1, 1], "
        "position: [0, 0, 1], reflectivity: 0.8\n"
        "sphere, radius: 1.0, diffuse_color: [0.9, 0.2, 0.2], specular_color: [1, 1, 1], "
        "position: [0.3, -0.2, -4], reflectivity: 0.4, refractivity: 0, ior: 1\n"
        "plane, normal: [0, 1, 0], diffuse_color: [0.3, 0.6, 0.3], position: [0, -1.5, 0], "
        "reflectivity: 0.0\n" + _LIGHT.format(c=2) + "position: [1, 3, -2]\n",
    # tests/test_gpu_window.py's zero-normalize scene turned round: a point light exactly on the hit
    # point of the backward view's centre ray of a 5 x 3 image (pixel size exactly 1)
    "light_on_plane_behind":
        "camera, width: 5.0, height: 3.0\n"
        "plane, normal: [0, 0, -1], diffuse_color: [0.3, 0.5, 0.7], specular_color: [1, 1, 1], "
        "position: [0, 0, 5], reflectivity: 0.5\n" + _LIGHT.format(c=4) + "position: [0, 0, 5]\n",
}

_scenes = {}


def scene(name):
    """A golden scene or one of OWN_SCENES, loaded once."""
    if name not in _scenes:
        path = scene_path(name)
        if name in OWN_SCENES:
            td = tempfile.TemporaryDirectory()
            _TMP.append(td)
            path = os.path.join(td.name, name + ".scene")
            with open(path, "w") as f:
                f.write(OWN_SCENES[name])
        _scenes[name] = rc.Scene.from_file(path)
    return _scenes[name]


def grid_dirs(name, view, s, mode, full=FULL):
    """view_dirs of every subsample of the s*full image, row-major."""
    js = scene(name).js
    fw, fh = s * full[0], s * full[1]
    return rc.view_dirs(js.camera_width, js.camera_height, (fw, fh), rc.view_grid(fw, fh),
                        VIEWS[view], cuda=mode == "cuda")


def oracle_shoot(name, d, mode):
    """(rgb [n, 3] float32, zero-normalize events, counts) of the oracle's bounce loop along d."""
    js = scene(name).js
    d = np.ascontiguousarray(d, F32)
    if mode == "cuda":
        rgb, cnt = sc.ref_shoot_cuda(js, d, DEPTH)
        return rgb, 0, cnt
    rgb, _, _, zero, cnt = sc.ref_shoot(js, d, DEPTH + 1, "fast")
    return rgb, int(zero.sum()), cnt


def oracle_quant(rgb):
    return sc.ref_quant(np.ascontiguousarray(rgb, F32).ravel()).reshape(rgb.shape)


_REF = {}


def view_image(name, view, s, mode, full=FULL):
    """(image [full_h, full_w, 3] uint8, zero-normalize events, counts): the box filter of the
    quantised oracle colours of view_dirs at s*full.  The events include the directions' own: a
    zero-length q, which the C port's normalize counts (none under these views: q.z = -+1)."""
    key = (name, view, s, mode, full)
    if key not in _REF:
        d = grid_dirs(name, view, s, mode, full)
        rgb, zero, cnt = oracle_shoot(name, d, mode)
        if mode != "cuda":
            zero += int((~d.any(axis=1)).sum())
        img = rc.box_downsample(oracle_quant(rgb).reshape(s * full[1], s * full[0], 3), s)
        img.setflags(write=False)
        _REF[key] = (img, zero, cnt)
    return _REF[key]


def oracle_hits(name, d, frame):
    """rco_prim_nearest(O = 0, D = d, skip = -1) as HIT_DTYPE records in rc_hit's conventions (a
    miss: id -1 and +0 everywhere; P and N +0 without frame), and the frames' zero events."""
    js = scene(name).js
    d = np.ascontiguousarray(d, F32)
    n = len(d)
    idx, t, P, N, z = pc.ref_nearest(js, np.zeros_like(d), d, np.full(n, -1, np.int32))
    hits = np.zeros(n, rc.HIT_DTYPE)
    hit = idx >= 0
    hits["id"] = np.where(hit, idx, -1)
    hits["t"][hit] = t[hit]
    if frame:
        hits["P"][hit] = P[hit]
        hits["N"][hit] = N[hit]
    return hits, int(z[hit].sum()) if frame else 0


def oracle_hits_cuda(name, d):
    js = scene(name).js
    d = np.ascontiguousarray(d, F32)
    idx, t = pc.ref_nearest(js, np.zeros_like(d), d, np.full(len(d), -1, np.int32), cuda=True)
    hits = np.zeros(len(d), rc.HIT_DTYPE)
    hit = idx >= 0
    hits["id"] = np.where(hit, idx, -1)
    hits["t"][hit] = t[hit]
    return hits
