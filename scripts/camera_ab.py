"""A free camera and rays with origins A/B on one visit: quadric.scene, depth 6, device-resident.
   python3 scripts/camera_ab.py            (after `make camera-variants`)
The builds under test run in child processes of their own, one after the other and PASSES times
round robin, so a drift of the box touches all alike; inside a child the cases alternate round by
round (REPS rounds after WARM warm-up rounds).  Builds:
  table    libraycast_hip_camtable.so (RC_CAMERA_TABLE=1): k_camera reads the eye's origin-only
           shape terms from its workgroup's LDS table
  general  libraycast_hip_camgen.so (RC_CAMERA_TABLE=0): k_camera calls the general nearest with
           O = eye; one of the two is the product's form, and every other kernel is the product's
  parent   optional, PARENT=<a built checkout of the parent commit>: its k_view and k_rays
Cases, each per size:
  view1       the identity view (k_view, rc_render_view_device): the yardstick
  rays        k_rays (rc_trace_rays_device, rgb8 only) on the directions of that frame
  cam-0       k_camera at eye = (-0, -0, -0) with the identity: the origin's image through the
              camera kernel (an eye of three +0 dispatches to k_view and would measure nothing new)
  cam+0       eye = (+0, +0, +0): the dispatch to k_view, against view1
  cam_moved   eye = (0.5, 0.25, 1.0): another picture, so the cost depends on the content
  from0       k_rays_from (rc_trace_rays_from_device, rgb8 only) with every origin +0 on the
              frame's directions, against rays: the cost of the second strided load and of the
              general nearest in nearest_primary's place
  from_moved  the same with every origin (0.5, 0.25, 1.0), against cam_moved
Kernel times are the library's event spans (rc_timing.kernel_ms, rc_view_phase_ms for the ray
batches).  Every timed image is checked against the first round's; cam-0, cam+0 and from0 against
view1's bytes, from_moved against cam_moved's.  Prints a table (and writes it to OUT).  No ratio
is a gate."""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
D = int(os.environ.get("DEPTH", "6"))
REPS = int(os.environ.get("REPS", "20"))
WARM = int(os.environ.get("WARM", "3"))
PASSES = int(os.environ.get("PASSES", "2"))
SIZES = [tuple(int(v) for v in c.split("x"))
         for c in os.environ.get("SIZES", "1024x1024,2048x2048").split(",")]
MOVED = (0.5, 0.25, 1.0)
SAME_BYTES = [("cam-0", "view1"), ("cam+0", "view1"), ("from0", "view1"), ("rays", "view1"),
              ("from_moved", "cam_moved")]


def child():
    """One build: {"WxH": {case: [ms, ...]}, ...} and the byte checks, as one JSON line."""
    sys.path.insert(0, os.path.join(os.environ.get("CAMERA_AB_TREE", os.path.join(HERE, "..")),
                                    "tests"))
    import numpy as np
    import torch
    from helpers import rc, scene_path

    scene = rc.Scene.from_file(scene_path(os.environ.get("SCENE", "quadric")))
    ident = rc.view_identity()
    camera = hasattr(rc, "render_camera_device")
    cases = ["view1", "rays"] + (["cam-0", "cam+0", "cam_moved", "from0", "from_moved"]
                                 if camera else [])
    out = {"version": rc.version(), "sizes": {}}
    for w, h in SIZES:
        img = {k: torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for k in cases}
        dirs = rc.view_dirs(scene.js.camera_width, scene.js.camera_height, (w, h),
                            rc.view_grid(w, h), ident)
        d_dirs = torch.from_numpy(dirs).cuda()
        d_zero = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
        d_moved = torch.from_numpy(np.tile(np.asarray(MOVED, np.float32), (w * h, 1))).cuda()
        torch.cuda.synchronize()

        def launch(k):
            tim = {}
            if k == "rays":
                rc.trace_rays_device(scene, w * h, d_dirs.data_ptr(), d_rgb8_ptr=img[k].data_ptr(),
                                     depth=D, mode="fast")
                return rc.view_phase_ms()["kernel"]
            if k.startswith("from"):
                o = d_zero if k == "from0" else d_moved
                rc.trace_rays_from_device(scene, w * h, o.data_ptr(), d_dirs.data_ptr(),
                                          d_rgb8_ptr=img[k].data_ptr(), depth=D)
                return rc.view_phase_ms()["kernel"]
            if k == "view1":
                rc.render_view_device(scene, ident, w, h, img[k].data_ptr(), depth=D, mode="fast",
                                      timing=tim)
            else:
                eye = {"cam-0": (-0.0, -0.0, -0.0), "cam+0": (0.0, 0.0, 0.0), "cam_moved": MOVED}[k]
                rc.render_camera_device(scene, eye, ident, w, h, img[k].data_ptr(), depth=D,
                                        timing=tim)
            return tim["kernel_ms"]

        ms = {k: [] for k in cases}
        first, same = {}, {k: True for k in cases}
        for r in range(WARM + REPS):
            for k in cases:
                t = launch(k)
                if r >= WARM:
                    ms[k].append(t)
            for k in cases:
                if k not in first:
                    first[k] = img[k].clone()
                elif not torch.equal(img[k], first[k]):
                    same[k] = False
        ok = {f"{a}=={b}": bool(torch.equal(img[a], img[b])) for a, b in SAME_BYTES
              if a in img and b in img}
        out["sizes"][f"{w}x{h}"] = {"ms": ms, "same_every_round": same, "bytes_ok": ok}
        del img, first, d_dirs, d_zero, d_moved
    print("CAMERA_AB " + json.dumps(out), flush=True)


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


def main():
    builds = [("table", "libraycast_hip_camtable.so", None),
              ("general", "libraycast_hip_camgen.so", None)]
    if os.environ.get("PARENT"):
        builds.append(("parent", "libraycast_hip.so", os.environ["PARENT"]))
    runs = {b[0]: [] for b in builds}
    for _ in range(PASSES):
        for name, lib, tree in builds:
            env = dict(os.environ, RC_HIP_LIB=lib)
            if tree:
                env["CAMERA_AB_TREE"] = tree
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env,
                               stdout=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"the {name} build's child ended with {p.returncode}")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("CAMERA_AB ")][-1]
            runs[name].append(json.loads(line[len("CAMERA_AB "):]))

    lines = []
    for w, h in SIZES:
        key = f"{w}x{h}"
        lines.append(f"{key} depth {D}, {PASSES} passes of {REPS} rounds a build, medians "
                     f"(max-min) in ms over all of a build's rounds; per pass in brackets")
        ms = {}
        for name, _, _ in builds:
            for k in runs[name][0]["sizes"][key]["ms"]:
                per = [r["sizes"][key]["ms"][k] for r in runs[name]]
                allv = [x for p in per for x in p]
                ms[name, k] = allv
                same = all(r["sizes"][key]["same_every_round"][k] for r in runs[name])
                lines.append(f"  {name:<8}{k:<11}{med(allv):8.4f} ({spread(allv):.4f})  "
                             f"[{', '.join(f'{med(p):.4f}' for p in per)}]   "
                             f"same every round: {same}")
            ok = {}
            for r in runs[name]:
                ok.update(r["sizes"][key]["bytes_ok"])
            lines.append(f"  {name:<8}bytes: {ok}")

        def ratio(a, b, what):
            if a in ms and b in ms:
                lines.append(f"  {what}: {a[0]} {a[1]} / {b[0]} {b[1]} = "
                             f"{med(ms[a]) / med(ms[b]):.4f}, difference "
                             f"{med(ms[a]) - med(ms[b]):+.4f} ms (spreads {spread(ms[a]):.4f} and "
                             f"{spread(ms[b]):.4f} ms)")

        for b in ("table", "general"):
            ratio((b, "view1"), ("parent", "view1"), "k_view against the parent's")
            ratio((b, "rays"), ("parent", "rays"), "k_rays against the parent's")
        ratio(("general", "view1"), ("table", "view1"), "what a ratio between builds resolves")
        for b in ("table", "general"):
            ratio((b, "cam-0"), ("parent", "view1"), "k_camera at the origin against the parent's k_view")
            ratio((b, "cam-0"), (b, "view1"), "k_camera at the origin against k_view")
            ratio((b, "cam+0"), (b, "view1"), "the +0 dispatch against k_view")
        ratio(("table", "cam-0"), ("general", "cam-0"), "table against general form, origin")
        ratio(("table", "cam_moved"), ("general", "cam_moved"), "table against general form, moved eye")
        for b in ("table", "general"):
            ratio((b, "cam_moved"), (b, "view1"), "moved eye (another picture) against k_view")
        ratio(("table", "from0"), ("table", "rays"), "k_rays_from against k_rays")
        ratio(("table", "from_moved"), ("table", "cam_moved"), "k_rays_from against k_camera, moved eye")
    table = "\n".join(lines)
    print(table, flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    child() if sys.argv[1:] == ["--child"] else main()
