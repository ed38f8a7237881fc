"""Accumulation through a free camera A/B on one visit: quadric.scene, depth 6, device-resident.
   PARENT=<a built checkout of the parent commit> python3 scripts/camera_accum_ab.py
The builds under test run in child processes of their own, one after the other and PASSES times
round robin, so a drift of the box touches all alike; inside a child the cases alternate round by
round (REPS rounds after WARM warm-up rounds).  Builds:
  new      this tree's libraycast_hip.so
  parent   PARENT's libraycast_hip.so through PARENT's own Python package: the yardstick of the
           window accumulation is the parent commit's library, never the new one's
Cases, each per size, all on hier4 (the parent runs the first three):
  one          k_render, one ray a pixel (rc_render_device)
  acc1         a one-sample pass of rc_accum_pass_device on a state of one sample (the record is
               read and written); acc1 / one is the plain family's own ratio
  win1         the same through rc_accum_pass_window_device, the whole image as its window
  frame        k_camera's one-ray frame through the moved camera (rc_render_camera_device)
  cam1         the one-sample pass of rc_accum_pass_camera_device through the moved camera
  cam1+0       the same with eye = +0 and the identity view: win1's records and bytes
  ssaa4        k_camera at ssaa = 4 through the moved camera
  cam16        all of hier4 as one reset pass of 16 through the moved camera: ssaa4's bytes
  lens16       the same pass through 16 thin-lens cameras around the moved one
Kernel times are the library's event spans (rc_timing.kernel_ms).  Every timed state (records and
image) is checked against the first round's; cam1+0 against win1's state and cam16 against ssaa4's
bytes.  Prints a table (and writes it to OUT).  No ratio is a gate."""
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
LENS_RADIUS, LENS_FOCUS = 0.3, 8.0
OLD = ["one", "acc1", "win1"]
NEW = ["frame", "cam1", "cam1+0", "ssaa4", "cam16", "lens16"]
STATES = ["acc1", "win1", "cam1", "cam1+0", "cam16", "lens16"]


def child():
    """One build: {"WxH": {case: [ms, ...]}, ...} and the state checks, as one JSON line."""
    sys.path.insert(0, os.path.join(os.environ.get("CAMERA_ACCUM_AB_TREE",
                                                   os.path.join(HERE, "..")), "tests"))
    import numpy as np
    import torch
    from helpers import rc, scene_path

    scene = rc.Scene.from_file(scene_path(os.environ.get("SCENE", "quadric")))
    new = hasattr(rc, "accum_pass_camera_device")
    cases = OLD + (NEW if new else [])
    if new:
        k = np.arange(16, dtype=np.float64)
        r, a = LENS_RADIUS * np.sqrt(k / 15.0), k * (np.pi * (3.0 - np.sqrt(5.0)))
        lens = rc.thin_lens(MOVED, None, LENS_FOCUS, np.stack([r * np.cos(a), r * np.sin(a)], 1))
    out = {"version": rc.version(), "sizes": {}}
    for w, h in SIZES:
        img = {k: torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for k in cases}
        acc = {k: torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
               for k in cases if k in STATES}
        torch.cuda.synchronize()
        whole = (w, h, 0, 0)

        def timed(fn, *args, **kw):
            tim = {}
            fn(*args, depth=D, timing=tim, **kw)
            return tim["kernel_ms"]

        def launch(k):
            a, o = (acc[k].data_ptr(), img[k].data_ptr()) if k in acc else (None, img[k].data_ptr())
            if k == "one":
                return timed(rc.render_device, scene, w, h, o, mode="fast")
            if k == "acc1":
                rc.accum_pass_device(scene, w, h, "hier4", 0, 1, a, o, reset=True, depth=D)
                return timed(rc.accum_pass_device, scene, w, h, "hier4", 1, 1, a, o)
            if k == "win1":
                rc.accum_pass_window_device(scene, whole, w, h, "hier4", 0, 1, a, o, reset=True,
                                            depth=D)
                return timed(rc.accum_pass_window_device, scene, whole, w, h, "hier4", 1, 1, a, o)
            if k == "frame":
                return timed(rc.render_camera_device, scene, MOVED, None, w, h, o)
            if k == "ssaa4":
                return timed(rc.render_camera_device, scene, MOVED, None, w, h, o, ssaa=4)
            if k in ("cam1", "cam1+0"):
                cam = (MOVED, None) if k == "cam1" else ((0.0, 0.0, 0.0), None)
                rc.accum_pass_camera_device(scene, cam, whole, w, h, "hier4", 0, 1, a, o,
                                            reset=True, depth=D)
                return timed(rc.accum_pass_camera_device, scene, cam, whole, w, h, "hier4", 1, 1,
                             a, o)
            cams = (MOVED, None) if k == "cam16" else lens
            return timed(rc.accum_pass_camera_device, scene, cams, whole, w, h, "hier4", 0, 16, a,
                         o, reset=True)

        ms = {k: [] for k in cases}
        first, same = {}, {k: True for k in cases}
        for r in range(WARM + REPS):
            for k in cases:
                t = launch(k)
                if r >= WARM:
                    ms[k].append(t)
            torch.cuda.synchronize()
            for k in cases:   # every timed state against the first round's
                state = [img[k]] + ([acc[k]] if k in acc else [])
                if k not in first:
                    first[k] = [s.clone() for s in state]
                elif not all(torch.equal(s, f) for s, f in zip(state, first[k])):
                    same[k] = False
        ok = {}
        if new:
            ok["cam1+0==win1"] = bool(torch.equal(img["cam1+0"], img["win1"]) and
                                      torch.equal(acc["cam1+0"], acc["win1"]))
            ok["cam16==ssaa4"] = bool(torch.equal(img["cam16"], img["ssaa4"]))
            ok["lens16!=cam16"] = bool(not torch.equal(img["lens16"], img["cam16"]))
        ok["win1==acc1"] = bool(torch.equal(img["win1"], img["acc1"]) and
                                torch.equal(acc["win1"], acc["acc1"]))
        out["sizes"][f"{w}x{h}"] = {"ms": ms, "same_every_round": same, "states_ok": ok}
        del img, acc, first
    print("CAMERA_ACCUM_AB " + json.dumps(out), flush=True)


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


def main():
    builds = [("new", None)]
    if os.environ.get("PARENT"):
        builds.append(("parent", os.environ["PARENT"]))
    runs = {b[0]: [] for b in builds}
    for _ in range(PASSES):
        for name, tree in builds:
            env = dict(os.environ)
            if tree:
                env["CAMERA_ACCUM_AB_TREE"] = tree
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env,
                               stdout=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"the {name} build's child ended with {p.returncode}")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("CAMERA_ACCUM_AB ")][-1]
            runs[name].append(json.loads(line[len("CAMERA_ACCUM_AB "):]))

    lines = [f"{name}: {runs[name][0]['version']}" for name, _ in builds]
    for w, h in SIZES:
        key = f"{w}x{h}"
        lines.append(f"{key} depth {D}, {PASSES} passes of {REPS} rounds a build, medians "
                     f"(max-min) in ms over all of a build's rounds; per pass in brackets")
        ms = {}
        for name, _ in builds:
            for k in runs[name][0]["sizes"][key]["ms"]:
                per = [r["sizes"][key]["ms"][k] for r in runs[name]]
                allv = [x for p in per for x in p]
                ms[name, k] = allv
                same = all(r["sizes"][key]["same_every_round"][k] for r in runs[name])
                lines.append(f"  {name:<8}{k:<9}{med(allv):8.4f} ({spread(allv):.4f})  "
                             f"[{', '.join(f'{med(p):.4f}' for p in per)}]   "
                             f"same every round: {same}")
            ok = {}
            for r in runs[name]:
                for k, v in r["sizes"][key]["states_ok"].items():
                    ok[k] = ok.get(k, True) and v
            lines.append(f"  {name:<8}states: {ok}")

        def ratio(a, b, what):
            if a in ms and b in ms:
                lines.append(f"  {what}: {a[0]} {a[1]} / {b[0]} {b[1]} = "
                             f"{med(ms[a]) / med(ms[b]):.4f}, difference "
                             f"{med(ms[a]) - med(ms[b]):+.4f} ms (spreads {spread(ms[a]):.4f} and "
                             f"{spread(ms[b]):.4f} ms)")

        ratio(("new", "one"), ("parent", "one"), "what a ratio between builds resolves (k_render)")
        ratio(("new", "win1"), ("parent", "win1"), "k_accum_win, new build against the parent's")
        ratio(("new", "acc1"), ("new", "one"), "the plain family's ratio, k_accum over k_render")
        ratio(("new", "cam1"), ("new", "frame"), "1. one-sample pass, moved camera, over k_camera's frame")
        ratio(("new", "cam1+0"), ("parent", "win1"), "2. one-sample pass at eye +0 over the parent's k_accum_win")
        ratio(("new", "cam16"), ("new", "ssaa4"), "3. hier4 in one pass of 16 over k_camera at ssaa 4")
        ratio(("new", "lens16"), ("new", "cam16"), "4. 16 lens cameras over one camera, 16 samples")
    table = "\n".join(lines)
    print(table, flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    child() if sys.argv[1:] == ["--child"] else main()
