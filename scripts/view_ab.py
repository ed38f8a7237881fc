"""Rotated views and ray batches A/B on one visit: quadric.scene, depth 6, device-resident.  For
every size the cases below alternate round by round (REPS rounds after WARM warm-up rounds), so a
drift of the box touches all alike.  The yardstick is k_window's time in the same visit:
  winS / win1'   the identity window at s = 1, 2, 4, 8 (k_window, rc_render_window_device); win1'
                 is win1's own repeat, whose ratio and spread say what a ratio of this visit resolves
  viewS          the identity view at s (k_view, rc_render_view_device): equal bytes, against winS
  cwinS / cviewS the same pair in cuda mode at s = 1 and 4
  yaw30:S        the view turned by 30 degrees at s = 1 and 4, against winS: other rays, another
                 picture, so the cost depends on the content; reported, not judged
  rays           k_rays (rc_trace_rays_device, rgb8 only) on the directions of the win1 frame
                 (rc.view_dirs of the identity), against win1: equal bytes; the cost of the 12-byte
                 strided loads and of the lost 8 x 8 blocks (a wave holds 64 pixels of one row)
  rays+hits      the same batch with the records too (frame = 1)
Kernel times are the library's event spans (rc_timing.kernel_ms, rc_view_phase_ms for the ray
batches).  Every timed image is checked against the first round's, the identity views and the ray
batch against k_window's bytes.  Prints a table (and writes it to OUT) and one JSON line per size
(JSON_OUT).  No ratio is a gate."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import torch
from helpers import rc, scene_path

D = int(os.environ.get("DEPTH", "6"))
REPS = int(os.environ.get("REPS", "20"))
WARM = int(os.environ.get("WARM", "3"))
SIZES = [tuple(int(v) for v in c.split("x"))
         for c in os.environ.get("SIZES", "1024x1024,2048x2048").split(",")]
scene = rc.Scene.from_file(scene_path(os.environ.get("SCENE", "quadric")))
IDENT = rc.view_identity()
YAW30 = rc.view_euler(np.pi / 6, 0.0, 0.0)

FACTORS = (1, 2, 4, 8)
CUDA_FACTORS = (1, 4)
CASES = (["win1'"] + [f"{p}{s}" for s in FACTORS for p in ("win", "view")]
         + [f"{p}{s}" for s in CUDA_FACTORS for p in ("cwin", "cview")]
         + ["yaw30:1", "yaw30:4", "rays", "rays+hits"])
# case -> its yardstick
PAIRS = ([("win1'", "win1")] + [(f"view{s}", f"win{s}") for s in FACTORS]
         + [(f"cview{s}", f"cwin{s}") for s in CUDA_FACTORS]
         + [("yaw30:1", "win1"), ("yaw30:4", "win4"), ("rays", "win1"), ("rays+hits", "win1")])
SAME_BYTES = [p for p in PAIRS if not p[0].startswith("yaw")]


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


def stat(v):
    return {"median": round(med(v), 4), "spread": round(spread(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4)}


lines, records = [], []
for w, h in SIZES:
    img = {k: torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for k in CASES}
    dirs = rc.view_dirs(scene.js.camera_width, scene.js.camera_height, (w, h), rc.view_grid(w, h),
                        IDENT)
    d_dirs = torch.from_numpy(dirs).cuda()
    d_hits = torch.zeros((w * h, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ident = (w, h, 0, 0)

    def launch(k):
        """The case's kernel time in ms."""
        tim = {}
        if k.startswith("rays"):
            rc.trace_rays_device(scene, w * h, d_dirs.data_ptr(), d_rgb8_ptr=img[k].data_ptr(),
                                 d_hits_ptr=d_hits.data_ptr() if k == "rays+hits" else None,
                                 frame=True, depth=D, mode="fast")
            return rc.view_phase_ms()["kernel"]
        mode = "cuda" if k.startswith("c") else "fast"
        s = int(k.rstrip("'")[-1])
        if "win" in k:
            rc.render_window_device(scene, ident, w, h, img[k].data_ptr(), ssaa=s, depth=D,
                                    mode=mode, timing=tim)
        else:
            rc.render_view_device(scene, YAW30 if k.startswith("yaw") else IDENT, w, h,
                                  img[k].data_ptr(), ssaa=s, depth=D, mode=mode, timing=tim)
        return tim["kernel_ms"]

    ms = {k: [] for k in CASES}
    first, same = {}, {k: True for k in CASES}
    for r in range(WARM + REPS):
        for k in CASES:
            t = launch(k)
            if r >= WARM:
                ms[k].append(t)
        for k in CASES:   # every timed image against the first round's
            if k not in first:
                first[k] = img[k].clone()
            elif not torch.equal(img[k], first[k]):
                same[k] = False
    ok = {a: bool(torch.equal(img[a], img[b])) for a, b in SAME_BYTES}

    rays = {k: w * h * (int(k.rstrip("'")[-1]) ** 2 if k[-1] in "1248'" else 1) for k in CASES}
    rec = {"scene": os.environ.get("SCENE", "quadric"), "w": w, "h": h, "depth": D,
           "launches": REPS, "version": rc.version(), "cases": {}, "comparisons": {}}
    lines.append(f"{w}x{h} depth {D}, {REPS} rounds, medians (max-min) in ms")
    for k in CASES:
        rec["cases"][k] = {"ms": stat(ms[k]), "rays": rays[k],
                           "ns_per_ray": round(med(ms[k]) * 1e6 / rays[k], 4),
                           "same_every_round": same[k], "bytes_ok": ok.get(k)}
        line = (f"  {k:<10} {med(ms[k]):8.4f} ({spread(ms[k]):.4f})   rays {rays[k]:>10}   "
                f"{med(ms[k]) * 1e6 / rays[k]:.4f} ns/ray   same every round: {same[k]}")
        if k in ok:
            line += f"   bytes ok: {ok[k]}"
        lines.append(line)
    for a, b in PAIRS:
        rec["comparisons"][f"{a}_vs_{b}"] = {
            "ratio": round(med(ms[a]) / med(ms[b]), 4),
            "difference_ms": round(med(ms[a]) - med(ms[b]), 4), "spread": round(spread(ms[a]), 4),
            "spread_yardstick": round(spread(ms[b]), 4)}
        lines.append(f"  {a} / {b}: ratio {med(ms[a]) / med(ms[b]):.4f}, difference "
                     f"{med(ms[a]) - med(ms[b]):+.4f} ms (spreads {spread(ms[a]):.4f} and "
                     f"{spread(ms[b]):.4f} ms)")
    records.append(rec)
    del img, first, d_dirs, d_hits

table = "\n".join(lines)
print(table, flush=True)
for rec in records:
    print(json.dumps(rec), flush=True)
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as fh:
        fh.write(table + "\n")
if os.environ.get("JSON_OUT"):
    with open(os.environ["JSON_OUT"], "w") as fh:
        for rec in records:
            fh.write(json.dumps(rec) + "\n")
