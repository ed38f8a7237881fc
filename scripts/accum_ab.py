"""Progressive supersampling A/B on one visit: quadric.scene, depth 6, fast mode, device-resident.
For every size the cases below alternate round by round (REPS rounds after WARM warm-up rounds),
so a drift of the box touches all alike:
  one / one'     k_render, one ray per pixel (rc_render_device), twice a round: the yardstick and
                 its own repeat, whose ratio and spread say what a ratio of this visit can resolve
  ssaa8          the fused ordered-grid kernel, 64 rays per pixel
  reset1         a reset pass of one sample (rc_accum_pass_device; the record is only written)
  acc1           the one-sample pass after it (the record is read and written)
  hier8x64       all of hier8 as a reset pass and 63 one-sample passes: the sum of their spans
  hier8x4        all of hier8 as four passes of 16 samples: the sum of their spans
  mask1:T        after a reset pass, one masked one-sample pass at threshold T, split by the
                 library's own HIP events into the edge list and the samples (rc_accum_phase_ms)
  rgss4:T        the pattern frame over the edge list (rc_pattern_phase_ms), for its refinement's
                 cost per ray
Kernel times are the library's event spans (rc_last_kernel_ms).  Three comparisons, none a gate:
  1. acc1 and reset1 against one            (what the 8-byte record costs beside a ray)
  2. hier8x64 and hier8x4 against ssaa8     (64 samples in 64, in 4 and in 1 launch)
  3. mask1:T's samples per ray against rgss4:T's refinement per ray
Every timed image is checked against the first round's, the hier8 images against ssaa8's bytes and
the masked pass against the numpy contract on the GPU's own 8W x 8H image (up to CHECK_MAX pixels
a side).  Prints a table (and writes it to OUT) and one JSON line per size (JSON_OUT)."""
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
T = int(os.environ.get("THRESHOLD", "16"))
CHECK_MAX = int(os.environ.get("CHECK_MAX", "8192"))
scene = rc.Scene.from_file(scene_path(os.environ.get("SCENE", "quadric")))

CASES = ["one", "one'", "ssaa8", "reset1", "acc1", "hier8x64", "hier8x4", f"mask1:{T}",
         f"rgss4:{T}"]
IMAGES = ["one", "one'", "ssaa8", "acc1", "hier8x64", "hier8x4", f"mask1:{T}", f"rgss4:{T}"]


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


def stat(v):
    return {"median": round(med(v), 4), "spread": round(spread(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4)}


lines, records = [], []
for w, h in SIZES:
    img = {k: torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for k in IMAGES}
    acc = {k: torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
           for k in ("acc1", "hier8x64", "hier8x4", f"mask1:{T}")}
    torch.cuda.synchronize()
    ms = {k: [] for k in CASES}
    phases = {f"mask1:{T}": {"mark": [], "shoot": []},
              f"rgss4:{T}": {"render": [], "mark": [], "refine": []}}
    first, same = {}, {k: True for k in IMAGES}
    counts = {}

    def accum(k, start, count, t=0, reset=False):
        rc.accum_pass_device(scene, w, h, "hier8", start, count, acc[k].data_ptr(),
                             img[k].data_ptr(), threshold=t, reset=reset, depth=D, mode="fast",
                             timing={})
        return rc.last_kernel_ms()

    def launch(k):
        """The case's kernel time in ms; a dict of further cases measured on the way."""
        if k in ("one", "one'"):
            rc.render_device(scene, w, h, img[k].data_ptr(), depth=D, mode="fast", timing={})
            return rc.last_kernel_ms()
        if k == "ssaa8":
            rc.render_device(scene, w, h, img[k].data_ptr(), depth=D, mode="fast", ssaa=8,
                             timing={})
            return rc.last_kernel_ms()
        if k == "acc1":
            return None   # measured with reset1, on one state
        if k == "reset1":
            return {"reset1": accum("acc1", 0, 1, reset=True), "acc1": accum("acc1", 1, 1)}
        if k == "hier8x64":
            return sum(accum(k, j, 1, reset=j == 0) for j in range(64))
        if k == "hier8x4":
            return sum(accum(k, j, 16, reset=j == 0) for j in range(0, 64, 16))
        if k.startswith("mask1"):
            accum(k, 0, 1, reset=True)
            t = accum(k, 1, 1, t=T)
            for name, v in rc.accum_phase_ms().items():
                phases[k][name].append(v)
            counts[k] = rc.accum_stats()
            return t
        rc.render_pattern_device(scene, w, h, "rgss4", img[k].data_ptr(), threshold=T, depth=D,
                                 mode="fast", timing={})
        t = rc.last_kernel_ms()
        for name, v in rc.pattern_phase_ms().items():
            phases[k][name].append(v)
        counts[k] = rc.pattern_stats()
        return t

    for r in range(WARM + REPS):
        for k in CASES:
            t = launch(k)
            if r >= WARM and t is not None:
                for name, v in (t.items() if isinstance(t, dict) else [(k, t)]):
                    ms[name].append(v)
        for k in IMAGES:   # every timed image against the first round's
            if k not in first:
                first[k] = img[k].clone()
            elif not torch.equal(img[k], first[k]):
                same[k] = False
    for k in phases:
        for name in phases[k]:
            phases[k][name] = phases[k][name][WARM:]

    # the bytes: the hier8 images are ssaa = 8's, the states hold 64 samples a pixel; the masked
    # pass is the numpy contract on the GPU's own 8W x 8H image
    ok = {"hier8x64": bool(torch.equal(img["hier8x64"], img["ssaa8"])
                           and (acc["hier8x64"][:, :, 3] == 64).all()),
          "hier8x4": bool(torch.equal(img["hier8x4"], img["ssaa8"])
                          and torch.equal(acc["hier8x4"], acc["hier8x64"])),
          "one'": bool(torch.equal(img["one'"], img["one"]))}
    if 8 * max(w, h) <= CHECK_MAX:
        big = torch.empty((8 * h, 8 * w, 3), dtype=torch.uint8, device="cuda")
        rc.render_device(scene, 8 * w, 8 * h, big.data_ptr(), depth=D, mode="fast", timing={})
        big = big.cpu().numpy()
        pts = rc.SAMPLE_SEQS["hier8"][1]
        zero = np.zeros((h, w, 4), np.uint16), np.zeros((h, w, 3), np.uint8)
        a1, o1, _, _ = rc.accum_step(*zero, big, 8, pts[:1], 0, reset=True)
        a2, o2, _, _ = rc.accum_step(a1, o1, big, 8, pts[1:2], 0)
        ok["acc1"] = bool((img["acc1"].cpu().numpy() == o2).all()
                          and (acc["acc1"].cpu().numpy().view(np.uint16) == a2).all())
        a3, o3, active, _ = rc.accum_step(a1, o1, big, 8, pts[1:2], T)
        k = f"mask1:{T}"
        ok[k] = bool((img[k].cpu().numpy() == o3).all()
                     and (acc[k].cpu().numpy().view(np.uint16) == a3).all()
                     and counts[k]["active_pixels"] == active)
        del big

    rays = {"one": w * h, "one'": w * h, "ssaa8": 64 * w * h, "reset1": w * h, "acc1": w * h,
            "hier8x64": 64 * w * h, "hier8x4": 64 * w * h,
            f"mask1:{T}": counts[f"mask1:{T}"]["rays"], f"rgss4:{T}": counts[f"rgss4:{T}"]["rays"]}
    rec = {"scene": os.environ.get("SCENE", "quadric"), "w": w, "h": h, "depth": D,
           "threshold": T, "launches": REPS, "version": rc.version(), "cases": {},
           "comparisons": {}}
    lines.append(f"{w}x{h} depth {D}, {REPS} rounds, medians (max-min) in ms")
    for k in CASES:
        rec["cases"][k] = {"ms": stat(ms[k]), "rays": rays[k],
                           "ns_per_ray": round(med(ms[k]) * 1e6 / rays[k], 4),
                           "same_every_round": same.get(k), "bytes_ok": ok.get(k)}
        line = (f"  {k:<10} {med(ms[k]):8.4f} ({spread(ms[k]):.4f})   rays {rays[k]:>10}   "
                f"{med(ms[k]) * 1e6 / rays[k]:.4f} ns/ray")
        if k in same:
            line += f"   same every round: {same[k]}"
        if k in ok:
            line += f"   bytes ok: {ok[k]}"
        lines.append(line)
        if k in phases:
            rec["cases"][k]["phases"] = {n: stat(v) for n, v in phases[k].items()}
            lines.append("      " + "  ".join(f"{n} {med(v):.4f} ({spread(v):.4f})"
                                              for n, v in phases[k].items()))
    base, rep = ms["one"], ms["one'"]
    noise = (f"one' / one {med(rep) / med(base):.4f}, spreads {spread(base):.4f} and "
             f"{spread(rep):.4f} ms")
    rec["comparisons"]["baseline_repeat"] = {"ratio": round(med(rep) / med(base), 4),
                                             "spread": round(spread(base), 4),
                                             "spread_repeat": round(spread(rep), 4)}
    # 1. what the record costs beside a ray
    for k in ("acc1", "reset1"):
        rec["comparisons"][f"{k}_vs_one"] = {
            "ratio": round(med(ms[k]) / med(base), 4),
            "difference_ms": round(med(ms[k]) - med(base), 4), "spread": round(spread(ms[k]), 4)}
        lines.append(f"  1. {k} / one: ratio {med(ms[k]) / med(base):.4f}, difference "
                     f"{med(ms[k]) - med(base):+.4f} ms (spread {spread(ms[k]):.4f}; {noise})")
    # 2. 64 samples in 64, in 4 and in 1 launch
    full = ms["ssaa8"]
    for k in ("hier8x64", "hier8x4"):
        rec["comparisons"][f"{k}_vs_ssaa8"] = {"ratio": round(med(ms[k]) / med(full), 4),
                                               "spread": round(spread(ms[k]), 4),
                                               "spread_ssaa8": round(spread(full), 4)}
        lines.append(f"  2. {k} / ssaa8: ratio {med(ms[k]) / med(full):.4f} (spreads "
                     f"{spread(ms[k]):.4f} and {spread(full):.4f} ms; {noise})")
    # 3. per ray over the edge list
    km, kp = f"mask1:{T}", f"rgss4:{T}"
    shoot, refine = phases[km]["shoot"], phases[kp]["refine"]
    mrays = counts[km]["rays"]
    prays = 4 * counts[kp]["refined_pixels"]
    per_m, per_p = med(shoot) * 1e6 / max(mrays, 1), med(refine) * 1e6 / max(prays, 1)
    rec["comparisons"]["mask1_vs_rgss4_per_ray"] = {
        "mask1_ns_per_ray": round(per_m, 4), "rgss4_ns_per_ray": round(per_p, 4),
        "ratio": round(per_m / per_p, 4), "mask1_rays": mrays, "rgss4_refine_rays": prays,
        "spread_shoot": round(spread(shoot), 4), "spread_refine": round(spread(refine), 4)}
    lines.append(f"  3. {km} samples {med(shoot):.4f} ({spread(shoot):.4f}) ms over {mrays} rays = "
                 f"{per_m:.4f} ns/ray; {kp} refinement {med(refine):.4f} ({spread(refine):.4f}) ms "
                 f"over {prays} rays = {per_p:.4f} ns/ray; ratio {per_m / per_p:.4f} ({noise})")
    records.append(rec)
    del img, acc, first

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
