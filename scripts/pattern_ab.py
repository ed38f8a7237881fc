"""Sparse sample patterns A/B on one visit: quadric.scene, depth 6, fast mode, device-resident.
For every size the cases below alternate round by round (REPS rounds after WARM warm-up rounds),
so a drift of the box touches all alike:
  one                     k_render (one ray per pixel)
  ssaa2 / ssaa4 / ssaa8   the fused ordered-grid kernel (4, 16, 64 rays per pixel)
  diag2 / rgss4 / checker8 / queens8
                          the dense pattern kernel (2, 4, 8, 8 rays per pixel)
  rgss4:T / queens8:T     the pattern over the edge list at threshold T, split by the library's
                          own HIP events into render, mark and refine (rc_pattern_phase_ms)
  ad4:T / ad8:T           RC_SSAA_ADAPTIVE(4, T) and (8, T): the full grid over the same list
Kernel times are the library's event spans (rc_last_kernel_ms).  Per case: median and max - min
spread in ms, rays and ns per ray.  Two claims are checked and printed either way:
  1. same ray count: dense rgss4 against ssaa2 (4 rays per pixel each): do the two
     [min, max] ranges overlap?
  2. against the full grid: rgss4 below ssaa4, and queens8 below ssaa8, by more than the two
     spreads combined?
The pattern bytes are checked against pattern_downsample of the GPU's own g*W x g*H image (where
that image has at most CHECK_MAX pixels a side) and the listed cases against adaptive_compose.
Prints a table (and writes it to OUT) and one JSON line per size (JSON_OUT)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import torch
from helpers import rc, scene_path

D = int(os.environ.get("DEPTH", "6"))
REPS = int(os.environ.get("REPS", "20"))
WARM = int(os.environ.get("WARM", "3"))
SIZES = [tuple(int(v) for v in c.split("x"))
         for c in os.environ.get("SIZES", "1024x1024,2048x2048").split(",")]
T = int(os.environ.get("THRESHOLD", "16"))
CHECK_MAX = int(os.environ.get("CHECK_MAX", "4096"))
scene = rc.Scene.from_file(scene_path(os.environ.get("SCENE", "quadric")))

DENSE = ["diag2", "rgss4", "checker8", "queens8"]
LISTED = ["rgss4", "queens8"]
CASES = (["one"] + [f"ssaa{s}" for s in (2, 4, 8)] + DENSE + [f"{p}:{T}" for p in LISTED]
         + [f"ad{s}:{T}" for s in (4, 8)])


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


def stat(v):
    return {"median": round(med(v), 4), "spread": round(spread(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4)}


lines, records = [], []
for w, h in SIZES:
    bufs = {k: torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for k in CASES}
    torch.cuda.synchronize()
    ms = {k: [] for k in CASES}
    phases = {k: {"render": [], "mark": [], "refine": []} for k in CASES if ":" in k}

    def launch(k):
        ptr = bufs[k].data_ptr()
        if k == "one":
            rc.render_device(scene, w, h, ptr, depth=D, mode="fast", timing={})
        elif k.startswith("ssaa"):
            rc.render_device(scene, w, h, ptr, depth=D, mode="fast", ssaa=int(k[4:]), timing={})
        elif k.startswith("ad"):
            rc.render_device(scene, w, h, ptr, depth=D, mode="fast", ssaa=int(k[2]), adaptive=T,
                             timing={})
        elif ":" in k:
            rc.render_pattern_device(scene, w, h, k.split(":")[0], ptr, threshold=T, depth=D,
                                     mode="fast", timing={})
        else:
            rc.render_pattern_device(scene, w, h, k, ptr, depth=D, mode="fast", timing={})
        return rc.last_kernel_ms()

    def spans(k):
        return rc.adaptive_phase_ms() if k.startswith("ad") else rc.pattern_phase_ms()

    for r in range(WARM + REPS):
        for k in CASES:
            t = launch(k)
            ph = spans(k) if k in phases else None
            if r >= WARM:
                ms[k].append(t)
                if ph:
                    for name in ph:
                        phases[k][name].append(ph[name])

    rays, listed_px = {"one": w * h}, {}
    for s in (2, 4, 8):
        rays[f"ssaa{s}"] = s * s * w * h
    for k in CASES:
        if k in rays:
            continue
        launch(k)   # the counts of a launch of its own
        st = rc.adaptive_stats() if k.startswith("ad") else rc.pattern_stats()
        rays[k] = st["rays"]
        if ":" in k:
            listed_px[k] = st["refined_pixels"]

    # the bytes: against the GPU's own images
    a = bufs["one"].cpu().numpy()
    ok = {}
    for k in DENSE:
        g, pts = rc.PATTERNS[k]
        if g * max(w, h) > CHECK_MAX:
            ok[k] = None   # not checked at this size
            continue
        big = torch.empty((g * h, g * w, 3), dtype=torch.uint8, device="cuda")
        rc.render_device(scene, g * w, g * h, big.data_ptr(), depth=D, mode="fast", timing={})
        ok[k] = bool((bufs[k].cpu().numpy() == rc.pattern_downsample(big.cpu().numpy(), g,
                                                                     pts)).all())
        del big
    for p in LISTED:
        ok[f"{p}:{T}"] = bool((bufs[f"{p}:{T}"].cpu().numpy()
                               == rc.adaptive_compose(a, bufs[p].cpu().numpy(), T)).all())
    for s in (4, 8):
        ok[f"ad{s}:{T}"] = bool((bufs[f"ad{s}:{T}"].cpu().numpy()
                                 == rc.adaptive_compose(a, bufs[f"ssaa{s}"].cpu().numpy(),
                                                        T)).all())

    rec = {"scene": os.environ.get("SCENE", "quadric"), "w": w, "h": h, "depth": D,
           "threshold": T, "launches": REPS, "version": rc.version(), "cases": {}, "claims": {}}
    lines.append(f"{w}x{h} depth {D}, {REPS} launches each, medians (max-min) in ms")
    for k in CASES:
        rec["cases"][k] = {"ms": stat(ms[k]), "rays": rays[k],
                           "ns_per_ray": round(med(ms[k]) * 1e6 / rays[k], 4),
                           "bytes_ok": ok.get(k)}
        line = (f"  {k:<12} {med(ms[k]):8.4f} ({spread(ms[k]):.4f})   rays {rays[k]:>10}   "
                f"{med(ms[k]) * 1e6 / rays[k]:.4f} ns/ray")
        if k in ok:
            line += f"   bytes ok: {ok[k] if ok[k] is not None else 'not checked'}"
        lines.append(line)
        if k in phases:
            rec["cases"][k]["phases"] = {n: stat(v) for n, v in phases[k].items()}
            rec["cases"][k]["listed_pixels"] = listed_px[k]
            sub = rays[k] - w * h
            refine = med(phases[k]["refine"])
            lines.append(
                f"      render {med(phases[k]['render']):.4f} ({spread(phases[k]['render']):.4f})  "
                f"mark {med(phases[k]['mark']):.4f} ({spread(phases[k]['mark']):.4f})  "
                f"refine {refine:.4f} ({spread(phases[k]['refine']):.4f})  listed {listed_px[k]} "
                f"({100.0 * listed_px[k] / (w * h):.2f} %)  refine {refine * 1e6 / max(sub, 1):.4f} "
                f"ns/ray")
    # claim 1: the same ray count
    p4, s2 = ms["rgss4"], ms["ssaa2"]
    overlap = min(p4) <= max(s2) and min(s2) <= max(p4)
    rec["claims"]["rgss4_vs_ssaa2"] = {"ranges_overlap": bool(overlap),
                                       "ratio": round(med(p4) / med(s2), 4)}
    lines.append(f"  claim 1  rgss4 / ssaa2 (4 rays per pixel each): ratio {med(p4) / med(s2):.4f}, "
                 f"ranges [{min(p4):.4f}, {max(p4):.4f}] and [{min(s2):.4f}, {max(s2):.4f}] "
                 f"overlap: {overlap}")
    # claim 2: against the full grid
    for p, s in (("rgss4", 4), ("queens8", 8)):
        full = ms[f"ssaa{s}"]
        beats = med(ms[p]) < med(full) - (spread(ms[p]) + spread(full))
        rec["claims"][f"{p}_vs_ssaa{s}"] = {"faster_beyond_spreads": bool(beats),
                                            "ratio": round(med(ms[p]) / med(full), 4)}
        lines.append(f"  claim 2  {p} / ssaa{s}: ratio {med(ms[p]) / med(full):.4f}, faster by "
                     f"more than the two spreads combined: {beats}")
    for p, s in (("rgss4", 4), ("queens8", 8)):
        kp, ka = f"{p}:{T}", f"ad{s}:{T}"
        lines.append(f"  listed   {kp} / {ka}: total ratio {med(ms[kp]) / med(ms[ka]):.4f}, "
                     f"refine ratio "
                     f"{med(phases[kp]['refine']) / med(phases[ka]['refine']):.4f}")
    records.append(rec)
    del bufs

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
