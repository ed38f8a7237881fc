"""Adaptive supersampling A/B on one visit: quadric.scene, depth 6, fast mode, device-resident.
For every configuration (W, H, s) three kinds of launch alternate round by round (REPS rounds
after WARM warm-up rounds), so a drift of the box touches all alike:
  one   k_render at W x H (one ray per pixel: what the adaptive frame starts with)
  full  the fused ssaa = s kernel at W x H (s*s rays per pixel: the path adaptive competes with)
  t8 / t16 / t32
        the adaptive frame at threshold t, split by the library's own HIP events into render,
        mark and refine (rc_adaptive_phase_ms)
Kernel times are the library's event spans (rc_last_kernel_ms).  Per case: median and max - min
spread in ms; per adaptive case also refined_pixels and rays (rc_adaptive_stats_get), the
refinement's ns per ray beside k_render's, mark's share of k_render, mark against a plain device
copy of the W*H*3 bytes it reads, and whether the adaptive total is below the full-ssaa median
by more than the two spreads combined.  The adaptive bytes are checked against
adaptive_compose of the GPU's own one-ray and full images.  Prints a table (and writes it to
OUT) and one JSON line per configuration (JSON_OUT)."""
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
CONFIGS = [tuple(int(v) for v in c.split("x"))
           for c in os.environ.get("CONFIGS", "1024x1024x4,2048x2048x2,2048x2048x4").split(",")]
THRESHOLDS = [int(t) for t in os.environ.get("THRESHOLDS", "8,16,32").split(",")]
if os.environ.get("ADAPTIVE_BLOCKS"):   # rc_tuning.adaptive_blocks for the whole run (0: default)
    rc.set_tuning(adaptive_blocks=int(os.environ["ADAPTIVE_BLOCKS"]))
scene = rc.Scene.from_file(scene_path(os.environ.get("SCENE", "quadric")))


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


lines, records = [], []
for w, h, s in CONFIGS:
    cases = ["one", "full"] + [f"t{t}" for t in THRESHOLDS]
    bufs = {k: torch.empty((h, w, 3), dtype=torch.uint8, device="cuda") for k in cases}
    copy_dst = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    phases = {k: {"render": [], "mark": [], "refine": []} for k in cases[2:]}
    copy_ms = []

    def launch(k):
        if k == "one":
            rc.render_device(scene, w, h, bufs[k].data_ptr(), depth=D, mode="fast", timing={})
        elif k == "full":
            rc.render_device(scene, w, h, bufs[k].data_ptr(), depth=D, mode="fast", ssaa=s,
                             timing={})
        else:
            rc.render_device(scene, w, h, bufs[k].data_ptr(), depth=D, mode="fast", ssaa=s,
                             adaptive=int(k[1:]), timing={})
        return rc.last_kernel_ms()

    for r in range(WARM + REPS):
        for k in cases:
            t = launch(k)
            ph = rc.adaptive_phase_ms() if k in phases else None
            if r >= WARM:
                ms[k].append(t)
                if ph:
                    for name in ph:
                        phases[k][name].append(ph[name])
        # the plain read mark is compared with: a device copy of the W*H*3 bytes
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        copy_dst.copy_(bufs["one"])
        e1.record()
        torch.cuda.synchronize()
        if r >= WARM:
            copy_ms.append(e0.elapsed_time(e1))

    a, f = bufs["one"].cpu().numpy(), bufs["full"].cpu().numpy()
    rec = {"scene": os.environ.get("SCENE", "quadric"), "w": w, "h": h, "s": s, "depth": D,
           "launches": REPS, "version": rc.version(),
           "one_ms": {"median": round(med(ms["one"]), 4), "spread": round(spread(ms["one"]), 4)},
           "full_ms": {"median": round(med(ms["full"]), 4),
                       "spread": round(spread(ms["full"]), 4)},
           "copy_ms": {"median": round(med(copy_ms), 4), "spread": round(spread(copy_ms), 4)},
           "adaptive": {}}
    one_ns_per_ray = med(ms["one"]) * 1e6 / (w * h)
    lines.append(f"{w}x{h} s={s} depth {D}, {REPS} launches each, medians (max-min) in ms")
    lines.append(f"  k_render {w}x{h}          {med(ms['one']):.4f} ({spread(ms['one']):.4f})   "
                 f"{one_ns_per_ray:.4f} ns/ray")
    lines.append(f"  fused ssaa {s}              {med(ms['full']):.4f} ({spread(ms['full']):.4f})   "
                 f"{med(ms['full']) * 1e6 / (w * h * s * s):.4f} ns/ray")
    lines.append(f"  copy of W*H*3 bytes       {med(copy_ms):.4f} ({spread(copy_ms):.4f})")
    for t in THRESHOLDS:
        k = f"t{t}"
        # the last launch of the loop was not this case's: take its counts from a launch of its own
        launch(k)
        st = rc.adaptive_stats()
        same = bool((bufs[k].cpu().numpy() == rc.adaptive_compose(a, f, t)).all())
        sub_rays = st["rays"] - w * h
        refine = med(phases[k]["refine"])
        beats = med(ms[k]) < med(ms["full"]) - (spread(ms[k]) + spread(ms["full"]))
        rec["adaptive"][k] = {
            "total_ms": {"median": round(med(ms[k]), 4), "spread": round(spread(ms[k]), 4)},
            **{name: {"median": round(med(v), 4), "spread": round(spread(v), 4)}
               for name, v in phases[k].items()},
            "refined_pixels": st["refined_pixels"], "rays": st["rays"],
            "refine_ns_per_ray": round(refine * 1e6 / sub_rays, 4) if sub_rays else None,
            "one_ns_per_ray": round(one_ns_per_ray, 4),
            "mark_over_one": round(med(phases[k]["mark"]) / med(ms["one"]), 4),
            "mark_over_copy": round(med(phases[k]["mark"]) / med(copy_ms), 3),
            "below_full_beyond_spreads": bool(beats), "bytes_equal_compose": same}
        lines.append(
            f"  adaptive t={t:<3} total       {med(ms[k]):.4f} ({spread(ms[k]):.4f})   "
            f"render {med(phases[k]['render']):.4f} ({spread(phases[k]['render']):.4f})  "
            f"mark {med(phases[k]['mark']):.4f} ({spread(phases[k]['mark']):.4f})  "
            f"refine {refine:.4f} ({spread(phases[k]['refine']):.4f})")
        lines.append(
            f"      refined_pixels {st['refined_pixels']} ({100.0 * st['refined_pixels'] / (w * h):.2f} %)  "
            f"rays {st['rays']}  refine {refine * 1e6 / max(sub_rays, 1):.4f} ns/ray  "
            f"mark/k_render {med(phases[k]['mark']) / med(ms['one']):.3f}  "
            f"mark/copy {med(phases[k]['mark']) / med(copy_ms):.2f}  "
            f"below full beyond spreads: {beats}  bytes ok: {same}")
    records.append(rec)
    del bufs, copy_dst

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
