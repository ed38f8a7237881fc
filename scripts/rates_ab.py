"""Rate-map supersampling A/B on one visit: quadric.scene, depth 6, fast mode, device-resident.
For every size (W = H) the cases below alternate round by round (REPS rounds after WARM warm-up
rounds), so a drift of the box touches all alike:
  one      k_render at W x H (one ray per pixel)
  ssaa4 / ssaa8
           the fused ssaa = 4 / 8 kernels (the dense paths a map competes with)
  adapt    the adaptive frame, s = 4, t = 16
  u1       the rate path, every pixel at rate 1   (against one: what the masked pass costs)
  u4       the rate path, every pixel at rate 4   (against ssaa4: list refinement against dense)
  fovea    disc of radius H/8 at 8, ring to H/4 at 4, ring to H/2 at 2, else 1
                                                  (against one and ssaa8)
  roi      a 256 x 256 rectangle of rate 4 in zeros (against ssaa4: the fixed cost)
  amap     adaptive's own map (edge_mask of the one-ray image at t = 16 -> 4, else 0) over the
           one-ray image                          (against adapt)
Kernel times are the library's event spans (rc_timing.kernel_ms; rc_rate_phase_ms splits a rate
frame into the rate-1 pass with the binning and the refinement).  Per case: median and max - min
spread in ms; per rate case also the rays (rc_rate_stats_get), the refinement's ns per subsample
ray, and the ratio to the case it is compared with, marked when the two differ by more than
their spreads combined.  Every rate image is checked against rates_compose of the GPU's own
images.  Prints a table (and writes it to OUT) and one JSON line per size (JSON_OUT)."""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import torch
from helpers import rc, scene_path

D = int(os.environ.get("DEPTH", "6"))
REPS = int(os.environ.get("REPS", "30"))
WARM = int(os.environ.get("WARM", "3"))
SIZES = [int(v) for v in os.environ.get("SIZES", "1024,2048").split(",")]
T, S = 16, 4   # the adaptive frame of case amap
if os.environ.get("ADAPTIVE_BLOCKS"):   # rc_tuning.adaptive_blocks for the whole run (0: default)
    rc.set_tuning(adaptive_blocks=int(os.environ["ADAPTIVE_BLOCKS"]))
scene = rc.Scene.from_file(scene_path(os.environ.get("SCENE", "quadric")))


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


def fovea(n):
    yy, xx = np.mgrid[0:n, 0:n]
    d2 = (xx - n // 2) ** 2 + (yy - n // 2) ** 2
    m = np.ones((n, n), dtype=np.uint8)
    m[d2 < (n // 2) ** 2] = 2
    m[d2 < (n // 4) ** 2] = 4
    m[d2 < (n // 8) ** 2] = 8
    return m


def gpu_image(n, **kw):
    return rc.render(scene, n, n, depth=D, mode="fast", **kw)


DENSE = {"one": {}, "ssaa4": {"ssaa": 4}, "ssaa8": {"ssaa": 8}, "adapt": {"ssaa": S, "adaptive": T}}
AGAINST = {"u1": ["one"], "u4": ["ssaa4"], "fovea": ["one", "ssaa8"], "roi": ["ssaa4"],
           "amap": ["adapt"]}

lines, records = [], []
for n in SIZES:
    images = {1: gpu_image(n), 2: gpu_image(n, ssaa=2), 4: gpu_image(n, ssaa=4),
              8: gpu_image(n, ssaa=8)}
    roi = np.zeros((n, n), dtype=np.uint8)
    o = (n - 256) // 2 + 1
    roi[o:o + 256, o:o + 256] = 4
    maps = {"u1": np.ones((n, n), dtype=np.uint8), "u4": np.full((n, n), 4, dtype=np.uint8),
            "fovea": fovea(n), "roi": roi,
            "amap": np.where(rc.edge_mask(images[1], T), S, 0).astype(np.uint8)}
    # what a rate frame's buffer holds before it: random bytes; the one-ray image for amap
    bases = {k: np.random.default_rng(n + i).integers(0, 256, size=(n, n, 3), dtype=np.uint8)
             for i, k in enumerate(maps)}
    bases["amap"] = images[1]
    d_maps = {k: torch.from_numpy(m).cuda() for k, m in maps.items()}
    d_bases = {k: torch.from_numpy(np.ascontiguousarray(b)).cuda() for k, b in bases.items()}
    cases = list(DENSE) + list(maps)
    bufs = {k: torch.empty((n, n, 3), dtype=torch.uint8, device="cuda") for k in cases}
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    phases = {k: {"render": [], "refine": []} for k in maps}

    def launch(k):
        tim = {}
        if k in DENSE:
            rc.render_device(scene, n, n, bufs[k].data_ptr(), depth=D, mode="fast", timing=tim,
                             **DENSE[k])
        else:
            bufs[k].copy_(d_bases[k])   # outside the library's events
            torch.cuda.synchronize()
            rc.render_rates_device(scene, n, n, d_maps[k].data_ptr(), bufs[k].data_ptr(),
                                   depth=D, mode="fast", timing=tim)
        return tim["kernel_ms"]

    for r in range(WARM + REPS):
        for k in cases:
            t = launch(k)
            ph = rc.rate_phase_ms() if k in maps else None
            if r >= WARM:
                ms[k].append(t)
                if ph:
                    for name in ph:
                        phases[k][name].append(ph[name])

    rec = {"scene": os.environ.get("SCENE", "quadric"), "n": n, "depth": D, "launches": REPS,
           "version": rc.version(), "dense": {}, "rates": {}}
    rays_dense = {"one": n * n, "ssaa4": 16 * n * n, "ssaa8": 64 * n * n}
    lines.append(f"{n}x{n} depth {D}, {REPS} launches each, medians (max-min) in ms")
    for k in DENSE:
        rec["dense"][k] = {"median": round(med(ms[k]), 4), "spread": round(spread(ms[k]), 4)}
        extra = f"   {med(ms[k]) * 1e6 / rays_dense[k]:.4f} ns/ray" if k in rays_dense else ""
        if k == "adapt":
            extra = f"   s={S} t={T}, {rc.adaptive_stats()['refined_pixels']} refined pixels"
        lines.append(f"  {k:<6} {med(ms[k]):8.4f} ({spread(ms[k]):.4f}){extra}")
    for k in maps:
        launch(k)   # the last launch of the loop was not this case's: its own counts and bytes
        st = rc.rate_stats()
        same = bool((bufs[k].cpu().numpy() == rc.rates_compose(bases[k], images, maps[k])).all())
        sub_rays = st["rays"] - st["pixels"][1]
        refine = med(phases[k]["refine"])
        ratios = {}
        for other in AGAINST[k]:
            apart = abs(med(ms[k]) - med(ms[other])) > spread(ms[k]) + spread(ms[other])
            ratios[other] = {"ratio": round(med(ms[k]) / med(ms[other]), 3),
                             "beyond_spreads": bool(apart)}
        rec["rates"][k] = {
            "total_ms": {"median": round(med(ms[k]), 4), "spread": round(spread(ms[k]), 4)},
            **{name: {"median": round(med(v), 4), "spread": round(spread(v), 4)}
               for name, v in phases[k].items()},
            "pixels": st["pixels"], "rays": st["rays"],
            "refine_ns_per_ray": round(refine * 1e6 / sub_rays, 4) if sub_rays else None,
            "against": ratios, "bytes_equal_compose": same}
        lines.append(
            f"  {k:<6} {med(ms[k]):8.4f} ({spread(ms[k]):.4f})   "
            f"render {med(phases[k]['render']):.4f} ({spread(phases[k]['render']):.4f})  "
            f"refine {refine:.4f} ({spread(phases[k]['refine']):.4f})")
        lines.append(
            f"         pixels {st['pixels']}  rays {st['rays']}  "
            f"refine {refine * 1e6 / max(sub_rays, 1):.4f} ns/ray  " +
            "  ".join(f"x{v['ratio']} of {o}{'' if v['beyond_spreads'] else ' (within spreads)'}"
                      for o, v in ratios.items()) + f"  bytes ok: {same}")
    records.append(rec)
    del bufs, d_maps, d_bases

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
