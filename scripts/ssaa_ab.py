"""Supersampling A/B on one visit: quadric.scene, depth 6, fast mode, device-resident, the same
16.8 M rays four ways (kernel time per launch from the library's own events, rc_last_kernel_ms):
  a  k_render at 4096^2 (one ray per pixel: the yardstick)
  b  the fused kernel at 2048^2, ssaa 2
  c  the fused kernel at 1024^2, ssaa 4
  d  two passes at 2048^2, ssaa 2 (k_render at 4096^2, then k_box_down; rc_tuning.ssaa_fused = 0)
The cases alternate launch by launch (REPS rounds after WARM warm-up rounds), so a drift of the
box touches all four alike.  Prints one JSON line (and writes it to OUT): per case the median,
min and max in ms, the spread of (a) (max - min), and whether (b) and (c) are slower than (a)'s
median by more than that spread.  The bytes of b, c and d are checked against the box filter of
a's image."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import torch
from helpers import rc, scene_path

N = int(os.environ.get("SIZE", "4096"))
D = int(os.environ.get("DEPTH", "6"))
REPS = int(os.environ.get("REPS", "30"))
WARM = int(os.environ.get("WARM", "3"))
scene = rc.Scene.from_file(scene_path(os.environ.get("SCENE", "quadric")))

CASES = {"a": (N, 1, 1), "b": (N // 2, 2, 1), "c": (N // 4, 4, 1), "d": (N // 2, 2, 0)}
bufs = {k: torch.empty((n, n, 3), dtype=torch.uint8, device="cuda") for k, (n, _, _) in CASES.items()}
torch.cuda.synchronize()


def launch(k):
    n, s, fused = CASES[k]
    if not fused:
        rc.set_tuning(ssaa_fused=0)
    try:
        rc.render_device(scene, n, n, bufs[k].data_ptr(), depth=D, mode="fast", ssaa=s, timing={})
    finally:
        if not fused:
            rc.set_tuning(ssaa_fused=1)
    return rc.last_kernel_ms()


ms = {k: [] for k in CASES}
for r in range(WARM + REPS):
    for k in CASES:
        t = launch(k)
        if r >= WARM:
            ms[k].append(t)

big = bufs["a"].cpu().numpy()
same = {k: bool((bufs[k].cpu().numpy() == rc.box_downsample(big, CASES[k][1])).all())
        for k in ("b", "c", "d")}
res = {"scene": os.environ.get("SCENE", "quadric"), "size": N, "depth": D, "launches": REPS,
       "ms": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                  "max": round(max(v), 4)} for k, v in ms.items()},
       "bytes_equal_box_of_a": same, "version": rc.version()}
spread = max(ms["a"]) - min(ms["a"])
res["spread_a_ms"] = round(spread, 4)
for k in ("b", "c"):
    res[f"{k}_slower_than_a_beyond_spread"] = bool(
        statistics.median(ms[k]) > statistics.median(ms["a"]) + spread)
line = json.dumps(res)
print(line, flush=True)
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as f:
        f.write(line + "\n")
