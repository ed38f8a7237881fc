"""Reconstruction-filter A/B on one visit: quadric.scene, depth 6, fast mode, device-resident, at
2048^2 with ssaa 2 and at 1024^2 with ssaa 4 (B is 4096^2 both times, 50.3 MB).  Every leg renders
B through the two-pass path and times the second pass alone (rc_filter_phase_ms, HIP events):
  kbox  k_box_down, the plain two-pass path (rc_tuning.ssaa_fused = 0): the parent's filter
  box   k_filter_down with the box taps (halo 0)
  tent  k_filter_down with the tent (halo s/2)
  wide  k_filter_down with a signed 3s-tap vector (halo s)
The legs alternate launch by launch (REPS rounds after WARM warm-up rounds), so a drift of the box
touches all alike.  Prints one JSON line per size (and appends them to OUT): per leg the median,
min and max in ms and the GB/s of B's bytes at the median, kbox's spread (max - min), whether each
k_filter_down leg is slower than kbox's median by more than that spread, and whether the tent is
above twice kbox.  Before the timing the legs' bytes are checked at CHECK^2 (default 250) against
numpy's statement of the contract on the plain kernel's s*CHECK image."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import torch
from helpers import rc, scene_path

D = int(os.environ.get("DEPTH", "6"))
REPS = int(os.environ.get("REPS", "30"))
WARM = int(os.environ.get("WARM", "3"))
CHECK = int(os.environ.get("CHECK", "250"))
SIZES = [(2048, 2), (1024, 4)]
WIDE = {2: [-4, 24, 108, 108, 24, -4],
        4: [-1, -2, 5, 22, 44, 60, 60, 44, 22, 5, -2, -1]}
scene = rc.Scene.from_file(scene_path(os.environ.get("SCENE", "quadric")))


def legs(s):
    return {"kbox": None, "box": rc.filter_box(s), "tent": rc.filter_tent(s), "wide": WIDE[s]}


def launch(n, s, taps, buf):
    if taps is None:
        with rc.tuned(ssaa_fused=0):
            rc.render_device(scene, n, n, buf.data_ptr(), depth=D, mode="fast", ssaa=s, timing={})
    else:
        rc.render_filtered_device(scene, n, n, taps, s, buf.data_ptr(), depth=D, mode="fast",
                                  timing={})
    return rc.filter_phase_ms()


out_path = os.environ.get("OUT")
for n, s in SIZES:
    # the bytes, at a small size
    small = torch.empty((CHECK, CHECK, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    big = rc.render(scene, s * CHECK, s * CHECK, depth=D, mode="fast")
    same = {}
    for k, taps in legs(s).items():
        launch(CHECK, s, taps, small)
        want = rc.filter_downsample(big, s, taps if taps is not None else rc.filter_box(s))
        same[k] = bool((small.cpu().numpy() == want).all())
    buf = torch.empty((n, n, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = {k: [] for k in legs(s)}
    render = []
    for r in range(WARM + REPS):
        for k, taps in legs(s).items():
            t = launch(n, s, taps, buf)
            if r >= WARM:
                ms[k].append(t["filter"])
                render.append(t["render"])
    b_bytes = 3 * (n * s) ** 2
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = max(ms["kbox"]) - min(ms["kbox"])
    res = {"scene": os.environ.get("SCENE", "quadric"), "size": n, "ssaa": s, "depth": D,
           "launches": REPS, "b_megabytes": round(b_bytes / 1e6, 1),
           "render_b_ms_median": round(statistics.median(render), 4),
           "filter_ms": {k: {"median": round(med[k], 4), "min": round(min(v), 4),
                             "max": round(max(v), 4),
                             "b_gb_per_s": round(b_bytes / (med[k] * 1e-3) / 1e9, 1)}
                         for k, v in ms.items()},
           "spread_kbox_ms": round(spread, 4),
           "slower_than_kbox_beyond_spread": {k: bool(med[k] > med["kbox"] + spread)
                                              for k in ("box", "tent", "wide")},
           "tent_over_kbox": round(med["tent"] / med["kbox"], 3),
           "tent_above_twice_kbox": bool(med["tent"] > 2 * med["kbox"]),
           f"bytes_equal_contract_at_{CHECK}": same, "version": rc.version()}
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")
