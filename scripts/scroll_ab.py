"""Scrolling an accumulated view, A/B on one visit: quadric.scene, depth 6, device-resident, the
identity-sized W x H window in the middle of the 4W x 4H virtual image, hier4.  For every size and
every count (1 and 16 samples a pixel) the cases below alternate round by round (REPS rounds after
WARM warm-up rounds), so a drift of the box touches all alike:
  reset / reset'  the whole window accumulated anew, a reset pass of `count` samples through
                  rc_accum_pass_window_device (k_accum_win, unchanged): what a viewer that pans does
                  without the scroll.  Twice a round: the yardstick and its own repeat, whose ratio
                  and spread say what a ratio of this visit can resolve
  move            rc_accum_scroll_device with dx = dy = 0: the move alone, nothing shot
  scroll dx,dy    rc_accum_scroll_device by (1, 1), (16, 0), (0, 16) and (W/2, H/2) into the new
                  window, from a source accumulated through the old one
  dense dx,dy     one reset pass of rc_accum_pass_window_device over a compact window of about as
                  many pixels as that pan exposes: the exposed strip itself where the pan has one
                  direction (the same rays), else W columns by ceil(E / W) rows at the new window's
                  origin (other rays of the same picture): those rays in the dense layout
  even W/2,H/2    the (W/2, H/2) scroll with rc_tuning.adaptive_blocks = EVEN (1024: four workgroups
                  a CU on 256 CUs), the even grid the default avoids: with it the waves' stride is
                  a multiple of W and a wave stays in one column of the window
Kernel times are the library's event spans (rc_timing.kernel_ms; for a scroll also its two phases,
rc_accum_phase_ms: the move and the samples).  Every scroll's destination is compared with the
state `reset` built from scratch, records and bytes.  Prints a table (and writes it to OUT) and
one JSON line per size and count (JSON_OUT).  No ratio is a gate."""
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
COUNTS = [int(v) for v in os.environ.get("COUNTS", "1,16").split(",")]
EVEN = int(os.environ.get("EVEN", "1024"))
SEQ = "hier4"
scene = rc.Scene.from_file(scene_path(os.environ.get("SCENE", "quadric")))


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


def stat(v):
    return {"median": round(med(v), 4), "spread": round(spread(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4)}


def state(w, h):
    return (torch.zeros((h, w, 4), dtype=torch.int16, device="cuda"),
            torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda"))


def reset_pass(window, w, h, count, st, tim=None):
    rc.accum_pass_window_device(scene, window, w, h, SEQ, 0, count, st[0].data_ptr(),
                                st[1].data_ptr(), reset=True, depth=D, mode="fast", timing=tim)


lines, records = [], []
for w, h in SIZES:
    new = (4 * w, 4 * h, 3 * w // 2, 3 * h // 2)
    pans = [(1, 1), (16, 0), (0, 16), (w // 2, h // 2)]
    for count in COUNTS:
        exposed = {p: w * h - (w - p[0]) * (h - p[1]) for p in pans}
        # the compact windows: (window, width, height)
        compact = {}
        for dx, dy in pans:
            if dy == 0:
                compact[(dx, dy)] = ((new[0], new[1], new[2] + w - dx, new[3]), dx, h)
            elif dx == 0:
                compact[(dx, dy)] = ((new[0], new[1], new[2], new[3] + h - dy), w, dy)
            else:
                compact[(dx, dy)] = (new, w, -(-exposed[(dx, dy)] // w))
        full = {k: state(w, h) for k in ("reset", "reset'", "dst")}
        src = {p: state(w, h) for p in pans}
        small = {p: state(compact[p][1], compact[p][2]) for p in pans}
        for p in pans:   # the sources, once: the old window's state
            reset_pass(rc.window_pan(new, -p[0], -p[1]), w, h, count, src[p])
        torch.cuda.synchronize()
        cases = (["reset", "reset'", "move"] + [f"scroll {dx},{dy}" for dx, dy in pans]
                 + [f"dense {dx},{dy}" for dx, dy in pans] + [f"even {w // 2},{h // 2}"])
        phases = {k: ([], []) for k in cases if not k.startswith(("reset", "dense"))}

        def launch(k):
            """The case's kernel time in ms."""
            tim = {}
            if k in ("reset", "reset'"):
                reset_pass(new, w, h, count, full[k], tim)
            elif k.startswith("dense"):
                p = tuple(int(v) for v in k.split()[1].split(","))
                reset_pass(compact[p][0], compact[p][1], compact[p][2], count, small[p], tim)
            else:
                p = (0, 0) if k == "move" else tuple(int(v) for v in k.split()[1].split(","))
                s = full["reset"] if k == "move" else src[p]
                with rc.tuned(adaptive_blocks=EVEN if k.startswith("even") else 0):
                    rc.accum_scroll_device(scene, new, w, h, SEQ, count, p[0], p[1],
                                           s[0].data_ptr(), s[1].data_ptr(),
                                           full["dst"][0].data_ptr(), full["dst"][1].data_ptr(),
                                           depth=D, mode="fast", timing=tim)
                ph = rc.accum_phase_ms()
                phases[k][0].append(ph["mark"])
                phases[k][1].append(ph["shoot"])
                if not (torch.equal(full["dst"][0], full["reset"][0])
                        and torch.equal(full["dst"][1], full["reset"][1])):
                    bytes_ok[k] = False
            return tim["kernel_ms"]

        ms = {k: [] for k in cases}
        bytes_ok = {k: True for k in phases}
        for r in range(WARM + REPS):
            for k in cases:
                t = launch(k)
                if r >= WARM:
                    ms[k].append(t)
        for k in phases:   # the warm-up rounds' spans go
            phases[k] = (phases[k][0][WARM:], phases[k][1][WARM:])

        rays = {"reset": w * h * count, "reset'": w * h * count, "move": 0}
        for p in pans:
            rays[f"scroll {p[0]},{p[1]}"] = exposed[p] * count
            rays[f"dense {p[0]},{p[1]}"] = compact[p][1] * compact[p][2] * count
        rays[f"even {w // 2},{h // 2}"] = exposed[pans[-1]] * count
        rec = {"scene": os.environ.get("SCENE", "quadric"), "w": w, "h": h, "depth": D,
               "count": count, "window": list(new), "launches": REPS, "version": rc.version(),
               "cases": {}, "comparisons": {}}
        lines.append(f"{w}x{h} window at ({new[2]}, {new[3]}) of {new[0]}x{new[1]}, {SEQ}[0..{count}), "
                     f"depth {D}, {REPS} rounds, medians (max-min) in ms")
        for k in cases:
            rec["cases"][k] = {"ms": stat(ms[k]), "rays": rays[k]}
            line = f"  {k:<16} {med(ms[k]):9.4f} ({spread(ms[k]):.4f})   rays {rays[k]:>10}"
            if k in phases:
                mv, sh = phases[k]
                rec["cases"][k].update(move_ms=stat(mv), samples_ms=stat(sh), bytes_ok=bytes_ok[k])
                line += (f"   move {med(mv):.4f} ({spread(mv):.4f})  samples {med(sh):.4f} "
                         f"({spread(sh):.4f})   = reset's state: {bytes_ok[k]}")
            lines.append(line)
        pairs = [("reset'", "reset"), ("move", "reset")]
        for dx, dy in pans:
            pairs += [(f"scroll {dx},{dy}", "reset"), (f"scroll {dx},{dy}", "move"),
                      (f"scroll {dx},{dy}", f"dense {dx},{dy}")]
        pairs.append((f"scroll {w // 2},{h // 2}", f"even {w // 2},{h // 2}"))
        for a, b in pairs:
            rec["comparisons"][f"{a} vs {b}"] = {
                "ratio": round(med(ms[a]) / med(ms[b]), 4),
                "difference_ms": round(med(ms[a]) - med(ms[b]), 4),
                "spread": round(spread(ms[a]), 4), "spread_yardstick": round(spread(ms[b]), 4)}
            lines.append(f"  {a} / {b}: ratio {med(ms[a]) / med(ms[b]):.4f}, difference "
                         f"{med(ms[a]) - med(ms[b]):+.4f} ms (spreads {spread(ms[a]):.4f} and "
                         f"{spread(ms[b]):.4f} ms)")
        records.append(rec)
        print(f"done {w}x{h} count {count}", file=sys.stderr, flush=True)
        del full, src, small

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
