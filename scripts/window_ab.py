"""Window rendering A/B on one visit: quadric.scene, depth 6, device-resident.  For every size the
cases below alternate round by round (REPS rounds after WARM warm-up rounds), so a drift of the box
touches all alike.  The yardsticks are the unchanged whole-frame kernels of the same visit:
  one / one'     k_render, one ray per pixel (rc_render_device), twice a round: the yardstick and
                 its own repeat, whose ratio and spread say what a ratio of this visit can resolve
  win1           the identity window at s = 1 (k_window)                       against one
  ssaaS / winS   k_render_ssaa (fast, s = 2, 4, 8) and the identity window at s (k_window)
  cudaS / cwinS  cuda mode's two-pass path (k_render_cuda on sW x sH, then k_box_down) and the
                 identity window at s in cuda mode (k_window, fused)
  zoom7:S        the centred W x H window of the 7W x 7H image at s = 1 and 4 against win1 / win4:
                 an origin far from 0 (and other rays: the picture is not the same)
  accum1 / awin1 a one-sample pass after a reset pass: rc_accum_pass_device and the same through
                 the identity window (k_accum and k_accum_win)
and once, whatever the sizes:
  frame4096:4    a 4096 x 4096 frame at s = 4 whole (k_render_ssaa) and as 64 tiles of 512 x 512
                 enqueued on one stream with no wait in between (k_window), both between two
                 events on that stream
Kernel times are the library's event spans (rc_timing.kernel_ms).  Every timed image is checked
against the first round's and the identity windows against the dense kernels' bytes; the tiles
are assembled and compared with the whole frame.  Prints a table (and writes it to OUT) and one
JSON line per size (JSON_OUT).  No ratio is a gate."""
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
POSTER = int(os.environ.get("POSTER", "4096"))
TILE = int(os.environ.get("TILE", "512"))
ZOOM = 7
scene = rc.Scene.from_file(scene_path(os.environ.get("SCENE", "quadric")))

FACTORS = (2, 4, 8)
CASES = (["one", "one'", "win1"] + [f"{p}{s}" for s in FACTORS for p in ("ssaa", "win")]
         + [f"{p}{s}" for s in FACTORS for p in ("cuda", "cwin")]
         + [f"zoom{ZOOM}:1", f"zoom{ZOOM}:4", "accum1", "awin1"])
# window case -> its yardstick
PAIRS = ([("one'", "one"), ("win1", "one")] + [(f"win{s}", f"ssaa{s}") for s in FACTORS]
         + [(f"cwin{s}", f"cuda{s}") for s in FACTORS]
         + [(f"zoom{ZOOM}:1", "win1"), (f"zoom{ZOOM}:4", "win4"), ("awin1", "accum1")])
SAME_BYTES = [p for p in PAIRS if not p[0].startswith("zoom")]


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
    acc = {k: torch.zeros((h, w, 4), dtype=torch.int16, device="cuda") for k in ("accum1", "awin1")}
    torch.cuda.synchronize()
    ident = (w, h, 0, 0)
    zoomed = rc.window_for_zoom(w, h, ZOOM, w // 2, h // 2)

    def launch(k):
        """The case's kernel time in ms."""
        tim = {}
        if k in ("one", "one'"):
            rc.render_device(scene, w, h, img[k].data_ptr(), depth=D, mode="fast", timing=tim)
        elif k.startswith("ssaa") or k.startswith("cuda"):
            rc.render_device(scene, w, h, img[k].data_ptr(), depth=D, ssaa=int(k[4:]),
                             mode="fast" if k.startswith("ssaa") else "cuda", timing=tim)
        elif k.startswith("win") or k.startswith("cwin"):
            rc.render_window_device(scene, ident, w, h, img[k].data_ptr(), ssaa=int(k[-1]),
                                    depth=D, mode="fast" if k.startswith("win") else "cuda",
                                    timing=tim)
        elif k.startswith("zoom"):
            rc.render_window_device(scene, zoomed, w, h, img[k].data_ptr(), ssaa=int(k[-1]),
                                    depth=D, mode="fast", timing=tim)
        elif k == "accum1":
            rc.accum_pass_device(scene, w, h, "hier8", 0, 1, acc[k].data_ptr(), img[k].data_ptr(),
                                 reset=True, depth=D, mode="fast")
            rc.accum_pass_device(scene, w, h, "hier8", 1, 1, acc[k].data_ptr(), img[k].data_ptr(),
                                 depth=D, mode="fast", timing=tim)
        else:
            rc.accum_pass_window_device(scene, ident, w, h, "hier8", 0, 1, acc[k].data_ptr(),
                                        img[k].data_ptr(), reset=True, depth=D, mode="fast")
            rc.accum_pass_window_device(scene, ident, w, h, "hier8", 1, 1, acc[k].data_ptr(),
                                        img[k].data_ptr(), depth=D, mode="fast", timing=tim)
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
    ok["awin1"] = ok["awin1"] and bool(torch.equal(acc["awin1"], acc["accum1"]))

    rays = {k: w * h for k in CASES}
    for k in CASES:
        if k[-1] in "248" and not k.startswith("a"):
            rays[k] = w * h * int(k[-1]) ** 2
    rec = {"scene": os.environ.get("SCENE", "quadric"), "w": w, "h": h, "depth": D,
           "launches": REPS, "version": rc.version(), "zoom_window": list(zoomed), "cases": {},
           "comparisons": {}}
    lines.append(f"{w}x{h} depth {D}, {REPS} rounds, medians (max-min) in ms")
    for k in CASES:
        rec["cases"][k] = {"ms": stat(ms[k]), "rays": rays[k],
                           "ns_per_ray": round(med(ms[k]) * 1e6 / rays[k], 4),
                           "same_every_round": same[k], "bytes_ok": ok.get(k)}
        line = (f"  {k:<8} {med(ms[k]):8.4f} ({spread(ms[k]):.4f})   rays {rays[k]:>10}   "
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
    del img, acc, first

# a poster frame whole and in tiles, both between two events of one stream
P, S = POSTER, 4
tiles = rc.window_tiles(P, P, TILE, TILE)
stream = torch.cuda.Stream()
whole = torch.zeros((P, P, 3), dtype=torch.uint8, device="cuda")
bufs = [torch.zeros((th, tw, 3), dtype=torch.uint8, device="cuda") for _, tw, th in tiles]
torch.cuda.synchronize()
ms = {"whole": [], "tiles": []}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def render_whole():
    rc.render_device(scene, P, P, whole.data_ptr(), stream_ptr=stream.cuda_stream, depth=D,
                     mode="fast", ssaa=S)


def render_tiles():
    for (win, tw, th), buf in zip(tiles, bufs):
        rc.render_window_device(scene, win, tw, th, buf.data_ptr(), ssaa=S,
                                stream_ptr=stream.cuda_stream, depth=D, mode="fast")


for r in range(WARM + REPS):
    for k, fn in (("whole", render_whole), ("tiles", render_tiles)):
        t = timed(fn)
        if r >= WARM:
            ms[k].append(t)
torch.cuda.synchronize()
tiles_ok = all(bool(torch.equal(buf, whole[win[3]:win[3] + th, win[2]:win[2] + tw]))
               for (win, tw, th), buf in zip(tiles, bufs))
lines.append(f"{P}x{P} at s = {S}, depth {D}, {REPS} rounds, stream events, medians (max-min) in ms")
lines.append(f"  whole    {med(ms['whole']):8.4f} ({spread(ms['whole']):.4f})")
lines.append(f"  {len(tiles)} tiles of {TILE}x{TILE} {med(ms['tiles']):8.4f} "
             f"({spread(ms['tiles']):.4f})   assembled = whole: {tiles_ok}")
lines.append(f"  tiles / whole: ratio {med(ms['tiles']) / med(ms['whole']):.4f}, difference "
             f"{med(ms['tiles']) - med(ms['whole']):+.4f} ms")
records.append({"poster": P, "s": S, "tile": TILE, "tiles": len(tiles), "whole_ms": stat(ms["whole"]),
                "tiles_ms": stat(ms["tiles"]), "tiles_ok": tiles_ok,
                "ratio": round(med(ms["tiles"]) / med(ms["whole"]), 4)})

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
