"""G-buffer A/B on one visit: quadric.scene, device-resident, fast and cuda mode.  For every size the
cases below alternate round by round (REPS rounds after WARM warm-up rounds), so a drift of the box
touches all alike.  The yardstick is the unchanged whole-frame kernel of the same visit:
  one / one'   k_render (cuda: k_render_cuda), one ray per pixel at depth D (rc_render_device),
               twice a round: the yardstick and its own repeat, whose ratio and spread say what a
               ratio of this visit can resolve
  idt          the id and t planes of the whole image (k_gbuffer, 8 bytes a pixel)   against one
  all4         id, t, P and N (fast mode only; 32 bytes a pixel)                     against one
These four are the library's event spans (rc_timing.kernel_ms).  The cases below have no span of
their own or are several kernels, so they are timed between two events on one stream, with a
yardstick timed the same way:
  one_ev       the one-ray frame again, between stream events
  copy         a device copy of the id plane (4 bytes read and 4 written a pixel): the copy
               roofline the memory-bound kernels are held against
  edge         k_id_edge_rates over the id plane (4 bytes read, 1 written a pixel)
  geo4         the geometric-edge frame: rc_render_gbuffer_device (id), rc_id_edge_rates_device
               (s = 4, base = 1), rc_render_rates_device, three enqueues with no host wait
  adapt4       adaptive supersampling, ssaa = 4 at threshold 16 (rc_render_device)
  ssaa4        full supersampling, ssaa = 4
with the share of the pixels each of the last three refines.  Every timed output is checked against
the first round's.  Prints a table (and writes it to OUT) and one JSON line per size and mode
(JSON_OUT).  No ratio is a gate."""
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
         for c in os.environ.get("SIZES", "1024x1024,4096x4096").split(",")]
MODES = os.environ.get("MODES", "fast,cuda").split(",")
THRESHOLD = 16
scene = rc.Scene.from_file(scene_path(os.environ.get("SCENE", "quadric")))

SPAN_CASES = ["one", "one'", "idt", "all4"]
EVENT_CASES = ["one_ev", "copy", "edge", "geo4", "adapt4", "ssaa4"]
PAIRS = [("one'", "one"), ("idt", "one"), ("all4", "one"), ("edge", "copy"), ("geo4", "one_ev"),
         ("adapt4", "one_ev"), ("ssaa4", "one_ev"), ("geo4", "adapt4"), ("geo4", "ssaa4")]
BYTES = {"idt": 8, "all4": 32, "copy": 8, "edge": 5}      # a pixel, for the GB/s column


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


def stat(v):
    return {"median": round(med(v), 4), "spread": round(spread(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4)}


lines, records = [], []
stream = torch.cuda.Stream()
sp = stream.cuda_stream
for (w, h), mode in ((s, m) for s in SIZES for m in MODES):
    cases = [k for k in SPAN_CASES + EVENT_CASES if not (k == "all4" and mode == "cuda")]
    img = {k: torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
           for k in ("one", "one'", "one_ev", "geo4", "adapt4", "ssaa4")}
    ids = {k: torch.zeros((h, w), dtype=torch.int32, device="cuda")
           for k in ("idt", "all4", "geo4", "copy")}
    ts = {k: torch.zeros((h, w), dtype=torch.float32, device="cuda") for k in ("idt", "all4")}
    pn = {k: torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") for k in ("P", "N")}
    rates = {k: torch.zeros((h, w), dtype=torch.uint8, device="cuda") for k in ("edge", "geo4")}
    torch.cuda.synchronize()
    refined = {}

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def launch(k):
        """The case's time in ms: the library's kernel span, or stream events."""
        tim = {}
        if k in ("one", "one'"):
            rc.render_device(scene, w, h, img[k].data_ptr(), depth=D, mode=mode, timing=tim)
        elif k == "idt":
            rc.render_gbuffer_device(scene, w, h, d_id_ptr=ids[k].data_ptr(),
                                     d_t_ptr=ts[k].data_ptr(), mode=mode, timing=tim)
        elif k == "all4":
            rc.render_gbuffer_device(scene, w, h, d_id_ptr=ids[k].data_ptr(),
                                     d_t_ptr=ts[k].data_ptr(), d_p_ptr=pn["P"].data_ptr(),
                                     d_n_ptr=pn["N"].data_ptr(), mode=mode, timing=tim)
        elif k == "one_ev":
            return events(lambda: rc.render_device(scene, w, h, img[k].data_ptr(), stream_ptr=sp,
                                                   depth=D, mode=mode))
        elif k == "copy":
            with torch.cuda.stream(stream):
                return events(lambda: ids["copy"].copy_(ids["idt"]))
        elif k == "edge":
            return events(lambda: rc.id_edge_rates_device(ids["idt"].data_ptr(), w, h, 4,
                                                          rates[k].data_ptr(), stream_ptr=sp))
        elif k == "geo4":
            def frame():
                rc.render_gbuffer_device(scene, w, h, d_id_ptr=ids[k].data_ptr(), stream_ptr=sp,
                                         mode=mode)
                rc.id_edge_rates_device(ids[k].data_ptr(), w, h, 4, rates[k].data_ptr(),
                                        stream_ptr=sp)
                rc.render_rates_device(scene, w, h, rates[k].data_ptr(), img[k].data_ptr(),
                                       stream_ptr=sp, depth=D, mode=mode)
            return events(frame)
        elif k == "adapt4":
            return events(lambda: rc.render_device(scene, w, h, img[k].data_ptr(), stream_ptr=sp,
                                                   depth=D, mode=mode, ssaa=4, adaptive=THRESHOLD))
        else:
            return events(lambda: rc.render_device(scene, w, h, img[k].data_ptr(), stream_ptr=sp,
                                                   depth=D, mode=mode, ssaa=4))
        return tim["kernel_ms"]

    def outputs(k):
        """What the case wrote, for the comparison with the first round."""
        if k in img:
            out = [img[k]]
            if k == "geo4":
                out += [ids[k], rates[k]]
            return out
        if k == "idt":
            return [ids[k], ts[k]]
        if k == "all4":
            return [ids[k], ts[k], pn["P"], pn["N"]]
        return [ids["copy"]] if k == "copy" else [rates[k]]

    ms = {k: [] for k in cases}
    first, same = {}, {k: True for k in cases}
    for r in range(WARM + REPS):
        for k in cases:
            t = launch(k)
            if r >= WARM:
                ms[k].append(t)
        torch.cuda.synchronize()
        for k in cases:   # every timed output against the first round's
            if k not in first:
                first[k] = [o.clone() for o in outputs(k)]
            elif not all(torch.equal(o, f) for o, f in zip(outputs(k), first[k])):
                same[k] = False
    pixels = w * h
    refined["geo4"] = int((rates["geo4"] == 4).sum().item()) / pixels
    rc.render_device(scene, w, h, img["adapt4"].data_ptr(), depth=D, mode=mode, ssaa=4,
                     adaptive=THRESHOLD, timing={})
    refined["adapt4"] = rc.adaptive_stats()["refined_pixels"] / pixels
    refined["ssaa4"] = 1.0
    ok = {"idt": bool(torch.equal(ids["idt"], ids["geo4"])),
          "edge": bool(torch.equal(rates["edge"], rates["geo4"])),
          "one'": bool(torch.equal(img["one'"], img["one"])),
          "one_ev": bool(torch.equal(img["one_ev"], img["one"]))}
    if "all4" in cases:
        ok["all4"] = bool(torch.equal(ids["all4"], ids["idt"]) and torch.equal(ts["all4"], ts["idt"]))
    miss = int((ids["idt"] < 0).sum().item()) / pixels

    rec = {"scene": os.environ.get("SCENE", "quadric"), "w": w, "h": h, "mode": mode, "depth": D,
           "launches": REPS, "version": rc.version(), "miss_share": round(miss, 4), "cases": {},
           "comparisons": {}}
    lines.append(f"{w}x{h} {mode} depth {D}, {REPS} rounds, medians (max-min) in ms; "
                 f"{100 * miss:.1f} % of the pixels miss")
    for k in cases:
        c = {"ms": stat(ms[k]), "same_every_round": same[k], "bytes_ok": ok.get(k)}
        line = f"  {k:<7} {med(ms[k]):9.4f} ({spread(ms[k]):.4f})   same every round: {same[k]}"
        if k in ok:
            line += f"   bytes ok: {ok[k]}"
        if k in BYTES:
            c["gb_per_s"] = round(BYTES[k] * pixels / med(ms[k]) / 1e6, 1)
            line += f"   {BYTES[k]} B/pixel, {c['gb_per_s']} GB/s"
        if k in refined:
            c["refined_share"] = round(refined[k], 4)
            line += f"   refines {100 * refined[k]:.1f} % of the pixels"
        rec["cases"][k] = c
        lines.append(line)
    for a, b in PAIRS:
        if a not in cases or b not in cases:
            continue
        rec["comparisons"][f"{a}_vs_{b}"] = {
            "ratio": round(med(ms[a]) / med(ms[b]), 4),
            "difference_ms": round(med(ms[a]) - med(ms[b]), 4), "spread": round(spread(ms[a]), 4),
            "spread_yardstick": round(spread(ms[b]), 4)}
        lines.append(f"  {a} / {b}: ratio {med(ms[a]) / med(ms[b]):.4f}, difference "
                     f"{med(ms[a]) - med(ms[b]):+.4f} ms (spreads {spread(ms[a]):.4f} and "
                     f"{spread(ms[b]):.4f} ms)")
    records.append(rec)
    del img, ids, ts, pn, rates, first

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
