"""Ambient occlusion and any-hit queries A/B on one visit: quadric.scene, a moved camera,
device-resident.
   PARENT=<a built checkout of the parent commit> python3 scripts/ao_ab.py
The builds under test run in child processes of their own, one after the other and PASSES times
round robin, so a drift of the box touches all alike; inside a child the cases alternate round by
round (REPS rounds after WARM warm-up rounds).  Builds:
  new      this tree's libraycast_hip.so
  parent   PARENT's libraycast_hip.so through PARENT's own Python package
Cases, each per size:
  yard16       the parent commit's way to an occlusion plane of 16 directions, in both builds: the
               camera's rays as one batch through rc_trace_rays_from_device with records and frames,
               then 16 batches with records only, one a direction, over the HIT pixels' rays, which
               are prepared beforehand on the device.  Preparing the rays (the flip, the compaction
               to the hit pixels) and reducing the records are not timed, which favours this way;
               and its rays go with skip = -1 (the entry has no other), so its counts are not quite
               the contract's.  The sum of the 17 kernel spans.
  rays1        the first of those 16 batches alone: k_rays_from with records only
The new build adds:
  ao16 / ao16t one reset pass of rc_ao_pass_device with ao_dirs(16), tmax inf / 2.0, bytes stored
  ao64         the same with ao_dirs(64), tmax inf
  ao1          the same with ao_dirs(1), tmax inf
  frame        k_camera's one-ray frame through the same camera (rc_render_camera_device)
  gbuf         the G-buffer's id + t planes (rc_render_gbuffer_device; the reference camera at the
               origin: the G-buffer takes no other)
  occ1         rays1's rays through rc_occluded_rays_device, skip = the hit shape, tmax inf
  resolve      rc_ao_resolve_device on ao16's state, 10 launches between two stream events
  copy         a device copy of the state's bytes (4 in, 4 out a pixel), timed the same way
Kernel times are the library's event spans (rc_timing.kernel_ms, rc_view_phase_ms).  Every timed
state (records and bytes) is checked against the first round's.  Prints a table (and writes it to
OUT).  No ratio is a gate."""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
D = int(os.environ.get("DEPTH", "6"))
REPS = int(os.environ.get("REPS", "20"))
WARM = int(os.environ.get("WARM", "3"))
PASSES = int(os.environ.get("PASSES", "2"))
SIZES = [tuple(int(v) for v in c.split("x"))
         for c in os.environ.get("SIZES", "1024x1024,2048x2048").split(",")]
MOVED = (0.5, 0.25, 1.0)
OLD = ["yard16", "rays1"]
NEW = ["ao16", "ao16t", "ao64", "ao1", "frame", "gbuf", "occ1", "resolve", "copy"]
NDIRS = 16


def spiral(n):
    """rc.ao_dirs(n)'s directions, for the parent's package too (float64, rounded once)."""
    import numpy as np
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)


def child():
    """One build: {"WxH": {case: [ms, ...]}, ...} and the state checks, as one JSON line."""
    sys.path.insert(0, os.path.join(os.environ.get("AO_AB_TREE", os.path.join(HERE, "..")),
                                    "tests"))
    import numpy as np
    import torch
    from helpers import rc, scene_path

    scene = rc.Scene.from_file(scene_path(os.environ.get("SCENE", "quadric")))
    new = hasattr(rc, "ao_pass_device")
    cases = OLD + (NEW if new else [])
    u16 = spiral(NDIRS)
    out = {"version": rc.version(), "sizes": {}}
    for w, h in SIZES:
        n = w * h
        # the camera's rays and, once, their primary hits: what the yardstick's rays are made of
        d = rc.view_dirs(scene.js.camera_width, scene.js.camera_height, (w, h),
                         rc.view_grid(w, h), rc.view_identity())
        d_dirs = torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).cuda()
        d_eye = torch.tensor(MOVED, dtype=torch.float32, device="cuda").repeat(n, 1).contiguous()
        d_hits = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rc.trace_rays_from_device(scene, n, d_eye.data_ptr(), d_dirs.data_ptr(),
                                  d_hits_ptr=d_hits.data_ptr(), frame=True, depth=D)
        torch.cuda.synchronize()
        ids = d_hits[:, 0].contiguous().view(torch.int32)
        hit = ids >= 0
        nh = int(hit.sum())
        P = d_hits[hit][:, 2:5].contiguous()
        N = d_hits[hit][:, 5:8].contiguous()
        skip = ids[hit].contiguous()
        rays = []
        for j in range(NDIRS):   # the contract's flip, in torch: prepared beforehand, not timed
            uj = torch.from_numpy(u16[j]).cuda()
            dot = (N[:, 0] * uj[0] + N[:, 1] * uj[1]) + N[:, 2] * uj[2]
            rays.append(torch.where((dot < 0)[:, None], uj * -1.0, uj).contiguous())
        d_rec = torch.zeros((nh, 8), dtype=torch.float32, device="cuda")
        img = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        st = {k: (torch.zeros((h, w), dtype=torch.int32, device="cuda"),
                  torch.zeros((h, w), dtype=torch.uint8, device="cuda"))
              for k in ("ao16", "ao16t", "ao64", "ao1")}
        planes = (torch.zeros((h, w), dtype=torch.int32, device="cuda"),
                  torch.zeros((h, w), dtype=torch.float32, device="cuda"))
        flags = torch.zeros((nh,), dtype=torch.uint8, device="cuda")
        res = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        cpy = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def batch(origins, dirs, count, hits, frame):
            rc.trace_rays_from_device(scene, count, origins.data_ptr(), dirs.data_ptr(),
                                      d_hits_ptr=hits.data_ptr(), frame=frame, depth=D)
            return rc.view_phase_ms()["kernel"]

        def timed(fn, *args, **kw):
            tim = {}
            fn(*args, timing=tim, **kw)
            return tim["kernel_ms"]

        def between_events(fn, reps=10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / reps

        def ao(k, nd, tmax):
            return timed(rc.ao_pass_device, scene, MOVED, None, w, h, (spiral(nd), tmax),
                         st[k][0].data_ptr(), st[k][1].data_ptr(), reset=True, depth=D)

        def launch(k):
            if k == "yard16":
                t = batch(d_eye, d_dirs, n, d_hits, True)
                for j in range(NDIRS):
                    t += batch(P, rays[j], nh, d_rec, False)
                return t
            if k == "rays1":
                return batch(P, rays[0], nh, d_rec, False)
            if k == "ao16":
                return ao(k, 16, float("inf"))
            if k == "ao16t":
                return ao(k, 16, 2.0)
            if k == "ao64":
                return ao(k, 64, float("inf"))
            if k == "ao1":
                return ao(k, 1, float("inf"))
            if k == "frame":
                return timed(rc.render_camera_device, scene, MOVED, None, w, h, img.data_ptr(),
                             depth=D)
            if k == "gbuf":
                return timed(rc.render_gbuffer_device, scene, w, h, d_id_ptr=planes[0].data_ptr(),
                             d_t_ptr=planes[1].data_ptr())
            if k == "occ1":
                return timed(rc.occluded_rays_device, scene, nh, P.data_ptr(), rays[0].data_ptr(),
                             flags.data_ptr(), d_skip_ptr=skip.data_ptr(), depth=D)
            s = torch.cuda.current_stream().cuda_stream
            if k == "resolve":
                return between_events(lambda: rc.ao_resolve_device(st["ao16"][0].data_ptr(), w, h,
                                                                   res.data_ptr(), stream_ptr=s))
            return between_events(lambda: cpy.copy_(st["ao16"][0]))

        def state_of(k):
            if k in st:
                return list(st[k])
            return {"yard16": [d_hits, d_rec], "rays1": [d_rec], "frame": [img],
                    "gbuf": list(planes), "occ1": [flags], "resolve": [res], "copy": [cpy]}[k]

        ms = {k: [] for k in cases}
        first, same = {}, {k: True for k in cases}
        for r in range(WARM + REPS):
            for k in cases:
                t = launch(k)
                torch.cuda.synchronize()
                if r >= WARM:
                    ms[k].append(t)
                state = state_of(k)   # every timed state against the first round's
                if k not in first:
                    first[k] = [s.clone() for s in state]
                else:
                    for i, (s, f) in enumerate(zip(state, first[k])):
                        bad = int((s.view(torch.uint8) != f.view(torch.uint8)).sum())
                        if bad and same[k] is True:   # the first difference, in words
                            same[k] = f"False (round {r}, tensor {i}: {bad} bytes differ)"
        ok = {"hit_pixels": nh}
        if new:
            ok["resolve==ao16 bytes"] = bool(torch.equal(res, st["ao16"][1]))
            ok["copy==ao16 state"] = bool(torch.equal(cpy, st["ao16"][0]))
            blocked = int(flags.sum())
            # occ1's rays are direction 0 of the 16: a pass with that one direction counts the same
            rc.ao_pass_device(scene, MOVED, None, w, h, (u16[:1], float("inf")),
                              st["ao1"][0].data_ptr(), reset=True, depth=D)
            ok["occ1==k_ao blocked"] = bool(rc.ao_stats()["blocked"] == blocked)
            ok["ao16t opens more"] = bool(int((st["ao16t"][0] & 0xffff).sum()) >
                                          int((st["ao16"][0] & 0xffff).sum()))
        out["sizes"][f"{w}x{h}"] = {"ms": ms, "same_every_round": same, "states_ok": ok}
        del d_dirs, d_eye, d_hits, rays, d_rec, st, first
    print("AO_AB " + json.dumps(out), flush=True)


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


def main():
    builds = [("new", None)]
    if os.environ.get("PARENT"):
        builds.append(("parent", os.environ["PARENT"]))
    runs = {b[0]: [] for b in builds}
    for _ in range(PASSES):
        for name, tree in builds:
            env = dict(os.environ)
            if tree:
                env["AO_AB_TREE"] = tree
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env,
                               stdout=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"the {name} build's child ended with {p.returncode}")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("AO_AB ")][-1]
            runs[name].append(json.loads(line[len("AO_AB "):]))

    lines = [f"{name}: {runs[name][0]['version']}" for name, _ in builds]
    for w, h in SIZES:
        key = f"{w}x{h}"
        lines.append(f"{key} depth {D}, {PASSES} passes of {REPS} rounds a build, medians "
                     f"(max-min) in ms over all of a build's rounds; per pass in brackets")
        ms = {}
        for name, _ in builds:
            for k in runs[name][0]["sizes"][key]["ms"]:
                per = [r["sizes"][key]["ms"][k] for r in runs[name]]
                allv = [x for p in per for x in p]
                ms[name, k] = allv
                notes = [r["sizes"][key]["same_every_round"][k] for r in runs[name]]
                same = next((v for v in notes if v is not True), True)
                lines.append(f"  {name:<8}{k:<9}{med(allv):9.4f} ({spread(allv):.4f})  "
                             f"[{', '.join(f'{med(p):.4f}' for p in per)}]   "
                             f"same every round: {same}")
            ok = {}
            for r in runs[name]:
                for k, v in r["sizes"][key]["states_ok"].items():
                    ok[k] = v if isinstance(v, int) and not isinstance(v, bool) else (
                        ok.get(k, True) and v)
            lines.append(f"  {name:<8}states: {ok}")

        def ratio(a, b, what):
            if a in ms and b in ms:
                lines.append(f"  {what}: {a[0]} {a[1]} / {b[0]} {b[1]} = "
                             f"{med(ms[a]) / med(ms[b]):.4f}, difference "
                             f"{med(ms[a]) - med(ms[b]):+.4f} ms (spreads {spread(ms[a]):.4f} and "
                             f"{spread(ms[b]):.4f} ms)")

        ratio(("new", "yard16"), ("parent", "yard16"),
              "what a ratio between two processes resolves (the same kernels in both)")
        ratio(("new", "ao16"), ("parent", "yard16"), "1. k_ao, 16 directions, tmax inf, over the parent's way")
        ratio(("new", "ao16t"), ("parent", "yard16"), "1. k_ao, 16 directions, tmax 2.0, over the parent's way")
        ratio(("new", "ao16"), ("new", "yard16"), "1'. the same within the new build")
        ratio(("new", "ao1"), ("new", "frame"), "2. k_ao with one direction over k_camera's one-ray frame")
        ratio(("new", "ao1"), ("new", "gbuf"), "2. k_ao with one direction over the G-buffer's id + t")
        ratio(("new", "ao64"), ("new", "ao16"), "3. 64 directions over 16")
        ratio(("new", "occ1"), ("new", "rays1"), "4. k_occluded_rays over k_rays_from with records only")
        ratio(("new", "resolve"), ("new", "copy"), "5. k_ao_resolve over a device copy of the state")
    table = "\n".join(lines)
    print(table, flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    child() if sys.argv[1:] == ["--child"] else main()
