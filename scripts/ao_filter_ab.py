"""The guided filter, the camera's G-buffer and the ambient compose A/B on one visit: quadric.scene,
a moved camera, device-resident.
   make filter-variants && python3 scripts/ao_filter_ab.py
The builds under test run in child processes of their own, one after the other and PASSES times
round robin, so a drift of the box touches all alike; inside a child the cases alternate round by
round (REPS rounds after WARM warm-up rounds).  Builds:
  lds      this tree's libraycast_hip.so: k_ao_filter with the tile and its halo staged in LDS
  direct   libraycast_hip_aofdirect.so: the neighbours read from global memory through the caches
Cases, each per size, on the state of one reset pass with ao_dirs(16) and the camera's guide:
  filt1 / filt3 / filt8   rc_ao_filter_device with the tent of radius 1, 3, 8 (nmin 0.9, dplane 0.05)
  copy33   a device copy that moves the filter's 33 bytes a pixel (16.5 in, 16.5 out)
  ao16 / ao1              one reset pass of rc_ao_pass_device with 16 directions / one
  cgbuf    rc_render_camera_gbuffer_device, id + P + N (what the filter reads), the moved eye
  cgbuf0   the same with all four planes at eye +0;  gbuf0: rc_render_gbuffer_device, four planes
  compose  rc_ao_compose_device out of place;  copy11: a device copy that moves its 11 bytes a pixel
filt*, compose and the copies are 10 launches between two events on a stream of the script's own
(not torch's default stream: its null pointer would send the launches to the library's stream
and the events would bracket nothing); the others are the library's event spans
(rc_timing.kernel_ms).  Every timed output is checked against the first
round's, and the two builds' filtered planes against each other (their checksums are printed).
Prints a table (and writes it to OUT).  No ratio is a gate."""
import json
import os
import statistics
import subprocess
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
D = int(os.environ.get("DEPTH", "6"))
REPS = int(os.environ.get("REPS", "20"))
WARM = int(os.environ.get("WARM", "3"))
PASSES = int(os.environ.get("PASSES", "2"))
SIZES = [tuple(int(v) for v in c.split("x"))
         for c in os.environ.get("SIZES", "1024x1024,2048x2048").split(",")]
MOVED = (0.5, 0.25, 1.0)
CASES = ["filt1", "filt3", "filt8", "copy33", "ao16", "ao1", "cgbuf", "cgbuf0", "gbuf0", "compose",
         "copy11"]
AMBIENT = (0.2, 0.3, 0.4)


def child():
    """One build: {"WxH": {case: [ms, ...]}, ...} and the output checks, as one JSON line."""
    sys.path.insert(0, os.path.join(HERE, "..", "tests"))
    import torch
    from helpers import rc, scene_path

    scene = rc.Scene.from_file(scene_path(os.environ.get("SCENE", "quadric")))
    out = {"version": rc.version(), "sizes": {}}
    for w, h in SIZES:
        n = w * h
        z = lambda count, dt: torch.zeros((count,), dtype=dt, device="cuda")
        ao, byte = z(n, torch.int32), z(n, torch.uint8)
        ao1 = z(n, torch.int32)
        gid, gt, gp, gn = z(n, torch.int32), z(n, torch.float32), z(3 * n, torch.float32), \
            z(3 * n, torch.float32)
        oid, ot, op, on = z(n, torch.int32), z(n, torch.float32), z(3 * n, torch.float32), \
            z(3 * n, torch.float32)
        planes = {r: z(n, torch.uint8) for r in (1, 3, 8)}
        img_in, img = z(3 * n, torch.uint8), z(3 * n, torch.uint8)
        c33a, c33b = z(n * 33 // 2, torch.uint8), z(n * 33 // 2, torch.uint8)
        c11a, c11b = z(n * 11 // 2, torch.uint8), z(n * 11 // 2, torch.uint8)
        filt = {r: rc.ao_filter_params(r, "tent") for r in (1, 3, 8)}
        torch.cuda.synchronize()

        def timed(fn, *args, **kw):
            tim = {}
            fn(*args, timing=tim, **kw)
            return tim["kernel_ms"]

        # a stream of the script's own: torch's default stream is the null pointer, which the
        # library reads as "my own stream", and events on another stream would bracket nothing
        own = torch.cuda.Stream()
        s = own.cuda_stream

        def between_events(fn, reps=10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(own):
                a.record(own)
                for _ in range(reps):
                    fn()
                b.record(own)
            b.synchronize()
            return a.elapsed_time(b) / reps

        # the inputs: one reset pass with 16 directions, the camera's guide, the camera's image
        rc.ao_pass_device(scene, MOVED, None, w, h, rc.ao_dirs(16), ao.data_ptr(), reset=True,
                          depth=D)
        rc.render_camera_gbuffer_device(scene, MOVED, None, w, h, d_id_ptr=gid.data_ptr(),
                                        d_p_ptr=gp.data_ptr(), d_n_ptr=gn.data_ptr())
        torch.cuda.synchronize()

        def launch(k):
            if k.startswith("filt"):
                r = int(k[4:])
                return between_events(lambda: rc.ao_filter_device(
                    ao.data_ptr(), gid.data_ptr(), gp.data_ptr(), gn.data_ptr(), w, h, filt[r],
                    planes[r].data_ptr(), stream_ptr=s))
            if k == "copy33":
                return between_events(lambda: c33b.copy_(c33a))
            if k == "copy11":
                return between_events(lambda: c11b.copy_(c11a))
            if k == "ao16":
                return timed(rc.ao_pass_device, scene, MOVED, None, w, h, rc.ao_dirs(16),
                             ao.data_ptr(), byte.data_ptr(), reset=True, depth=D)
            if k == "ao1":
                return timed(rc.ao_pass_device, scene, MOVED, None, w, h, rc.ao_dirs(1),
                             ao1.data_ptr(), byte.data_ptr(), reset=True, depth=D)
            if k == "cgbuf":
                return timed(rc.render_camera_gbuffer_device, scene, MOVED, None, w, h,
                             d_id_ptr=gid.data_ptr(), d_p_ptr=gp.data_ptr(), d_n_ptr=gn.data_ptr())
            if k == "cgbuf0":
                return timed(rc.render_camera_gbuffer_device, scene, (0.0, 0.0, 0.0), None, w, h,
                             d_id_ptr=oid.data_ptr(), d_t_ptr=ot.data_ptr(), d_p_ptr=op.data_ptr(),
                             d_n_ptr=on.data_ptr())
            if k == "gbuf0":
                return timed(rc.render_gbuffer_device, scene, w, h, d_id_ptr=oid.data_ptr(),
                             d_t_ptr=ot.data_ptr(), d_p_ptr=op.data_ptr(), d_n_ptr=on.data_ptr())
            return between_events(lambda: rc.ao_compose_device(
                scene, gid.data_ptr(), planes[3].data_ptr(), AMBIENT, img_in.data_ptr(),
                img.data_ptr(), w, h, stream_ptr=s))

        def state_of(k):
            if k.startswith("filt"):
                return [planes[int(k[4:])]]
            return {"copy33": [c33b], "copy11": [c11b], "ao16": [ao, byte], "ao1": [ao1],
                    "cgbuf": [gid, gp, gn], "cgbuf0": [oid, ot, op, on],
                    "gbuf0": [oid, ot, op, on], "compose": [img]}[k]

        ms = {k: [] for k in CASES}
        first, same = {}, {k: True for k in CASES}
        for r in range(WARM + REPS):
            for k in CASES:
                t = launch(k)
                torch.cuda.synchronize()
                if r >= WARM:
                    ms[k].append(t)
                state = state_of(k)
                if k not in first:
                    first[k] = [x.clone() for x in state]
                else:
                    for i, (x, f) in enumerate(zip(state, first[k])):
                        bad = int((x.view(torch.uint8) != f.view(torch.uint8)).sum())
                        if bad and same[k] is True:
                            same[k] = f"False (round {r}, tensor {i}: {bad} bytes differ)"
        plain = torch.zeros_like(byte)
        rc.ao_resolve_device(ao.data_ptr(), w, h, plain.data_ptr())
        torch.cuda.synchronize()
        ok = {"hit_pixels": int((gid >= 0).sum())}
        for r in (1, 3, 8):
            ok[f"crc filt{r}"] = zlib.crc32(planes[r].cpu().numpy().tobytes())
            ok[f"filt{r} changes a share of"] = round(float((planes[r] != plain).sum()) / n, 4)
        ok["crc compose"] = zlib.crc32(img.cpu().numpy().tobytes())
        out["sizes"][f"{w}x{h}"] = {"ms": ms, "same_every_round": same, "states_ok": ok}
    print("AO_FILTER_AB " + json.dumps(out), flush=True)


def med(v):
    return statistics.median(v)


def spread(v):
    return max(v) - min(v)


def main():
    builds = [("lds", None), ("direct", "libraycast_hip_aofdirect.so")]
    runs = {b[0]: [] for b in builds}
    for _ in range(PASSES):
        for name, lib in builds:
            env = dict(os.environ)
            if lib:
                env["RC_HIP_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env,
                               stdout=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"the {name} build's child ended with {p.returncode}")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("AO_FILTER_AB ")][-1]
            runs[name].append(json.loads(line[len("AO_FILTER_AB "):]))

    lines = [f"{name}: {runs[name][0]['version']}" for name, _ in builds]
    for w, h in SIZES:
        key = f"{w}x{h}"
        lines.append(f"{key} depth {D}, {PASSES} passes of {REPS} rounds a build, medians "
                     f"(max-min) in ms over all of a build's rounds; per pass in brackets")
        ms = {}
        for name, _ in builds:
            for k in CASES:
                per = [r["sizes"][key]["ms"][k] for r in runs[name]]
                allv = [x for p in per for x in p]
                ms[name, k] = allv
                notes = [r["sizes"][key]["same_every_round"][k] for r in runs[name]]
                same = next((v for v in notes if v is not True), True)
                lines.append(f"  {name:<8}{k:<9}{med(allv):9.4f} ({spread(allv):.4f})  "
                             f"[{', '.join(f'{med(p):.4f}' for p in per)}]   "
                             f"same every round: {same}")
            lines.append(f"  {name:<8}states: {runs[name][0]['sizes'][key]['states_ok']}")
        a, b = (runs[n][0]["sizes"][key]["states_ok"] for n in ("lds", "direct"))
        lines.append("  the two builds' planes and images are the same: "
                     f"{all(a[k] == b[k] for k in a if k.startswith('crc'))}")

        def ratio(x, y, what):
            lines.append(f"  {what}: {x[0]} {x[1]} / {y[0]} {y[1]} = "
                         f"{med(ms[x]) / med(ms[y]):.4f}, difference "
                         f"{med(ms[x]) - med(ms[y]):+.4f} ms (spreads {spread(ms[x]):.4f} and "
                         f"{spread(ms[y]):.4f} ms)")

        ratio(("lds", "copy33"), ("direct", "copy33"),
              "what a ratio between two processes resolves (the same copy in both)")
        for r in (1, 3, 8):
            ratio(("lds", f"filt{r}"), ("direct", f"filt{r}"), f"1. radius {r}, LDS over direct")
        for r in (1, 3, 8):
            ratio(("lds", f"filt{r}"), ("lds", "copy33"), f"2. radius {r} over the copy of its bytes")
        ratio(("lds", "filt3"), ("lds", "ao16"), "3. radius 3 over the 16-direction pass it follows")
        ratio(("lds", "cgbuf"), ("lds", "ao1"), "4. k_camera_gbuffer over k_ao with one direction")
        ratio(("lds", "cgbuf0"), ("lds", "gbuf0"), "4. k_camera_gbuffer over k_gbuffer at eye +0")
        ratio(("lds", "compose"), ("lds", "copy11"), "5. the compose over the copy of its bytes")
    table = "\n".join(lines)
    print(table, flush=True)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as fh:
            fh.write(table + "\n")


if __name__ == "__main__":
    child() if sys.argv[1:] == ["--child"] else main()
