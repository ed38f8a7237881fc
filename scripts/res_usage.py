"""Per-kernel register / scratch / occupancy table of HIP sources (hipcc
-Rpass-analysis=kernel-resource-usage), for before/after comparisons of a kernel change.
   python3 scripts/res_usage.py [SRC.hip ...] [extra hipcc flags...]
Without a source: the two kernel files, rc_kernels.hip and rc_sample_kernels.hip."""
import re, subprocess, sys
srcs = [a for a in sys.argv[1:] if a.endswith(".hip")] or [
    "raytracing-programs_amd/csrc/rc_kernels.hip",
    "raytracing-programs_amd/csrc/rc_sample_kernels.hip"]
flags = ("--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off "
         "-fno-gpu-flush-denormals-to-zero -fhip-fp32-correctly-rounded-divide-sqrt "
         "-Iinclude -Iraytracing-programs_amd/csrc -w --cuda-device-only").split() + [
             a for a in sys.argv[1:] if not a.endswith(".hip")]
procs = [subprocess.Popen(["/opt/rocm/bin/hipcc", *flags, "-Rpass-analysis=kernel-resource-usage",
                           "-c", src, "-o", "/dev/null"], stderr=subprocess.PIPE, text=True)
         for src in srcs]
cur, rows = None, {}
for p in procs:
    for line in p.communicate()[1].splitlines():
        m = re.search(r"remark: (.*?) \[-Rpass", line)
        if not m:
            continue
        k, _, v = m.group(1).strip().partition(": ")
        if k == "Function Name":
            cur = v
            rows[cur] = {}
        elif cur:
            rows[cur][k] = v
for name, d in rows.items():
    short = re.sub(r"^_ZN2rc\d+", "", name)[:40]
    print(f"{short:40s} vgpr {d.get('VGPRs','?'):>4} agpr {d.get('AGPRs','?'):>3} "
          f"scratch {d.get('ScratchSize [bytes/lane]','?'):>4} occ {d.get('Occupancy [waves/SIMD]','?'):>2} "
          f"vspill {d.get('VGPRs Spill','?'):>3} lds {d.get('LDS Size [bytes/block]','?')}")
