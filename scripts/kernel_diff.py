"""Compare two device assembly files (hipcc --cuda-device-only -S) kernel by kernel: comments,
directives and local label names stripped, the instruction streams compared as text.
   python3 scripts/kernel_diff.py PARENT.s NEW.s
Prints the counts (identical, different, missing) and one line per kernel only one side has:
its instruction count and symbol.  Exit status 1 when a kernel of PARENT.s differs or is missing."""
import re
import sys


def kernels(path):
    out, cur = {}, None
    labels = {}
    for line in open(path):
        line = line.split(";")[0].rstrip()
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, labels = m.group(1), {}
            out[cur] = []
            continue
        if cur is None or not line.strip():
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if s.startswith("."):
            if re.match(r"^\.LBB\w+:", s):      # a local label: numbered in order of appearance
                out[cur].append(f"L{labels.setdefault(s[:-1], len(labels))}:")
            continue
        s = re.sub(r"\.LBB\w+", lambda m: f"L{labels.setdefault(m.group(0), len(labels))}", s)
        out[cur].append(s)
    return {k: v for k, v in out.items() if any(not x.endswith(":") for x in v)}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    same = [k for k in old if new.get(k) == old[k]]
    diff = [k for k in old if k in new and new[k] != old[k]]
    gone = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    print(f"parent kernels {len(old)}: identical {len(same)}, different {len(diff)}, missing "
          f"{len(gone)}; new {len(added)}")
    for k in diff:
        print(f"different {k}")
    for k in gone:
        print(f"missing   {k}")
    for k in added:
        print(f"new {sum(not x.endswith(':') for x in new[k]):5d} {k}")
    return 1 if diff or gone else 0


if __name__ == "__main__":
    sys.exit(main())
