#!/usr/bin/env python3
"""Golden messages of the sampling family's refusals and environment warnings (no GPU).

Runs every call of tests/test_refusals.py's table (REFUSALS, ENV) and writes
tests/golden/refusals.json: per case the return code and the bytes on stderr, or the decision
and the warning.  The committed file was recorded from the library as it stood before the
entry points were gathered in csrc/rc_sampling.hip; a re-run must reproduce it byte for byte.
Usage: python tests/golden/make_refusals_golden.py [--package DIR] [--out FILE]
  --package DIR   record from the built package in DIR (another checkout's
                  raytracing-programs_amd) instead of this tree's
"""
import argparse
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package")
    ap.add_argument("--out", default=os.path.join(HERE, "refusals.json"))
    a = ap.parse_args()
    if a.package:   # tests/helpers.py takes the package already in sys.modules
        name = "raytracing_programs_amd"
        spec = importlib.util.spec_from_file_location(name, os.path.join(a.package, "__init__.py"))
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_refusals as t

    table = {"refusals": {cid: t.run_refusal(export, args) for cid, export, args in t.REFUSALS},
             "env": {cid: t.run_env(env, fn, kw, os.environ.__setitem__,
                                    lambda name: os.environ.pop(name, None))
                     for cid, env, fn, kw in t.ENV}}
    with open(a.out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(table["refusals"]), "refusals,", len(table["env"]), "environment cases")


if __name__ == "__main__":
    main()
