#!/usr/bin/env python3
"""RaylibAMD_MotionHost (float32, include/raylib_amd.h statements T2 to T4) against a float64 restatement, on the CPU: the largest |prevX|, |prevY| and
relative prevT differences over the scenes and cases of tests/temporal_cases.py, into profiles/temporal_accuracy.json.  tests/test_temporal_host.py and the GPU
tests assert tests/temporal_cases.MARGIN times these figures.  No device needed.

usage: tools/temporal_accuracy.py [--out profiles/temporal_accuracy.json]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import temporal_cases as tc                     # noqa: E402  (tests/helpers.py puts the package on sys.path)
from raylib_amd import binding                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=tc.ACCURACY_JSON)
    args = ap.parse_args()
    os.environ.setdefault("RAYLIB_QUIET", "1")
    rec = tc.measure_accuracy(binding.load(), tempfile.mkdtemp())
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec["worst"]))


if __name__ == "__main__":
    main()
