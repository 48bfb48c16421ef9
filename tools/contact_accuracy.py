#!/usr/bin/env python3
"""The accuracy of statements C1 to C6 (include/raylib_amd.h, contact segments) as arithmetic: the float32 NumPy restatement of tests/contact_cases.py against the
float64 edge-piercing reference, on the inputs of tests/test_contact_host.py's accuracy test.  No library, no device.

usage: tools/contact_accuracy.py [OUT.json]        (default profiles/contact_accuracy.json)

Per spacing and seed: the meeting pairs, the largest endpoint error in ulps of the largest coordinate magnitude among the pair's six vertices, the 99.9th
percentile; per spacing the test's bound, 8 times the largest error rounded up to a power of two (tests/contact_cases.py ACCURACY_BOUND_ULPS must say the same)."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contact_cases as cc  # noqa: E402
import overlap_cases as oc  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "contact_accuracy.json")
    result = {"pairs": cc.ACCURACY_PAIRS, "unit": "float32 ulps of the largest coordinate magnitude among the pair's six vertices", "spacings": {}}
    for spacing in (8.0, 0.0):
        rows = []
        for seed in cc.ACCURACY_SEEDS:
            Q, T = oc.generic_pairs(np.random.RandomState(seed), cc.ACCURACY_PAIRS, spacing)
            meets = oc.pierce64(Q, T)
            count, pts = cc.pierce_points64(Q, T)
            recs = cc.contact_of_pairs(Q[meets], T[meets])
            err = cc.segment_error_ulps(recs, Q[meets], T[meets], pts[meets])
            rows.append({"seed": seed, "meeting": int(meets.sum()), "two_points": bool((count[meets] == 2).all()), "segment": int((recs["kind"] == cc.SEGMENT).sum()),
                         "max_ulp": float(err.max()), "p999_ulp": float(np.percentile(err, 99.9)), "median_ulp": float(np.median(err))})
        worst = max(r["max_ulp"] for r in rows)
        bound = float(2 ** math.ceil(math.log2(8 * worst)))
        assert bound == cc.ACCURACY_BOUND_ULPS[spacing], (spacing, bound, cc.ACCURACY_BOUND_ULPS[spacing])
        result["spacings"]["%g" % spacing] = {"seeds": rows, "max_ulp": worst, "bound_ulp": bound}
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
