#!/usr/bin/env python3
"""The libm pins of OptimizeSim3 measured: runs the case list of
tests/sim3opt_cases.py with math.exp / sin / cos / pow against the pinned forms
and writes profiles/sim3opt_libm.json.  CPU only."""
import json
import math
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import sim3opt_cases as C  # noqa: E402
import sim3opt_ref as R  # noqa: E402


def key(r):
    return (r["status"], r["n_corr"], r["n_bad"], r["n_inliers"], r["q"].tobytes(), r["t"].tobytes(),
            np.float64(r["s"]).tobytes(), r["R"].tobytes(), r["t_f"].tobytes(), r["match12"].tobytes())


def study():
    cases = C.all_cases()
    changed, counts_changed, args = [], [], set()
    for name, c in cases.items():
        a, b = C.run_ref(c), C.run_ref(c, libm=True)
        args |= a["trace"]["exp_args"]
        if key(a) != key(b):
            changed.append(name)
        if (a["n_corr"], a["n_bad"], a["n_inliers"]) != (b["n_corr"], b["n_bad"], b["n_inliers"]) or \
                not np.array_equal(a["match12"], b["match12"]):
            counts_changed.append(name)
    fin = [R._from_bits(v) for v in args if math.isfinite(R._from_bits(v))]
    differ = sum(R._bits(R.pinned_exp(x)) != R._bits(math.exp(x)) for x in fin)
    return {"cases": len(cases), "outputs_changed_by_libm": len(changed), "changed": changed,
            "counts_or_matches_changed": counts_changed, "exp_arguments_reached": len(fin),
            "exp_arguments_where_libm_differs": differ,
            "note": "math.exp / sin / cos / pow of this machine's libm in place of pinned_exp, "
                    "pinned_sincos_d and (x * x) * x"}


if __name__ == "__main__":
    res = study()
    out = ROOT / "profiles" / "sim3opt_libm.json"
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
