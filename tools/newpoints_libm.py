#!/usr/bin/env python3
"""The libm pins of CreateNewMapPoints measured (pins N4 and
N6): cos(2 * atan2(mb / 2, depth)) through glibc's atan2f / cosf against the
pinned double chain over a sweep of depths and every stereo keypoint of the
shared case list of tests/newpoints_cases.py, then the whole case list with
libm=True (atan2f, cosf, math.hypot) against the pinned mode.  Writes
profiles/newpoints_libm.json.  CPU only."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import newpoints_cases as C  # noqa: E402
import newpoints_ref as R  # noqa: E402


def cos_census():
    f32 = np.float32
    rng = np.random.default_rng(7)
    depths = [f32(d) for d in np.exp(rng.uniform(np.log(0.2), np.log(400.0), 20000))]
    for c in C.all_cases():
        for kf in (c.kf1, c.kf2):
            if kf["depth"] is not None:
                depths += [d for d in kf["depth"] if d > 0]
    out = {}
    for name, mb in (("kitti_mb", f32(C.CAM_N[5])), ("directed_mb", f32(C.CAM_D[5]))):
        differ, worst = 0, 0
        for d in depths:
            a, b = R.cos_stereo(mb, d, False), R.cos_stereo(mb, d, True)
            if a != b:
                differ += 1
                worst = max(worst, abs(R.f32_bits(a) - R.f32_bits(b)))
        out[name] = {"mb": float(mb), "depths": len(depths), "differing_cosines": differ,
                     "max_ulp_difference": worst}
    return out


def case_census():
    res = {"cases": 0, "matches": 0, "differing_status": 0, "differing_x3d": 0,
           "differing_point_records": 0, "max_abs_x3d_difference": 0.0}
    for c in C.all_cases():
        a, b = c.ref(), c.run(libm=True)
        n = len(c.match12)
        res["cases"] += 1
        res["matches"] += int((c.match12 >= 0).sum())
        res["differing_status"] += int((a["status"][:n] != b["status"][:n]).sum())
        dx = a["x3d"].view(np.uint32) != b["x3d"].view(np.uint32)
        res["differing_x3d"] += int(dx.any(axis=1).sum())
        with np.errstate(all="ignore"):
            diff = np.abs(a["x3d"].astype(np.float64) - b["x3d"].astype(np.float64))[dx]
        if diff.size and np.isfinite(diff).any():
            res["max_abs_x3d_difference"] = max(res["max_abs_x3d_difference"],
                                                float(diff[np.isfinite(diff)].max()))
        res["differing_point_records"] += int(sum(
            a["points"][i].tobytes() != b["points"][i].tobytes() for i in range(len(a["points"]))))
    return res


if __name__ == "__main__":
    res = {"cos_2atan2": cos_census(), "case_list_libm_vs_pinned": case_census()}
    out = ROOT / "profiles" / "newpoints_libm.json"
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
