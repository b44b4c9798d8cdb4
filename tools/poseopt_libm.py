#!/usr/bin/env python3
"""The libm pins of PoseOptimization measured: runs the shared
case list of tests/poseopt_cases.py with math.sin / cos / pow against the pinned
forms and writes profiles/poseopt_libm.json.  CPU only."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import poseopt_cases  # noqa: E402

if __name__ == "__main__":
    res = poseopt_cases.libm_study()
    out = ROOT / "profiles" / "poseopt_libm.json"
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
