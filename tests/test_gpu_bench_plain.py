"""A plain `bench.py` run: the headline line only, `--steps` timed steps, and
`--dump-outputs` files of the last step; `--full` keys stay out of it."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_plain_run_headline_and_dump(gpu, tmp_path):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--frames", "192", "--batch", "64", "--threads", "4", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["unit"] == "frames/s"
    assert res["higher_is_better"] is True and res["dtype"] == "u8"
    assert res["ms_per_step"] > 0
    assert abs(res["value"] - 192 / (res["ms_per_step"] * 1e-3)) < 1e-6 * res["value"]
    assert abs(res["config"]["timed_region_s"] - 3 * res["ms_per_step"] * 1e-3) < 1e-9
    for key in ("roofline", "kernels", "host_input", "parity_sample", "cpu_baseline", "dropin",
                "C3_stereo_pairs_per_s", "C5_problems_per_s", "C4_latency"):
        assert key not in res
    out = {p.stem: np.load(p) for p in (tmp_path / "out").glob("*.npy")}
    assert set(out) == {"keypoint_counts", "sample_frames", "keypoints", "descriptors", "kp_match",
                        "nmatches"}
    assert all(a.dtype == np.float32 for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    cnt = out["keypoint_counts"]
    assert cnt.shape == (192,) and cnt.min() > 0
    assert abs(cnt.mean() - res["config"]["mean_keypoints_per_frame"]) < 1e-3
    f = out["sample_frames"].astype(int)  # 3 launches per step, all resident in the 4 buffer sets
    assert len(f) == 192 and sorted(f) == list(range(192))
    live = np.arange(out["keypoints"].shape[1])[None, :] < cnt[f][:, None]
    assert (out["keypoints"][..., 2][live] > 0).all()  # size of every live keypoint
    assert not out["keypoints"][~live].any() and not out["descriptors"][~live].any()
    assert (out["nmatches"] == (out["kp_match"] >= 0).sum(1)).all()
