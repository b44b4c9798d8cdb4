#!/usr/bin/env python3
"""Isolated device time of orb_update_local_map_batch at the headline's map
size: P problems, each about 80 local keyframes of 1,000 map-point slots whose
union is about 5,000 local points, 1,000 keypoints per frame.

The map is a chain of keyframes; keyframe k lists the 1,000 points from 50 k
on, so 80 neighbouring keyframes name 4,950 distinct points.  A frame at
keyframe c holds about 800 matches spread over the points of c - 40 .. c + 40.
Device events around `reps` back-to-back calls after a warm-up; two problems are
compared with the Python restatement first.  One JSON line, also written to
--out.

    python tools/local_map_time.py --problems 256 --reps 50 --out profiles/localmap_L1.json
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def build_map(n_kf, step, slots, rng):
    n_mp = (n_kf - 1) * step + slots
    kf_mp = [list(range(k * step, k * step + slots)) for k in range(n_kf)]
    obs = [[] for _ in range(n_mp)]
    for k, lst in enumerate(kf_mp):
        for pi in lst:
            obs[pi].append(k)
    for k in range(n_kf):                      # keypoint order is not point order
        rng.shuffle(kf_mp[k])
        for j in rng.integers(0, slots, slots // 20):
            kf_mp[k][j] = -1                   # keypoints without a map point
    near = lambda k: [q for d in range(1, 8) for q in (k - d, k + d) if 0 <= q < n_kf][:12]
    import local_map_ref as R
    pts = np.zeros(n_mp, R.MAP_POINT_DTYPE)
    pts["pos"] = rng.standard_normal((n_mp, 3)).astype(np.float32)
    pts["has_obs"] = 1
    pts["bad"] = rng.random(n_mp) < 0.02
    return dict(rank=rng.permutation(n_kf).astype(np.int32), bad=np.zeros(n_kf, np.uint8),
                parent=np.arange(-1, n_kf - 1, dtype=np.int32), cov=[near(k) for k in range(n_kf)],
                child=[[k + 1] if k + 1 < n_kf else [] for k in range(n_kf)], kf_mp=kf_mp, obs=obs,
                points=pts, desc=rng.integers(0, 256, (n_mp, 32), dtype=np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--keyframes", type=int, default=400)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as g
    import local_map_cases as C
    import local_map_ref as R
    orb = g.load_package()
    rng = np.random.default_rng(1)
    step, slots, nkp = 50, 1000, 1000
    m = build_map(a.keyframes, step, slots, rng)
    n_kf, n_mp = a.keyframes, len(m["points"])
    P, S, MS = a.problems, nkp, 8192
    km = np.full((P, S), -1, np.int32)
    for p in range(P):
        c = int(rng.integers(45, n_kf - 45))
        lo = (c - 10) * step                   # points first listed by keyframes c - 10 .. c + 50
        ids = rng.integers(lo, lo + 61 * step, 800)
        km[p, rng.permutation(S)[:800]] = ids
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).cuda()
    view = orb.MapView(**C.view_arrays(m))
    d = dict(nk=dev(np.full(P, nkp, np.int32)), km=dev(km),
             lkf=torch.zeros(P * n_kf, dtype=torch.int32, device="cuda"),
             nlkf=torch.zeros(P, dtype=torch.int32, device="cuda"),
             li=torch.zeros(P * MS, dtype=torch.int32, device="cuda"),
             mps=torch.zeros(P * MS * 36, dtype=torch.uint8, device="cuda"),
             desc=torch.zeros(P * MS * 32, dtype=torch.uint8, device="cuda"),
             nmps=torch.zeros(P, dtype=torch.int32, device="cuda"),
             locked=torch.zeros(P * S, dtype=torch.uint8, device="cuda"),
             info=torch.zeros(P * 8, dtype=torch.int32, device="cuda"))
    mt = orb.ORBmatcher(0.8, True)
    st = torch.cuda.Stream()

    def call(n):
        mt.update_local_map_batch(n, view, d["nk"].data_ptr(), d["km"].data_ptr(), S,
                                  d["lkf"].data_ptr(), d["nlkf"].data_ptr(), n_kf,
                                  d["li"].data_ptr(), d["mps"].data_ptr(), d["desc"].data_ptr(),
                                  d["nmps"].data_ptr(), MS, d["locked"].data_ptr(),
                                  d["info"].data_ptr(), stream=st.cuda_stream)

    def timed(n):
        for _ in range(a.warmup):
            call(n)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            e0.record(st)
            for _ in range(a.reps):
                call(n)
            e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / a.reps      # us per call

    call(P)                                    # the first call on fresh matches is checked
    torch.cuda.synchronize()
    info = d["info"].cpu().numpy().view(R.INFO_DTYPE).copy()
    li = d["li"].cpu().numpy().view(np.int32).reshape(P, MS)
    km_out = d["km"].cpu().numpy().view(np.int32).reshape(P, S)
    for p in (0, P - 1):                       # the timed work is the reference's answer
        e = R.update_local_map(m, km[p], [], MS)
        assert info[p].tolist() == e["info"].tolist(), (info[p], e["info"])
        assert np.array_equal(li[p, :len(e["local_index"])], e["local_index"])
        assert np.array_equal(km_out[p], e["kp_match"])
    us_batch = [timed(P) for _ in range(3)]
    us_one = [timed(1) for _ in range(3)]
    res = dict(kernel="k_local_map", problems=P, reps=a.reps, keypoints=nkp, n_kf=n_kf, n_mp=n_mp,
               slots_per_keyframe=slots,
               local_keyframes_mean=float(info["n_local_kf"].mean()),
               local_points_mean=float(info["n_local_points"].mean()),
               local_points_max=int(info["n_local_points"].max()),
               us_per_call_batch=[round(x, 2) for x in us_batch],
               us_per_problem_batch=round(min(us_batch) / P, 3),
               us_per_call_one_problem=[round(x, 2) for x in us_one],
               timing="device events around reps back-to-back calls on one stream, warm")
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
