"""Problems for Optimizer::OptimizeSim3 (test infrastructure): seeded natural
ones (two keyframes seeing 30-200 common points, a start from a perturbed true
Sim3, pixel noise, gross outliers) and directed ones of at most 130 pairs.

A case is a dict: keys1 / keys2 (xy float32 n x 2), octave1 / octave2,
point_index1, pose1 / pose2 ((rcw 9, tcw 3) float32), pos / bad (the shared map
points), match12, index2, start ((R 9, t 3, scale) float32), n1 / n2 (the
keyframes' counts; the arrays may be longer: junk past the counts), and `host`,
the name of its host values in HOSTS (levels, K1, K2, th2, fix_scale: one set
per device call, so a batch mixes cases of one host only)."""
from __future__ import annotations

import numpy as np

f32, f64 = np.float32, np.float64

_LEV8 = np.array([1.0 / (1.2 ** (2 * l)) for l in range(8)], f32)
_K = (f32(458.654), f32(457.296), f32(367.215), f32(248.375))
_FLAT = (f32(2.0 ** -70), f32(2.0 ** -70), f32(1.0), f32(0.5))
HOSTS = {
    "std": dict(levels=_LEV8, K1=_K, K2=_K, th2=f32(10.0), fix_scale=False),
    "fix": dict(levels=_LEV8, K1=_K, K2=_K, th2=f32(10.0), fix_scale=True),
    "lev16": dict(levels=np.array([1.0 / (1.1 ** (2 * l)) for l in range(16)], f32), K1=_K,
                  K2=(f32(520.9), f32(521.0), f32(325.1), f32(249.7)), th2=f32(10.0), fix_scale=False),
    # every projection is (1, 0.5) exactly: errors are obs - (1, 0.5), Jacobians 0
    "flat": dict(levels=np.array([1.0], f32), K1=_FLAT, K2=_FLAT, th2=f32(16.0), fix_scale=False),
    "neg": dict(levels=-_LEV8, K1=_K, K2=_K, th2=f32(10.0), fix_scale=False),
    "neg0": dict(levels=np.concatenate([[f32(-40.0)], _LEV8[1:]]).astype(f32), K1=_K, K2=_K,
                 th2=f32(10.0), fix_scale=False),
}


def _rot(axis, ang):
    a = np.asarray(axis, f64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def make(seed, n_pairs, n_out=0, noise=0.5, host="std", extra1=7, extra2=5, R12=None, t12=None,
         s12=1.15, pert=(0.03, 0.08, 1.04), out_px=60.0):
    """A natural problem.  X1c = s12 R12 X2c + t12; the first n_out pairs (in
    keypoint order of keyframe 1: scattered) are gross outliers."""
    rng = np.random.default_rng(seed)
    H = HOSTS[host]
    nl = len(H["levels"])
    R12 = _rot([0.2, 1.0, 0.1], 0.25) if R12 is None else np.asarray(R12, f64)
    t12 = np.array([0.4, -0.1, 0.3]) if t12 is None else np.asarray(t12, f64)
    # points in front of camera 2, kept where camera 1 sees them in front too
    X2 = np.empty((0, 3))
    while len(X2) < n_pairs:
        c = np.stack([rng.uniform(-2, 2, 4 * n_pairs + 8), rng.uniform(-1.5, 1.5, 4 * n_pairs + 8),
                      rng.uniform(3, 9, 4 * n_pairs + 8)], 1)
        X1 = s12 * (c @ R12.T) + t12
        X2 = np.concatenate([X2, c[X1[:, 2] > 1.0]])
    X2 = X2[:n_pairs]
    X1 = s12 * (X2 @ R12.T) + t12
    R1w, t1w = _rot([1, 0.3, -0.2], 0.4), np.array([0.3, 0.2, -0.5])
    R2w, t2w = _rot([-0.1, 1, 0.4], -0.7), np.array([-1.0, 0.1, 0.6])
    pose1 = (R1w.astype(f32).reshape(9), t1w.astype(f32))
    pose2 = (R2w.astype(f32).reshape(9), t2w.astype(f32))
    pos1 = (X1 - t1w) @ R1w
    pos2 = (X2 - t2w) @ R2w
    n1, n2 = n_pairs + extra1, n_pairs + extra2
    slot1 = np.sort(rng.permutation(n1)[:n_pairs])
    slot2 = rng.permutation(n2)[:n_pairs]
    K1, K2 = [float(v) for v in H["K1"]], [float(v) for v in H["K2"]]
    keys1 = rng.uniform(0, 700, (n1, 2))
    keys2 = rng.uniform(0, 700, (n2, 2))
    keys1[slot1] = np.stack([X1[:, 0] / X1[:, 2] * K1[0] + K1[2], X1[:, 1] / X1[:, 2] * K1[1] + K1[3]], 1) \
        + noise * rng.standard_normal((n_pairs, 2))
    keys2[slot2] = np.stack([X2[:, 0] / X2[:, 2] * K2[0] + K2[2], X2[:, 1] / X2[:, 2] * K2[1] + K2[3]], 1) \
        + noise * rng.standard_normal((n_pairs, 2))
    outl = rng.permutation(n_pairs)[:n_out]
    ang = rng.uniform(0, 2 * np.pi, n_out)
    keys1[slot1[outl]] += out_px * np.stack([np.cos(ang), np.sin(ang)], 1)
    # the map: points of keyframe 1, points of keyframe 2, a few others
    n_pts = 2 * n_pairs + 6
    pos = rng.uniform(-5, 5, (n_pts, 3))
    pos[:n_pairs], pos[n_pairs:2 * n_pairs] = pos1, pos2
    pidx1 = np.full(n1, -1, np.int32)
    pidx1[slot1] = np.arange(n_pairs)
    extra = np.setdiff1d(np.arange(n1), slot1)
    pidx1[extra[::2]] = 2 * n_pairs + (np.arange(len(extra[::2])) % 6)  # points without a match
    match12 = np.full(n1, -1, np.int32)
    match12[slot1] = n_pairs + np.arange(n_pairs)
    index2 = np.full(n1, -1, np.int32)
    index2[slot1] = slot2
    Rs = _rot(rng.standard_normal(3), pert[0]) @ R12
    ts = t12 + pert[1] * rng.standard_normal(3)
    return dict(keys1=keys1.astype(f32), keys2=keys2.astype(f32),
                octave1=rng.integers(0, nl, n1).astype(np.int32),
                octave2=rng.integers(0, nl, n2).astype(np.int32), point_index1=pidx1, pose1=pose1,
                pose2=pose2, pos=pos.astype(f32), bad=np.zeros(n_pts, np.uint8), match12=match12,
                index2=index2, start=(Rs.astype(f32).reshape(9), ts.astype(f32), f32(s12 * pert[2])),
                n1=n1, n2=n2, host=host, slot1=slot1, slot2=slot2)


def _flat(n_zero, specials):
    """Host "flat": every error is obs - (1, 0.5) at any estimate, so H = b = 0,
    the first trial has rho == 0 and the check sees exactly these errors."""
    n = n_zero + len(specials)
    rng = np.random.default_rng(5)
    pos = np.stack([rng.uniform(-1, 1, 2 * n), rng.uniform(-1, 1, 2 * n), rng.uniform(2, 6, 2 * n)], 1)
    eye = (np.eye(3, dtype=f32).reshape(9), np.zeros(3, f32))
    keys1 = np.tile(np.array([1.0, 0.5], f32), (n, 1))
    for k, (ex, ey) in enumerate(specials):
        keys1[n_zero // 2 + k] = (f32(1.0) + f32(ex), f32(0.5) + f32(ey))
    return dict(keys1=keys1, keys2=np.tile(np.array([1.0, 0.5], f32), (n, 1)),
                octave1=np.zeros(n, np.int32), octave2=np.zeros(n, np.int32),
                point_index1=np.arange(n, dtype=np.int32), pose1=eye, pose2=eye, pos=pos.astype(f32),
                bad=np.zeros(2 * n, np.uint8), match12=(n + np.arange(n)).astype(np.int32),
                index2=np.arange(n, dtype=np.int32)[::-1].copy(),
                start=(np.eye(3, dtype=f32).reshape(9), np.zeros(3, f32), f32(1.0)), n1=n, n2=n,
                host="flat")


def _with(case, **kw):
    c = dict(case)
    for k, v in kw.items():
        c[k] = v
    return c


def _edit(case, field, where, value):
    c = dict(case)
    a = np.array(case[field])
    a[where] = value
    c[field] = a
    return c


def natural():
    return {
        "nat30": make(101, 30, 4),
        "nat75": make(102, 75, 10, noise=0.8),
        "nat150": make(103, 150, 25),
        "nat200": make(104, 200, 30, noise=1.0),
        "nat120_fix": make(105, 120, 12, host="fix", s12=1.0, pert=(0.03, 0.08, 1.0)),
    }


def noise_free():
    return {"clean40": make(201, 40, 0, noise=0.0), "clean90": make(202, 90, 0, noise=0.0),
            "clean60_fix": make(203, 60, 0, noise=0.0, host="fix", s12=1.0, pert=(0.02, 0.05, 1.0))}


def directed():
    d = {}
    # ---- the < 10 gate after the first removal, nBad == 0 and nBad > 0
    for left in (0, 1, 9, 10, 11):
        d["gate%d_clean" % left] = make(300 + left, left, 0, noise=0.2, extra1=3, extra2=2)
    # (seeds chosen so that the first check removes exactly the gross outliers;
    # 0 left with nBad > 0 is "z0_point" / "start_half_turn" below)
    d["gate1_bad"] = make(411, 4, 3, noise=0.2, out_px=200.0)
    d["gate9_bad"] = make(400, 12, 3, noise=0.2)
    d["gate10_bad"] = make(322, 13, 3, noise=0.2)
    d["gate11_bad"] = make(323, 14, 3, noise=0.2)
    # ---- tile and wave edges
    for n in (32, 33, 64, 65, 129):
        d["pairs%d" % n] = make(330 + n, n, n // 8, extra1=1 if n != 129 else 0, extra2=1 if n != 129 else 0)
    # ---- every skip rule
    c = make(340, 40, 5)
    s1 = c["slot1"]
    c = _edit(c, "match12", s1[3], -1)                       # NULL match
    c = _edit(c, "point_index1", s1[7], -1)                  # NULL pMP1
    c = _edit(c, "bad", c["point_index1"][s1[11]], 1)        # pMP1 bad
    c = _edit(c, "bad", c["match12"][s1[13]], 1)             # pMP2 bad
    c = _edit(c, "index2", s1[17], -1)                       # i2 < 0
    c = _edit(c, "index2", s1[19], -2147483648)
    d["skips"] = c
    # ---- malformed problems
    c = make(341, 30, 3)
    d["bad_i2"] = _edit(c, "index2", c["slot1"][12], c["n2"])
    d["bad_i2_big"] = _edit(c, "index2", c["slot1"][29], 2147483647)
    d["bad_oct1"] = _edit(c, "octave1", c["slot1"][5], 8)
    d["bad_oct1_neg"] = _edit(c, "octave1", c["slot1"][0], -1)
    d["bad_oct2"] = _edit(c, "octave2", c["slot2"][20], 8)
    d["bad_oct2_neg"] = _edit(c, "octave2", c["slot2"][9], -3)
    # a bad octave on a skipped pair, or on a keypoint no pair names, is not malformed
    c2 = _edit(c, "octave1", c["slot1"][5], 99)
    d["bad_oct_skipped"] = _edit(c2, "match12", c["slot1"][5], -1)
    # ---- fix_scale
    d["fix50"] = make(350, 50, 6, host="fix", s12=1.0, pert=(0.03, 0.08, 1.0))
    d["fix_scale_off_start"] = make(351, 50, 6, host="fix", s12=1.0, pert=(0.03, 0.08, 1.1))
    # ---- exp branches of the steps: a start at the optimum (small, small),
    # the usual start (large, large), fix_scale (sigma == 0, theta large), a
    # start whose scale alone is off
    d["start_exact"] = make(360, 45, 0, noise=0.0, pert=(0.0, 0.0, 1.0))
    d["start_scale_only"] = make(361, 45, 0, noise=0.0, pert=(0.0, 0.0, 1.002))
    d["start_far"] = make(362, 60, 5, pert=(0.5, 0.6, 1.5))
    # ---- Quaterniond(Matrix3d) branches from the start value: half turns
    # about x, y and z (trace <= 0, the largest diagonal entry first / second /
    # third); the cameras face each other for x and y
    d["quat_x"] = make(370, 40, 4, R12=_rot([1, 0.02, 0.01], np.pi - 0.01), t12=[0.2, 0.1, 12.0],
                       s12=1.0)
    d["quat_y"] = make(371, 40, 4, R12=_rot([0.01, 1, 0.02], np.pi - 0.01), t12=[0.2, 0.1, 12.0],
                       s12=1.0)
    d["quat_z"] = make(372, 40, 4, R12=_rot([0.01, 0.02, 1], np.pi - 0.01), t12=[0.2, 0.1, 0.3])
    # a start half a turn away from the truth: large steps
    c = make(373, 40, 0, noise=0.1)
    Rs = (_rot([0.1, 1, 0], 3.0) @ np.asarray(c["start"][0], f64).reshape(3, 3)).astype(f32).reshape(9)
    d["start_half_turn"] = _with(c, start=(Rs, c["start"][1], c["start"][2]))
    # ---- Quaterniond(Matrix3d) inside Sim3(Vector7d): one-pair problems from a
    # far start whose LM steps turn by about half a turn, so that the trace of
    # the step's R is not positive and the second (quat_exp_y) or third
    # (quat_exp_z) diagonal entry is the largest (seeds found by search; the
    # first is what the NaN steps take)
    far = (1.5, 1.0, 2.0)
    d["quat_exp_y"] = make(9848, 1, 0, noise=0.2, pert=far)
    d["quat_exp_z"] = make(9023, 1, 0, noise=0.2, pert=far)
    # ---- LDLT pivot pairs (k, idx) the other cases leave out: (1, 4), (0, 3),
    # (0, 4), (0, 2) (quat_exp_z adds (1, 2)); degenerate few-pair systems
    d["pivot_14"] = make(9208, 1, 0, noise=0.2, pert=far)
    d["pivot_03"] = make(9340, 1, 0, noise=0.2, pert=far)
    d["pivot_04"] = make(9269, 2, 0, noise=0.2, pert=far)
    d["pivot_02"] = make(9483, 2, 0, noise=0.2, host="neg0", pert=far)
    # ---- exact thresholds (host "flat", th2 = 16 = delta^2): chi2 == th2 stays,
    # the double above it goes; Huber's argument is delta^2 on the first
    d["threshold"] = _flat(10, [(4.0, 0.0), (4.0, 2.0 ** -24)])
    d["threshold_gate"] = _flat(9, [(4.0, 2.0 ** -24), (4.0, 0.0)])
    # ---- level tables of 1 (above) and 16 entries
    d["lev16"] = make(380, 70, 8, host="lev16")
    # ---- NaN, infinite and z == 0 inputs
    c = make(390, 40, 4)
    d["nan_point"] = _edit(c, "pos", (c["match12"][c["slot1"][6]], 1), np.nan)
    d["inf_point"] = _edit(c, "pos", (c["point_index1"][c["slot1"][8]], 0), np.inf)
    d["nan_key"] = _edit(c, "keys1", (c["slot1"][2], 0), np.nan)
    d["nan_start"] = _with(c, start=(c["start"][0], np.array([np.nan, 0, 0], f32), c["start"][2]))
    d["inf_scale"] = _with(c, start=(c["start"][0], c["start"][1], f32(np.inf)))
    d["zero_scale"] = _with(c, start=(c["start"][0], c["start"][1], f32(0.0)))
    eye = (np.eye(3, dtype=f32).reshape(9), np.zeros(3, f32))
    c0 = _with(c, pose2=eye)
    d["z0_point"] = _edit(c0, "pos", (c["match12"][c["slot1"][4]], 2), 0.0)
    # ---- negative level weights: isPositive() == false
    d["neg_all"] = make(395, 40, 4, host="neg")
    d["neg_level0"] = make(396, 60, 6, host="neg0")
    # ---- junk past every count: the keyframes' counts are below the arrays
    c = make(397, 50, 6)
    cut = int(c["slot1"][40])  # keyframe 1 ends inside its pairs
    rng = np.random.default_rng(9)
    j = dict(c)
    for f, lo, hi in (("match12", -5, 2 ** 31 - 1), ("index2", -5, 2 ** 31 - 1),
                      ("point_index1", -5, 2 ** 31 - 1), ("octave1", -100, 100)):
        a = np.array(c[f])
        a[cut:] = rng.integers(lo, hi, len(a) - cut)
        j[f] = a
    j["n1"] = cut
    d["junk"] = j
    for c in d.values():
        assert int((np.asarray(c["match12"])[:c["n1"]] >= 0).sum()) <= 130
    return d


def all_cases():
    c = {}
    c.update(natural())
    c.update(noise_free())
    c.update(directed())
    return c


def run_ref(case, libm=False, variants=()):
    """tests/sim3opt_ref.optimize_sim3 on a case."""
    import sim3opt_ref as ref

    H = HOSTS[case["host"]]
    return ref.optimize_sim3(case["keys1"], case["octave1"], case["point_index1"], case["pose1"],
                             case["keys2"], case["octave2"], case["pose2"], case["pos"], case["bad"],
                             case["match12"], case["index2"], case["start"], H["levels"], H["K1"],
                             H["K2"], H["th2"], H["fix_scale"], n1=case["n1"], n2=case["n2"],
                             libm=libm, variants=variants)
