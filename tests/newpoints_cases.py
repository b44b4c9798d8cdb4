"""Inputs of the CreateNewMapPoints device batch (test infrastructure): cases as
tests/newpoints_ref.py reads them, and their packing into the slot arrays of
orb_create_new_map_points_batch / orb_scene_median_depth_batch.

A Case is two keyframes (dict: keys, u_right, depth, point_index, pose), the
match12 row, the neighbour's median depth, the cameras, a cursor and a point
capacity.  `tags` names the conditions a case was built for; the census of
tests/test_newpoints_ref.py checks what they claim against the restatement's
traces.  Natural cases come from tests/scenarios.py poses and its camera:
ground-truth points projected into both keyframes with sub-pixel noise.
Directed cases sit on a threshold: the deciding input is written as two
adjacent floats by bit pattern (found by bisection over the bits, or stated).
"""
from __future__ import annotations

import numpy as np

import scenarios
from newpoints_ref import (ACCEPTED, KEYPOINT_DTYPE, LOW_PARALLAX, MAP_POINT_DTYPE,
                           NEW_POINT_INFO_DTYPE, POSE_DTYPE, REPROJ1, REPROJ2, cos_stereo,
                           create_new_map_points, f32_bits, f32_from_bits, f32_next,
                           scene_median_depth, triangulate_match)

f32 = np.float32
N_LEVELS = 8
_sf = [f32(1)]
for _ in range(N_LEVELS - 1):
    _sf.append(_sf[-1] * f32(1.2))
SCALE_FACTORS = np.array(_sf, f32)                       # mvScaleFactors
LEVEL_SIGMA2 = np.array([s * s for s in _sf], f32)       # mvLevelSigma2
CAM_D = (512.0, 512.0, 320.0, 240.0, 64.0, 0.125)        # directed: invfx is a power of two
CAM_N = tuple(float(f32(v)) for v in scenarios.camera())  # natural: the KITTI-like camera
WG = 256  # NP_T of the product build ("one more than the workgroup size" refers to it)
I3 = np.eye(3, dtype=np.float32)


def pose_rec(R, t, ow=None):
    rec = np.zeros(1, POSE_DTYPE)[0]
    R, t = np.asarray(R, f32), np.asarray(t, f32)
    rec["rcw"], rec["tcw"] = R.reshape(9), t
    rec["ow"] = scenarios._camera_center(R, t) if ow is None else np.asarray(ow, f32)
    return rec


def make_kf(kps, pose, stereo=True, point_index=None):
    """kps: rows (u, v, octave[, u_right, depth])."""
    n = len(kps)
    keys = np.zeros(n, KEYPOINT_DTYPE)
    ur, dp = np.full(n, -1, f32), np.full(n, -1, f32)
    for i, k in enumerate(kps):
        keys[i]["x"], keys[i]["y"], keys[i]["octave"] = f32(k[0]), f32(k[1]), int(k[2])
        keys[i]["size"], keys[i]["class_id"] = 31, -1
        if len(k) > 3:
            ur[i], dp[i] = f32(k[3]), f32(k[4])
    pidx = np.full(n, -1, np.int32) if point_index is None else np.asarray(point_index, np.int32)
    return dict(keys=keys, u_right=ur if stereo else None, depth=dp if stereo else None,
                point_index=pidx.copy(), pose=pose)


class Case:
    def __init__(self, name, kf1, kf2, match12, monocular=False, median=np.nan, cam1=CAM_D,
                 cam2=CAM_D, cursor=0, capacity=None, tags=(), points=None):
        self.name, self.kf1, self.kf2 = name, kf1, kf2
        self.match12 = np.asarray(match12, np.int32)
        assert len(self.match12) == len(kf1["keys"])
        self.monocular, self.median = bool(monocular), f32(median)
        self.cam1, self.cam2 = cam1, cam2
        self.cursor = int(cursor)
        self.capacity = int(capacity if capacity is not None else cursor + len(match12) + 3)
        self.tags = set(tags)
        # the map before the call (records below the cursor; junk above it)
        self.points = points
        self._ref = {}

    def run(self, libm=False, sw=frozenset(), traces=None, prefill=None):
        """The restatement on copies: dict(info, cursor, status, x3d, pairs,
        points, pidx1, pidx2).  prefill: (status, x3d, pairs, points) junk."""
        n1 = len(self.kf1["keys"])
        kf1 = dict(self.kf1, point_index=self.kf1["point_index"].copy())
        kf2 = dict(self.kf2, point_index=self.kf2["point_index"].copy())
        if prefill is None:
            status = np.full(n1, 0xEE, np.uint8)
            x3d = np.full((n1, 3), -7.25, f32)
            pairs = np.full((n1, 2), -77, np.int32)
            points = junk_points(self.capacity)
        else:
            status, x3d, pairs, points = (a.copy() for a in prefill)
        if self.points is not None:
            points[:len(self.points)] = self.points
        info, cur = create_new_map_points(kf1, kf2, self.match12, self.median, self.cam1,
                                          self.cam2, SCALE_FACTORS, LEVEL_SIGMA2, self.monocular,
                                          points, self.cursor, status, x3d, pairs, libm, sw, traces)
        return dict(info=info, cursor=cur, status=status, x3d=x3d, pairs=pairs, points=points,
                    pidx1=kf1["point_index"], pidx2=kf2["point_index"])

    def ref(self):
        """The restatement's answer, computed once and left unchanged."""
        if "r" not in self._ref:
            tr = []
            self._ref["r"] = self.run(traces=tr)
            self._ref["t"] = tr
        return self._ref["r"]

    def traces(self):
        self.ref()
        return self._ref["t"]


def junk_points(n):
    pts = np.zeros(n, MAP_POINT_DTYPE)
    pts.view(np.uint8)[:] = 0xA5
    return pts


# ------------------------------------------------------------ natural cases
def natural_case(name, seed, n_match, monocular, stereo_frac=0.6, n_extra=20, noise=0.3,
                 outlier_frac=0.12, baseline=(0.9, 0.05, 0.1), n_exist=30, z_range=(4.0, 30.0),
                 cam2=None, accept=None, tags=()):
    """n_match matches of ground-truth points seen from a scenarios.pose() keyframe
    and from a neighbour rotated about y and moved by `baseline`; sub-pixel
    noise on every coordinate; a fraction of gross outliers.  accept (a bool
    per match, in i1 order) replaces the random outliers: True rows get the
    noise alone, False rows a 60-pixel error."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf, mb = CAM_N
    R1, t1, _ = scenarios.pose(rng)
    Ry = scenarios._ry(rng.uniform(-0.03, 0.03))
    R2 = (Ry @ R1.astype(np.float64)).astype(f32)
    t2 = (Ry @ t1.astype(np.float64) - R2.astype(np.float64) @ np.asarray(baseline)).astype(f32)
    p1, p2 = pose_rec(R1, t1), pose_rec(R2, t2)
    n = n_match + n_exist
    z = rng.uniform(*z_range, n)
    u = rng.uniform(80, 1160, n)
    v = rng.uniform(40, 330, n)
    Xc1 = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    Xw = (Xc1 - t1.astype(np.float64)) @ R1.astype(np.float64)
    Xc2 = Xw @ R2.astype(np.float64).T + t2.astype(np.float64)
    u2 = fx * Xc2[:, 0] / Xc2[:, 2] + cx
    v2 = fy * Xc2[:, 1] / Xc2[:, 2] + cy
    octave = rng.integers(0, 4, n)
    octave2 = np.clip(octave + rng.integers(-1, 2, n), 0, N_LEVELS - 1)
    nz = lambda: rng.normal(0, noise, n)
    k1 = np.stack([u + nz(), v + nz(), octave, u - bf / z + nz(), z * (1 + rng.normal(0, 0.01, n))], 1)
    k2 = np.stack([u2 + nz(), v2 + nz(), octave2, u2 - bf / Xc2[:, 2] + nz(),
                   Xc2[:, 2] * (1 + rng.normal(0, 0.01, n))], 1)
    if accept is None:
        bad = rng.random(n) < outlier_frac
        bad[n_match:] = False
    else:
        bad = np.zeros(n, bool)
        bad[:n_match] = ~np.asarray(accept, bool)
        k2[:, 2] = k1[:, 2]
    k2[bad, 1] += 60.0
    if monocular:
        s1 = s2 = np.zeros(n, bool)
    else:
        s1, s2 = rng.random(n) < stereo_frac, rng.random(n) < stereo_frac
    k1[~s1, 3:] = -1
    k2[~s2, 3:] = -1
    # KF1: the matched keypoints in i1 order with n_extra unmatched ones interleaved
    # at random (accept patterns keep the matched ones first, in order); KF2: shuffled
    n1 = n_match + n_exist + n_extra
    if accept is None:
        slots1 = rng.permutation(n1)[:n]
        slots1[:n_match] = np.sort(slots1[:n_match])
    else:
        slots1 = np.arange(n)
    n2 = n + n_extra // 2
    slots2 = rng.permutation(n2)[:n]
    rows1 = np.tile(np.array([100.0, 100.0, 0, -1, -1]), (n1, 1))
    rows2 = np.tile(np.array([100.0, 100.0, 0, -1, -1]), (n2, 1))
    rows1[slots1], rows2[slots2] = k1, k2
    # the keypoints past n_match already have a map point (the matcher skips them)
    pidx1, pidx2 = np.full(n1, -1, np.int32), np.full(n2, -1, np.int32)
    pidx1[slots1[n_match:]] = np.arange(n_exist)
    pidx2[slots2[n_match:]] = np.arange(n_exist)
    points = np.zeros(n_exist, MAP_POINT_DTYPE)
    points["pos"] = Xw[n_match:].astype(f32)
    points["has_obs"] = 1
    match12 = np.full(n1, -1, np.int32)
    match12[slots1[:n_match]] = slots2[:n_match]
    kf1 = make_kf(rows1, p1, stereo=not monocular, point_index=pidx1)
    kf2 = make_kf(rows2, p2, stereo=not monocular, point_index=pidx2)
    median = scene_median_depth(pidx2, p2, points["pos"], 2)[0] if monocular else np.nan
    c2 = CAM_N if cam2 is None else cam2
    return Case(name, kf1, kf2, match12, monocular, median, CAM_N, c2, cursor=n_exist,
                capacity=n_exist + n_match + 5, tags=tags, points=points)


def natural_cases():
    return [
        natural_case("nat_mono_300", 11, 300, True, tags=("natural", "mono")),
        natural_case("nat_stereo_200", 12, 200, False, tags=("natural", "stereo")),
        natural_case("nat_stereo_far_120", 13, 120, False, stereo_frac=0.9, z_range=(30.0, 120.0),
                     tags=("natural", "stereo", "unproject")),
        natural_case("nat_mono_100", 14, 100, True, baseline=(0.3, 0.4, -0.2),
                     tags=("natural", "mono")),
    ]


# ----------------------------------------------------------- directed cases
def _one(kp1, kp2, p1, p2, cam1=CAM_D, cam2=CAM_D, sw=frozenset()):
    tr = {}
    g = lambda k, j: k[j] if len(k) > 3 else -1.0
    st = triangulate_match(
        dict(x=kp1[0], y=kp1[1], octave=kp1[2]), g(kp1, 3), g(kp1, 4),
        dict(x=kp2[0], y=kp2[1], octave=kp2[2]), g(kp2, 3), g(kp2, 4), p1, p2, cam1, cam2,
        SCALE_FACTORS, LEVEL_SIGMA2, False, sw, tr)[0]
    return st, tr


def bisect_f32(lo, hi, pred):
    """Adjacent floats (a, b) by bit pattern, between lo and hi (same sign), with
    pred(a) == pred(lo) != pred(b) == pred(hi)."""
    a, b = f32_bits(lo), f32_bits(hi)
    pa = pred(f32_from_bits(a))
    assert pa != pred(f32_from_bits(b)), "the bracket does not straddle the threshold"
    while abs(b - a) > 1:
        m = (a + b) // 2
        if pred(f32_from_bits(m)) == pa:
            a = m
        else:
            b = m
    return f32_from_bits(a), f32_from_bits(b)


def directed_cases():
    cases = []
    P0 = pose_rec(I3, (0, 0, 0))
    Px = pose_rec(I3, (-1, 0, 0))  # centre (1, 0, 0)
    mono = dict(monocular=True, median=10.0)

    def add(name, kps1, kps2, p1, p2, tags, match=None, stereo=True, **kw):
        m = list(range(len(kps1))) if match is None else match
        cases.append(Case(name, make_kf(kps1, p1, stereo), make_kf(kps2, p2, stereo), m,
                          tags=tags, **kw))

    # no match / undefined / counts 0 and 1
    add("empty", [], [], P0, Px, ("count0",), stereo=False, **mono)
    add("no_match_only", [(300, 200, 0)], [(300, 200, 0)], P0, Px, ("no_match", "count0"),
        match=[-1], stereo=False, **mono)
    add("undefined_kinds",
        [(371.2, 265.6, 0), (371.2, 265.6, 8), (371.2, 265.6, 0), (371.2, 265.6, 0, 358.4, 0.0),
         (371.2, 265.6, 0), (371.2, 265.6, -1)],
        [(268.8, 265.6, 0), (268.8, 265.6, 0), (268.8, 265.6, 0, 256.0, -1.0),
         (268.8, 265.6, 0), (268.8, 265.6, 9)], P0, Px,
        ("undefined_index", "undefined_octave", "undefined_depth"), match=[0, 1, 2, 3, 7, 4])

    # low parallax: cosParallaxRays on both sides of 0.9998 (monocular)
    lo_hi = bisect_f32(309.0, 310.5,
                       lambda u2: _one((320, 240, 0), (u2, 240, 0), P0, Px)[0] == LOW_PARALLAX)
    add("low_parallax_edge", [(320, 240, 0), (320, 240, 0)],
        [(lo_hi[0], 240, 0), (lo_hi[1], 240, 0)], P0, Px, ("low_parallax_edge",), stereo=False,
        **mono)
    add("coincident_rays", [(320, 240, 0), (320, 240, 0, 304.0, 4.0)],
        [(320, 240, 0), (320, 240, 0)], P0, pose_rec(I3, (0, 0, -1)), ("coincident",))
    # cosParallaxRays == 0 exactly (perpendicular rays) and just above
    add("rays_zero", [(832, 240, 0), (f32_next(832.0, False), 240, 0)],
        [(-192, 240, 0), (-192, 240, 0)], P0, Px, ("rays_zero",), stereo=False, **mono)

    # z1 == 0 and the float above (x3D = UnprojectStereo(idx2) = (0, 0, 4))
    for name, tz in (("z1_zero", f32(-4)), ("z1_above", f32_next(-4.0, True))):
        add(name, [(320, 240, 0)], [(320, 240, 0, 304.0, 4.0)], pose_rec(I3, (0, 0, tz)), P0,
            ("z1_edge", "branch_st2"))
    # z2 == 0 and the float above (x3D = UnprojectStereo(idx1) = (0, 0, 4))
    for name, tz in (("z2_zero", f32(-4)), ("z2_above", f32_next(-4.0, True))):
        add(name, [(320, 240, 0, 304.0, 4.0)], [(320, 240, 0)], P0, pose_rec(I3, (0, 0, tz)),
            ("z2_edge", "branch_st1"))

    # reprojection thresholds: the point (0.5, 0.25, 5) seen from P0 and Px; the
    # coarser octave on the other side keeps its threshold out of the way
    u1, v1, u2, v2 = 371.2, 265.6, 268.8, 265.6
    a, b = bisect_f32(v1, v1 + 20, lambda v: _one((u1, v, 0), (u2, v2, 3), P0, Px)[0] == REPROJ1)
    add("reproj1_mono_edge", [(u1, a, 0), (u1, b, 0)], [(u2, v2, 3), (u2, v2, 3)], P0, Px,
        ("reproj1_edge", "chi2_mono"), stereo=False, **mono)
    a, b = bisect_f32(v2, v2 + 6.5, lambda v: _one((u1, v1, 3), (u2, v, 0), P0, Px)[0] == REPROJ2)
    add("reproj2_mono_edge", [(u1, v1, 3), (u1, v1, 3)], [(u2, a, 0), (u2, b, 0)], P0, Px,
        ("reproj2_edge", "chi2_mono"), stereo=False, **mono)
    ur1, ur2 = u1 - 64.0 / 5, u2 - 64.0 / 5
    a, b = bisect_f32(ur1, ur1 + 20,
                      lambda r: _one((u1, v1, 0, r, 5.0), (u2, v2, 3), P0, Px)[0] == REPROJ1)
    add("reproj1_stereo_edge", [(u1, v1, 0, a, 5.0), (u1, v1, 0, b, 5.0)],
        [(u2, v2, 3), (u2, v2, 3)], P0, Px, ("reproj1_edge", "chi2_stereo"))
    a, b = bisect_f32(ur2, ur2 + 20,
                      lambda r: _one((u1, v1, 3), (u2, v2, 0, r, 5.0), P0, Px)[0] == REPROJ2)
    add("reproj2_stereo_edge", [(u1, v1, 3), (u1, v1, 3)],
        [(u2, v2, 0, a, 5.0), (u2, v2, 0, b, 5.0)], P0, Px, ("reproj2_edge", "chi2_stereo"))

    # zero distance: KF2's camera centre written onto the point (its tcw says
    # otherwise: the pose record's ow is an input like any other), and one float off
    for name, oz in (("dist2_zero", f32(4)), ("dist2_above", f32_next(4.0, True))):
        add(name, [(320, 240, 0, 304.0, 4.0)], [(320, 240, 0)], P0,
            pose_rec(I3, (0, 0, 1), ow=(0, 0, oz)), ("zero_dist_edge",))
    for name, oz in (("dist1_zero", f32(4)), ("dist1_below", f32_next(4.0, False))):
        add(name, [(320, 240, 0)], [(320, 240, 0, 304.0, 4.0)],
            pose_rec(I3, (0, 0, 1), ow=(0, 0, oz)), P0, ("zero_dist_edge",))

    # scale ratio: ratioDist == ratioOctave * ratioFactor exactly, and one float above
    rf = f32(1.5) * SCALE_FACTORS[1]
    oz = f32(1) - rf  # exact
    for name, o in (("ratio_eq", oz), ("ratio_above", f32_next(oz, False))):
        add(name, [(320, 240, 0, 256.0, 1.0)], [(320, 240, 0)], P0,
            pose_rec(I3, (0, 0, -o), ow=(0, 0, o)), ("ratio_edge",))

    # the SVD's own edges: A with orthogonal columns (every pair under the epsilon)
    xk1, xk2 = (576, 240, 0), (64, 240, 0)  # xn1 = (0.5, 0), xn2 = (-0.5, 0)
    add("svd_tie", [xk1], [xk2], pose_rec(I3, (1, -0.5, 2)), pose_rec(I3, (-1, 0.5, 2)),
        ("svd_orthogonal", "svd_tie"), stereo=False, monocular=True, median=1.0)
    add("w_zero", [xk1], [xk2], pose_rec(I3, (1, -0.75, 2)), pose_rec(I3, (-1, 0.75, 2)),
        ("svd_orthogonal", "w_zero"), stereo=False, monocular=True, median=1.0)
    e = f32(2.0 ** -24)
    add("svd_eps_edge", [xk1], [xk2], pose_rec(I3, (f32(0.5) - e, -0.25, 1)),
        pose_rec(I3, (f32(-0.5) + e, 0.25, 1)), ("svd_eps_edge",), stereo=False, monocular=True,
        median=1.0)

    # the `else if` of :372 decides: KF1's keypoint is stereo and far, KF2's stereo and near
    Pq = pose_rec(I3, (-0.2, 0, 0))
    add("else_if_quirk", [(320, 240, 0, 320 - 0.64, 100.0)], [(294.4, 240, 0, 294.4 - 64.0, 1.0)],
        P0, Pq, ("quirk_else_if",))
    # KF2's u_r uses KF1's mbf (:480): consistent with cam1's bf, not with cam2's
    cam2 = (512.0, 512.0, 320.0, 240.0, 128.0, 0.25)
    add("kf1_bf_quirk", [(u1, v1, 0)], [(u2, v2, 0, u2 - 64.0 / 5, 5.0)], P0, Px,
        ("quirk_bf",), cam2=cam2)
    # cosParallaxRays == cosParallaxStereo1 exactly, and the depth one float above
    cr = _one((u1, v1, 0, 0.0, 5.0), (345.6, v1, 0), P0, Pq)[1]["cos_rays"]
    a, b = bisect_f32(1.0, 60.0, lambda d: cos_stereo(CAM_D[5], d) > cr)
    assert cos_stereo(CAM_D[5], a) == cr
    add("rays_eq_stereo", [(u1, v1, 0, u1 - 64.0 / float(a), a), (u1, v1, 0, u1 - 64.0 / float(b), b)],
        [(345.6, v1, 0), (345.6, v1, 0)], P0, Pq, ("rays_eq",))

    # the gates
    add("gate_stereo_eq", [(u1, v1, 0)], [(u2, v2, 0)], P0, pose_rec(I3, (-0.125, 0, 0)),
        ("gate_stereo_edge",))
    add("gate_stereo_below", [(u1, v1, 0)], [(u2, v2, 0)], P0,
        pose_rec(I3, (f32_next(-0.125, True), 0, 0)), ("gate_stereo_edge", "gated"))
    g = f32(0.01)  # below 0.01 as a double
    add("gate_mono_below", [(u1, v1, 0)], [(u2, v2, 0)], P0, pose_rec(I3, (-g, 0, 0)),
        ("gate_mono_edge", "gated"), stereo=False, monocular=True, median=1.0)
    add("gate_mono_above", [(u1, v1, 0)], [(u2, v2, 0)], P0,
        pose_rec(I3, (-f32_next(g, True), 0, 0)), ("gate_mono_edge",), stereo=False,
        monocular=True, median=1.0)
    add("gate_mono_nan", [(u1, v1, 0)], [(u2, v2, 0)], P0, Px, ("gate_nan", "gated"),
        stereo=False, monocular=True, median=np.nan)
    return cases


def pattern_cases():
    """Match counts around the wave and the workgroup with accept patterns."""
    cases = []
    seed = 100
    for n in (1, 63, 64, 65, WG + 1):
        pats = {"all": np.ones(n, bool), "none": np.zeros(n, bool),
                "alt": np.arange(n) % 2 == 0, "last": np.arange(n) == n - 1}
        if n > 64:
            pats["wave2_first"] = np.arange(n) == 64
        if n > WG:
            pats["round2_first"] = np.arange(n) == WG
        if n == 1:
            pats = {"all": pats["all"], "none": pats["none"]}
        for pname, acc in pats.items():
            seed += 1
            c = natural_case(f"pat_{n}_{pname}", seed, n, True, n_extra=0, n_exist=4,
                             z_range=(4.0, 20.0), accept=acc, tags=("pattern", f"count{n}", pname))
            c.accept = acc
            cases.append(c)
    return cases


def capacity_cases():
    """A cursor that ends exactly at point_capacity, and one past it."""
    base = natural_case("cap_probe", 21, 40, False, tags=())
    n_new = int(base.ref()["info"]["n_new"])
    out = []
    for name, cap, tag in (("cap_exact", base.cursor + n_new, "cap_exact"),
                           ("cap_over", base.cursor + n_new - 1, "cap_over")):
        c = natural_case(name, 21, 40, False, tags=(tag,))
        c.capacity = cap
        out.append(c)
    return out


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = natural_cases() + directed_cases() + pattern_cases() + capacity_cases()
        assert len({c.name for c in _ALL}) == len(_ALL)
    return _ALL


def median_cases():
    """(name, point_index, pose, points_pos, q): 0, 1, 2, an even count, ties, q = 3."""
    rng = np.random.default_rng(5)
    R, t, _ = scenarios.pose(rng)
    p = pose_rec(R, t)
    pos = np.zeros((12, 3), f32)
    pos[:, 0] = rng.uniform(-3, 3, 12)
    pos[:, 1] = rng.uniform(-2, 2, 12)
    pos[:, 2] = rng.uniform(3, 30, 12)
    pos[7] = pos[3]            # ties
    pos[8] = pos[3]
    mk = lambda idx, n=14: np.array(list(idx) + [-1] * (n - len(idx)), np.int32)
    return [
        ("median_0", mk([]), p, pos, 2),
        ("median_1", mk([4]), p, pos, 2),
        ("median_2", mk([-1, 4, -1, 9]), p, pos, 2),
        ("median_even6", mk([0, 1, -1, 2, 5, 6, -3, 10]), p, pos, 2),
        ("median_ties", mk([3, 0, 7, 8, 11]), p, pos, 2),
        ("median_all_tied", mk([3, 7, 8]), p, pos, 2),
        ("median_q3", mk([0, 1, 2, 3, 4, 5, 6]), p, pos, 3),
        ("median_neg", mk([0, 1, 2]), pose_rec(I3, (0, 0, -50)), pos, 2),
    ]


# ------------------------------------------------------------------ packing
def pack(cases, stride):
    """The arrays of one batch call: problem p = slots 2p and 2p + 1 and cursor
    p.  The problems share one `points` array; problem p's window starts at
    base[p] (its point indices and its cursor are the case's plus base[p]) and
    is case.capacity records long; the call's point_capacity is the total."""
    n = len(cases)
    keys = np.zeros((2 * n, stride), KEYPOINT_DTYPE)
    ur = np.full((2 * n, stride), -1, f32)
    depth = np.full((2 * n, stride), -1, f32)
    pidx = np.full((2 * n, stride), -9, np.int32)
    pose = np.zeros(2 * n, POSE_DTYPE)
    nkeys = np.zeros(2 * n, np.int32)
    m12 = np.full((n, stride), 5, np.int32)  # junk past the count: a valid-looking index
    base = np.concatenate([[0], np.cumsum([c.capacity for c in cases])]).astype(np.int32)
    points = junk_points(int(base[-1]))
    cursor = np.zeros(n, np.int32)
    for p, c in enumerate(cases):
        for j, kf in enumerate((c.kf1, c.kf2)):
            k = len(kf["keys"])
            assert k <= stride
            s = 2 * p + j
            keys[s, :k], nkeys[s], pose[s] = kf["keys"], k, kf["pose"]
            pi = kf["point_index"]
            pidx[s, :k] = np.where(pi >= 0, pi + base[p], pi)
            if kf["u_right"] is not None:
                ur[s, :k], depth[s, :k] = kf["u_right"], kf["depth"]
        m12[p, :len(c.match12)] = c.match12
        if c.points is not None:
            points[base[p]:base[p] + len(c.points)] = c.points
        cursor[p] = base[p] + c.cursor
    return dict(keys=keys, u_right=ur, depth=depth, point_index=pidx, pose=pose, nkeys=nkeys,
                match12=m12, kf1_slot=np.arange(0, 2 * n, 2, dtype=np.int32),
                kf2_slot=np.arange(1, 2 * n, 2, dtype=np.int32),
                median=np.array([c.median for c in cases], f32), base=base, points=points,
                cursor=cursor, cursor_index=np.arange(n, dtype=np.int32))


def groups(cases):
    """Cases that one batch call can hold: the same cameras and mode."""
    out = {}
    for c in cases:
        out.setdefault((c.cam1, c.cam2, c.monocular), []).append(c)
    return list(out.values())
