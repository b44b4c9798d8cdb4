"""Directed inputs for k_pose_optimization (test infrastructure): problems built
or searched so that the reference (tests/poseopt_ref.py) reaches the paths the
seeded KITTI-like cases of poseopt_cases.py never do -- every pivot pair of the
6x6 LDLT, the largest-diagonal branches of Quaterniond(Matrix3d), the sign flip
of normalizeRotation, the quadrants of the pinned sin / cos, each termination
rule, rounds without an active edge, chi2 exactly at a threshold, the
mono / stereo flag at +-0, NaN and a denormal, level tables of 1, 3 and 16
entries, non-finite and extreme inputs, and the tile and chunk boundaries of the
ordered sums and of the compaction.

CASES maps a name to (builder, census minimum).  A builder returns a dict in the
shape poseopt_cases.make_case returns, with `cam` and `levels` where they differ
from poseopt_cases.CAM / INV_LEVEL_SIGMA2, so poseopt_cases.run_ref and the GPU
helpers of test_gpu_poseopt.py take it as it is.  Searched cases commit the
generator and the chosen seeds, never arrays; test_poseopt_edge_cases.py asserts
the census of each, so a drift of the generator fails there."""
from __future__ import annotations

import functools
import math

import numpy as np

import poseopt_cases as pc
import poseopt_ref as ref
from rgbd_cases import KEYPOINT_DTYPE

f32, f64 = np.float32, np.float64
SENTINEL = pc.SENTINEL
ORB_MAX_LEVELS = 16


# ---------------------------------------------------------------- generators
def _axis_angle_pose(axis, angle, t=(0.0, 0.0, 0.0)):
    """POSE_DTYPE record of the rotation by `angle` about `axis` and translation t."""
    a = np.asarray(axis, f64)
    a = a / math.sqrt(float((a * a).sum()))
    s, c = math.sin(angle / 2), math.cos(angle / 2)
    return pc.pose_record(([float(a[0] * s), float(a[1] * s), float(a[2] * s), c],
                           [float(v) for v in t]))


def _matrix_pose(R, t=(0.0, 0.0, 0.0)):
    """POSE_DTYPE record of the float32 matrix R as given (mOw by the float rule)."""
    p = np.zeros(1, pc.POSE_DTYPE)
    R = np.asarray(R, f32).reshape(3, 3)
    tc = np.asarray(t, f32)
    p["rcw"], p["tcw"] = R.reshape(9), tc
    p["ow"] = [-(f32(f32(R[0, i] * tc[0]) + f32(R[1, i] * tc[1])) + f32(R[2, i] * tc[2]))
               for i in range(3)]
    return p


def _keys(n, octave=0):
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["size"], k["class_id"], k["octave"] = 31.0, -1, octave
    return k


def synth(seed, n_edges, kind="mixed", fx=500.0, ratio=1.0, depth=10.0, spread=0.3, axis=None,
          angle=0.0, tscale=0.5, twist=(.02, .02, .02, .2, .2, .2), noise=1.0, outlier_frac=0.2,
          n_kp=None, slots=None, levels=None, octaves=None, planted=None, gross=(25, 60)):
    """One seeded problem with its own camera (fx, fy = ratio fx, principal point
    (320, 240), bf = fx / 2): the start pose turns by `angle` about `axis` (a
    random axis when None) and sits tscale away; the generating pose is the
    twist (a normal draw scaled by `twist`) applied to it; the points lie at
    depth (1..10) x `depth` in the generating camera's frame, `spread` wide.
    slots: the keypoint slots of the edges (random when None); planted: the edge
    positions that get a gross error (a random outlier_frac of them when None)."""
    rng = np.random.default_rng(seed)
    cam = tuple(f32(v) for v in (fx, fx * ratio, 320.0, 240.0, fx * 0.5, 0.5))
    fx, fy, cx, cy, bf = (float(c) for c in cam[:5])
    ax = rng.normal(0, 1, 3) if axis is None else np.asarray(axis, f64)
    pose = _axis_angle_pose(ax, angle, rng.normal(0, 1, 3) * tscale)
    start = ref.to_se3quat(pose["rcw"][0], pose["tcw"][0])
    truth = ref.se3_mul(ref.se3_exp(list(rng.normal(0, 1, 6) * np.asarray(twist, f64))), start)
    n_pts = n_edges + 7
    zc = rng.uniform(1, 10, n_pts) * depth
    Pc = np.stack([rng.uniform(-1, 1, n_pts) * spread * zc, rng.uniform(-1, 1, n_pts) * spread * zc,
                   zc], 1)
    qi = [-truth[0][0], -truth[0][1], -truth[0][2], truth[0][3]]
    d = Pc - np.array(truth[1])
    Xw = np.stack(ref.quat_rotate(qi, d[:, 0], d[:, 1], d[:, 2]), 1).astype(f32)
    n_kp = n_edges * 5 // 4 + 3 if n_kp is None else n_kp
    lv = pc.INV_LEVEL_SIGMA2 if levels is None else np.asarray(levels, f32)
    keys = _keys(n_kp)
    keys["x"], keys["y"] = rng.uniform(0, 640, n_kp), rng.uniform(0, 480, n_kp)
    keys["octave"] = rng.integers(0, len(lv), n_kp)
    if slots is None:
        slots = np.sort(rng.choice(n_kp, n_edges, replace=False))
    slots = np.asarray(slots)
    if octaves is not None:
        keys["octave"][slots] = octaves
    pts = rng.permutation(n_pts)[:n_edges]
    point_index = np.full(n_kp, -1, np.int32)
    point_index[slots] = pts
    x, y, z = ref.quat_rotate(truth[0], *(Xw[pts].astype(f64).T))
    x, y, z = x + truth[1][0], y + truth[1][1], z + truth[1][2]
    u, v = x / z * fx + cx, y / z * fy + cy
    obs = np.stack([u, v, u - bf / z], 1)
    if noise:
        obs = obs + rng.normal(0, noise, obs.shape)
    bad = rng.random(n_edges) < outlier_frac
    if planted is not None:
        bad = np.zeros(n_edges, bool)
        bad[list(planted)] = True
    obs[bad] += rng.choice([-1, 1], (int(bad.sum()), 3)) * rng.uniform(*gross, (int(bad.sum()), 3))
    keys["x"][slots], keys["y"][slots] = obs[:, 0], obs[:, 1]
    st = {"mono": np.zeros(n_edges, bool), "stereo": np.ones(n_edges, bool),
          "mixed": rng.random(n_edges) < 0.5}[kind]
    u_right = np.full(n_kp, -1, f32)
    u_right[slots] = np.where(st, np.maximum(obs[:, 2], 0.0), -1.0)
    c = dict(keys=keys, u_right=None if kind == "mono" else u_right, point_index=point_index,
             points=Xw, pose=pose, outlier=np.full(n_kp, SENTINEL, np.uint8), planted=slots[bad],
             slots=slots, truth=truth, kind=kind, cam=cam)
    if levels is not None:
        c["levels"] = lv
    return c


def wild(seed):
    """The search space of the pivot and quaternion cases: one draw of edge
    count, kind, focal lengths, depth, spread, start rotation and distance."""
    rng = np.random.default_rng(10_000 + seed)
    axis = None if rng.random() < 0.5 else np.eye(3)[rng.integers(3)]
    return synth(seed, int(rng.integers(3, 41)), ("mono", "stereo", "mixed")[int(rng.integers(3))],
                 fx=float(rng.choice([1.0, 30.0, 500.0, 5000.0])),
                 ratio=float(rng.choice([0.2, 1.0, 5.0])),
                 depth=float(10.0 ** rng.uniform(math.log10(0.05), 3)),
                 spread=float(10.0 ** rng.uniform(-3, 0)),
                 axis=axis, angle=float(rng.choice([0.0, 0.1, 1.0, 2.2, 3.0, math.pi])),
                 tscale=float(rng.choice([0.0, 0.5, 10.0, 100.0])),
                 twist=tuple(np.array([.02, .02, .02, .2, .2, .2]) * float(rng.choice([0, 1, 4, 20]))))


@functools.lru_cache(maxsize=None)
def run(name):
    """(case, reference result) of a named case, computed once per process."""
    c = CASES[name][0]()
    return c, pc.run_ref(c)


def _wild(seed):
    return lambda: wild(seed)


# ------------------------------------------------------------------- 1. pivots
# The pivot cases are wild(640, 512, 581, 473, 184, 741, 143, 17), chosen by a
# greedy cover of the first 1,500 seeds of wild(): every one of the 21 (k, idx)
# pairs is reached by at least three of the first six problems, which mix mono,
# stereo and mixed edges; (0, 0), no swap at k = 0, occurs in five of them.
# 143 is a mono problem with fx = fy: H(3, 3) and H(4, 4) are then the same sum,
# bit for bit, a tie of equal |diagonal| that "last largest" resolves
# differently; in 17 the factorisation without pivoting gives another result.
# (The rarest pair is (0, 4), reached by 78 of the 1,500 seeds; the 32-edge
# half tiles and 64-edge chunks of the kernel are the business of section 9.)
ALL_PIVOTS = frozenset((k, i) for k in range(6) for i in range(k, 6))


# ------------------------------------------------------ 2. quaternion branches
def _start(seed, pose=None, **kw):
    kw.setdefault("kind", "mixed")
    c = synth(seed, 12, noise=0.5, outlier_frac=0.2, **kw)
    if pose is not None:
        # the exact matrix in place of the rounded axis-angle one the scene was made around
        c["pose"] = pose
    return c


def _near_pi(ax):
    return lambda: _start(200 + ax, axis=np.eye(3)[ax], angle=3.1)


def _exactly_pi(ax):
    d = -np.ones(3)
    d[ax] = 1.0
    return lambda: _start(210 + ax, pose=_matrix_pose(np.diag(d), (0.1, -0.2, 0.3)),
                          axis=np.eye(3)[ax], angle=math.pi)


def _perm120():
    """The rotation by 120 degrees about (1, 1, 1): trace exactly 0 and the
    three diagonal entries tie at 0, so the first is the 'largest'."""
    return _start(220, pose=_matrix_pose([[0, 0, 1], [1, 0, 0], [0, 1, 0]], (0.1, -0.2, 0.3)),
                  axis=(1.0, 1.0, 1.0), angle=2 * math.pi / 3)


def _qw_negative():
    """3.18 rad about x: the matrix is that of -3.10 rad, the largest-diagonal
    branch extracts qx > 0 with qw < 0 and normalizeRotation flips the sign."""
    return _start(230, axis=(1.0, 0.0, 0.0), angle=3.18)


# ------------------------------------------------- 5. thresholds, symmetrically
def _grid():
    """Offsets d in [2, 3) that 320 +- d holds exactly in float32 (multiples of
    2^-15) and, for each, the float32 weights within 3 ulps of 5.991 / d^2 and
    of 7.815 / d^2: (d, s, chi2 = d (s d)) as flat float64 arrays."""
    d = np.arange(2 * 2 ** 15, 3 * 2 ** 15, dtype=f64) / 2 ** 15
    out = []
    for target in (5.991, 7.815):
        s0 = (target / (d * d)).astype(f32)
        for k in range(-3, 4):
            s = s0.copy()
            for _ in range(abs(k)):
                s = np.nextafter(s, f32(np.inf if k > 0 else 0))
            out.append((d, s.astype(f64)))
    dd = np.concatenate([o[0] for o in out])
    ss = np.concatenate([o[1] for o in out])
    return dd, ss, dd * (ss * dd)


def threshold_edges():
    """The (d, s) pairs of the symmetric case, each named: chi2 narrows to the
    float32 threshold exactly / to the float above it (mono 5.991f, stereo
    7.815f), and the doubles closest to the squared Huber widths from below
    (<=) and from above that float32 offsets and weights give."""
    dd, ss, chi = _grid()
    cf = chi.astype(f32)
    out = {}
    for kind, T in (("mono", ref.CHI2_MONO), ("stereo", ref.CHI2_STEREO)):
        for name, want in (("at", T), ("above", np.nextafter(T, f32(np.inf)))):
            i = int(np.nonzero(cf == want)[0][0])
            out["%s_%s" % (kind, name)] = (float(dd[i]), float(ss[i]), float(chi[i]))
    for kind, delta in (("mono", ref.DELTA_MONO), ("stereo", ref.DELTA_STEREO)):
        g = chi - delta * delta
        lo = int(np.argmax(np.where(g <= 0, g, -np.inf)))
        hi = int(np.argmin(np.where(g > 0, g, np.inf)))
        out["huber_%s_le" % kind] = (float(dd[lo]), float(ss[lo]), float(chi[lo]))
        out["huber_%s_gt" % kind] = (float(dd[hi]), float(ss[hi]), float(chi[hi]))
    return out


SYM_CAM = tuple(f32(v) for v in (500.0, 400.0, 320.0, 240.0, 64.0, 0.128))


def _symmetric(pairs, cam=SYM_CAM):
    """Identity pose, integer principal point, every point on the optical
    axis; per entry (kind, d, s) of `pairs` two adjacent edges on one point,
    observed at (cx + d, cy) and (cx - d, cy) at a level of weight s (a stereo
    point sits at z = 1, where 1.0f / z and bf / z are exact, and both edges
    carry the exact right coordinate cx - bf).  The two edges' terms of b cancel
    exactly, so the step is zero, rho is 0 and the estimate never moves; every
    chi2 is d (s d)."""
    cx, cy, bf = float(cam[2]), float(cam[3]), float(cam[4])
    n = 2 * len(pairs) + 3
    keys = _keys(n)
    keys["x"], keys["y"] = 7.0, 9.0
    ur = np.full(n, -1, f32)
    idx = np.full(n, -1, np.int32)
    pts = np.zeros((len(pairs) + 2, 3), f32)
    pts[:, 2] = 50.0
    levels = []
    for p, (kind, d, s) in enumerate(pairs):
        if f32(s) not in levels:
            levels.append(f32(s))
        pts[p] = (0.0, 0.0, 1.0 if kind == "stereo" else 2.0 + p)
        for j, sign in enumerate((1.0, -1.0)):
            slot = 1 + 2 * p + j  # slot 0 and the last two carry no edge
            assert float(f32(cx + sign * d)) == cx + sign * d
            keys["x"][slot], keys["y"][slot] = cx + sign * d, cy
            keys["octave"][slot] = levels.index(f32(s))
            idx[slot] = p
            if kind == "stereo":
                ur[slot] = cx - bf
    assert len(levels) <= ORB_MAX_LEVELS
    pose = _matrix_pose(np.eye(3))
    return dict(keys=keys, u_right=ur, point_index=idx, points=pts, pose=pose,
                outlier=np.full(n, SENTINEL, np.uint8), slots=np.nonzero(idx >= 0)[0], kind="mixed",
                cam=cam, levels=np.array(levels, f32), pairs=pairs)


SYM_ORDER = ("mono_at", "mono_above", "stereo_at", "stereo_above", "huber_mono_le", "huber_mono_gt",
             "huber_stereo_le", "huber_stereo_gt")


def sym_thresholds():
    t = threshold_edges()
    return _symmetric([("stereo" if "stereo" in k else "mono",) + t[k][:2] for k in SYM_ORDER])


def sym_huber_exact():
    """Principal point (0, 0): the offset may be any float32, and d = delta with
    weight 1 gives chi2 = delta^2 exactly, the equality of e <= dsqr, for both
    widths.  The third pair is one float32 further out.  Six pairs keep the
    problem at twelve edges, so all four rounds run."""
    cam = tuple(f32(v) for v in (500.0, 400.0, 0.0, 0.0, -64.0, 0.128))   # (cx - bf = 64 >= 0)
    dm, ds = f32(ref.DELTA_MONO), f32(ref.DELTA_STEREO)
    up = lambda v: float(np.nextafter(v, f32(np.inf)))
    return _symmetric([("mono", float(dm), 1.0), ("stereo", float(ds), 1.0), ("mono", up(dm), 1.0),
                       ("stereo", up(ds), 1.0), ("mono", 1.0, 1.0), ("stereo", 1.0, 1.0)], cam)


# ---------------------------------------------------- 6. the mono / stereo flag
NEG_DENORMAL = np.array([0x80000001], np.uint32).view(f32)[0]   # the negative float32 nearest zero
POS_DENORMAL = np.array([0x00000001], np.uint32).view(f32)[0]


def _flag_base(seed):
    c = synth(seed, 14, "mixed", noise=0.5, outlier_frac=0.0, twist=(.01, .01, .01, .05, .05, .05))
    return c, c["slots"]


def flag_zeros():
    """mvuRight of +0.0, -0.0 (stereo under !(ur < 0)), the negative denormal
    (mono: a flushed compare would call it stereo) and -1.0, on edges that were
    stereo; a point and observations with denormal and -0.0 components."""
    c, s = _flag_base(300)
    c["u_right"][s[:5]] = [0.0, -0.0, NEG_DENORMAL, -1.0, POS_DENORMAL]
    c["flag_slots"] = s[:5]
    p = c["point_index"][s[5:8]]
    c["points"][p[0], 0] = NEG_DENORMAL
    c["points"][p[1], 1] = f32(-0.0)
    c["points"][p[2], 0] = POS_DENORMAL
    c["keys"]["x"][s[8]], c["keys"]["y"][s[9]] = f32(-0.0), POS_DENORMAL
    return c


def flag_nan():
    """mvuRight NaN is stereo under !(ur < 0): its e2 is NaN from the first pass on."""
    c, s = _flag_base(301)
    c["u_right"][s[2]] = f32(np.nan)
    c["flag_slots"] = s[2:3]
    return c


# -------------------------------------------------------------------- 7. levels
def _levels(n_levels, bad=False):
    """n_levels entries with a zero and a denormal weight among them (from three
    levels up), an edge at the top octave; bad: one edge at octave == n_levels."""
    lv = (f32(1.0) / f32(1.2) ** (2 * np.arange(n_levels))).astype(f32)
    if n_levels >= 3:
        lv[1], lv[n_levels - 1] = 0.0, POS_DENORMAL
    if n_levels == ORB_MAX_LEVELS:
        lv[7] = f32(2.5)

    def build():
        c = synth(310 + n_levels, 16, "mixed", noise=0.5, levels=lv,
                  octaves=(np.arange(16) + n_levels - 1) % n_levels)
        assert c["keys"]["octave"][c["slots"][0]] == n_levels - 1
        if bad:
            c["keys"]["octave"][c["slots"][9]] = n_levels
            c["keys"]["octave"][np.nonzero(c["point_index"] < 0)[0][0]] = n_levels + 3  # never read
        return c
    return build


# ------------------------------------------------- 8. non-finite, extreme inputs
def _extreme(what):
    def build():
        c = synth(320, 20, "mixed", noise=0.5, outlier_frac=0.2)
        s = c["slots"]
        if what == "nan_point":
            c["points"][c["point_index"][s[4]], 1] = np.nan
        elif what == "inf_observation":
            c["keys"]["x"][s[6]] = np.inf
        elif what == "nan_pose":
            c["pose"]["rcw"][0][4] = np.nan
        elif what == "huge_tiny_points":
            c["points"][c["point_index"][s[3]]] = (1e30, -1e30, 1e30)
            c["points"][c["point_index"][s[11]]] = (1e-30, 1e-30, 1e-30)
        elif what == "huge_camera":
            c["cam"] = tuple(f32(v) for v in (3e38, 3e38, 320.0, 240.0, 3e38, 0.5))
        elif what == "tiny_depth":
            # the smallest depths a float32 point gives at the identity pose: the
            # denormal 1.4e-45 (invz = 7e44, invz * invz = 5e89: a float32 depth
            # cannot overflow it) under coordinates of 3e38, whose products with
            # invz * invz and fx pass 1e169, and 1e-30; every pivot stays positive or NaN
            c["pose"] = _matrix_pose(np.eye(3))
            c["points"][c["point_index"][s], :] = (0, 0, 1e-30)
            c["points"][c["point_index"][s[::2]]] = (3e38, -3e38, POS_DENORMAL)
        return c
    return build


# -------------------------------------------------------- 9. accumulation order
def _acc(seed, planted, **kw):
    return lambda: synth(seed, 65, "mixed", noise=0.3, planted=planted, n_kp=80,
                         twist=(.005, .005, .005, .05, .05, .05), **kw)


# ------------------------------------------------------------------ 10. compaction
def compact_chunks():
    """193 = 3 x 64 + 1 keypoint slots: the first 64-slot chunk is full of
    edges, the second and third hold none, the last slot (n - 1) holds one."""
    return synth(340, 65, "mixed", noise=0.5, n_kp=193, slots=list(range(64)) + [192])


def compact_ends():
    """129 slots, edges at slot 0 and slot 128 and a few between."""
    return synth(341, 12, "stereo", noise=0.5, n_kp=129,
                 slots=[0, 5, 30, 31, 32, 63, 64, 65, 100, 126, 127, 128])


def negative_level_weight():
    """isPositive() == false: a level whose invSigma2 is negative (the ABI takes
    any float) makes H indefinite, LDLT meets a negative pivot without a NaN,
    the solver reports failure, x keeps its value and the trial counts as
    rejected with chi2 = DBL_MAX.  No other input reached this."""
    lv = pc.INV_LEVEL_SIGMA2.copy()
    lv[3] = f32(-0.3)
    return synth(400, 30, "mixed", noise=1.5, outlier_frac=0.3, levels=lv,
                 twist=(.05, .05, .05, .4, .4, .4))


# ----------------------------------------------------------------------- census
def census(c, r):
    """What the reference reached on case c (r = its result)."""
    t = r["trace"]
    out = {k: t[k] for k in ("pivots", "pivot_ties", "quat_start", "quat_step", "flips", "quadrants",
                             "exp_small", "exp_large", "ended", "skipped_rounds",
                             "outlier_to_inlier", "stale_changed_flags", "not_positive", "n_mono",
                             "n_stereo", "rounds", "huber_inlier", "huber_outlier")}
    out.update(n_edges=r["n_edges"], n_inliers=r["n_inliers"], lm_iterations=r["lm_iterations"],
               rejected_trials=r["rejected_trials"], n_keypoints=len(c["keys"]),
               n_levels=len(c.get("levels", pc.INV_LEVEL_SIGMA2)),
               finite_pose=bool(np.isfinite(np.concatenate([r["rcw"], r["tcw"], r["ow"]])).all()),
               active_after_round1=(tuple(e for e in range(max(r["n_edges"], 0))
                                          if e not in t["round_outliers"][0])
                                    if t["round_outliers"] else ()))
    return out


AT_LEAST = ("pivot_ties", "exp_small", "exp_large", "outlier_to_inlier", "stale_changed_flags",
            "not_positive", "rejected_trials")


def meets(cen, minimum):
    """Sets must hold the minimum's members, the AT_LEAST counts reach it,
    everything else equals it."""
    for k, v in minimum.items():
        if isinstance(v, (set, frozenset)):
            assert set(v) <= set(cen[k]), (k, sorted(v, key=str), sorted(cen[k], key=str))
        elif k in AT_LEAST:
            assert cen[k] >= v, (k, v, cen[k])
        else:
            assert cen[k] == v, (k, v, cen[k])


# ------------------------------------------------------------------------ cases
# name -> (builder, census minimum).  The minimum is what the case exists for;
# the rest of its census is printed by test_poseopt_edge_cases.py.
def _piv(*pairs):
    return set(pairs)


CASES = {
    # 1. pivots (the union must be ALL_PIVOTS: asserted by the CPU test)
    "pivots_640": (_wild(640), dict(n_edges=18, n_stereo=0, pivots=_piv((0, 0), (0, 3), (1, 2), (2, 5)))),
    "pivots_512": (_wild(512), dict(n_edges=40, n_mono=22, n_stereo=18, pivots=_piv((0, 0), (0, 1)))),
    "pivots_581": (_wild(581), dict(n_edges=10, n_mono=0, pivots=_piv((0, 0)), quadrants={0, 1, 2, 3})),
    "pivots_473": (_wild(473), dict(n_edges=5, n_mono=0, rounds=1)),
    "pivots_184": (_wild(184), dict(n_edges=6, n_mono=2, n_stereo=4, rounds=1, quat_start={1})),
    "pivots_741": (_wild(741), dict(n_edges=12, n_stereo=0, ended=["iterations"] * 4)),
    "pivots_tie_143": (_wild(143), dict(n_edges=11, n_stereo=0, pivot_ties=1, pivots=_piv((3, 3), (4, 4)))),
    "pivots_needed_17": (_wild(17), dict(n_edges=13, n_mono=6, n_stereo=7)),
    # 2. quaternion branches of the start pose, and of a step
    "quat_near_pi_x": (_near_pi(0), dict(quat_start={0}, n_edges=12)),
    "quat_near_pi_y": (_near_pi(1), dict(quat_start={1}, n_edges=12)),
    "quat_near_pi_z": (_near_pi(2), dict(quat_start={2}, n_edges=12)),
    "quat_pi_x": (_exactly_pi(0), dict(quat_start={0}, n_edges=12)),
    "quat_pi_y": (_exactly_pi(1), dict(quat_start={1}, n_edges=12)),
    "quat_pi_z": (_exactly_pi(2), dict(quat_start={2}, n_edges=12)),
    "quat_perm120": (_perm120, dict(quat_start={0}, n_edges=12)),
    "quat_qw_negative": (_qw_negative, dict(quat_start={0}, flips={"start"}, n_edges=12)),
    "quat_step_56": (_wild(56), dict(quat_step={"trace", 0, 1, 2}, flips={"exp", "mul"}, n_edges=9)),
    "quat_step_138": (_wild(138), dict(quat_step={"trace", 0, 1, 2}, quat_start={0}, n_edges=5)),
    # 3. exp: both sides of theta = 1e-5 in one problem, every quadrant
    "exp_quadrants_372": (_wild(372), dict(quadrants={0, 1, 2, 3}, exp_small=1, exp_large=1,
                                           n_edges=25)),
    # 4. termination
    "term_iterations": (_wild(4), dict(ended=["iterations"] * 4, lm_iterations=40, n_edges=14)),
    "term_qmax": (_wild(131), dict(ended=["nbad", "qmax", "qmax", "qmax"], n_edges=10)),
    "term_rho0": (_wild(96), dict(ended=["nbad", "rho0", "rho0", "nbad"], n_edges=10)),
    "term_nbad": (_wild(1), dict(ended=["nbad"] * 4, n_edges=26)),
    "all_outliers_after_round1": (_wild(0), dict(skipped_rounds=[1, 2, 3], ended=["nbad"], n_edges=19,
                                                 n_inliers=0, lm_iterations=8, rounds=4)),
    "outliers_return": (_wild(25), dict(skipped_rounds=[1], outlier_to_inlier=4, n_edges=40,
                                        n_inliers=4)),
    # (the only inputs found with stale_changed_flags > 0 are the non-finite
    # ones: the 40,000 finite problems of wild() searched gave none, the ten-times rejected
    # step of a qmax ending is too small to carry a float32 chi2 over its threshold)
    "stale_flags_inf_observation": (_extreme("inf_observation"),
                                    dict(stale_changed_flags=1, finite_pose=True, n_edges=20,
                                         lm_iterations=40, rejected_trials=40)),
    # 5. chi2 at the thresholds
    "sym_thresholds": (sym_thresholds, dict(n_edges=16, ended=["rho0"] * 4, lm_iterations=4,
                                            rejected_trials=4, n_inliers=8,
                                            active_after_round1=(0, 1, 4, 5, 8, 9, 10, 11))),
    "sym_huber_exact": (sym_huber_exact, dict(n_edges=12, ended=["rho0"] * 4, lm_iterations=4,
                                              n_inliers=6, active_after_round1=(0, 1, 8, 9, 10, 11))),
    # 6. the mono / stereo flag
    "flag_zeros": (flag_zeros, dict(n_edges=14, n_mono=7, n_stereo=7, finite_pose=True)),
    "flag_nan": (flag_nan, dict(n_edges=14, n_mono=3, n_stereo=11)),
    # 7. levels
    "levels_1": (_levels(1), dict(n_levels=1, n_edges=16)),
    "levels_3": (_levels(3), dict(n_levels=3, n_edges=16)),
    "levels_16": (_levels(16), dict(n_levels=16, n_edges=16)),
    "levels_1_bad_octave": (_levels(1, True), dict(n_levels=1, n_edges=-1)),
    "levels_3_bad_octave": (_levels(3, True), dict(n_levels=3, n_edges=-1)),
    "levels_16_bad_octave": (_levels(16, True), dict(n_levels=16, n_edges=-1)),
    # 8. non-finite and extreme inputs: every loop stays bounded
    "nan_point": (_extreme("nan_point"), dict(n_edges=20, lm_iterations=40)),
    "nan_pose": (_extreme("nan_pose"), dict(n_edges=20, lm_iterations=40, finite_pose=False)),
    "huge_tiny_points": (_extreme("huge_tiny_points"), dict(n_edges=20, finite_pose=True)),
    "huge_camera": (_extreme("huge_camera"), dict(n_edges=20, skipped_rounds=[1, 2, 3], n_inliers=0)),
    "tiny_depth": (_extreme("tiny_depth"), dict(n_edges=20, not_positive=0, lm_iterations=40)),
    "negative_level_weight": (negative_level_weight, dict(n_edges=30, not_positive=1,
                                                          finite_pose=True)),
    # 9. accumulation order: half tiles of 32, chunks of 64
    "acc_planted": (_acc(330, (0, 31, 32, 63, 64)),
                    dict(n_edges=65, active_after_round1=tuple(e for e in range(65)
                                                               if e not in (0, 31, 32, 63, 64)))),
    "acc_half_inactive": (_acc(331, range(32, 64)),
                          dict(n_edges=65, active_after_round1=tuple(range(32)) + (64,))),
    "acc_only_63": (_acc(339, range(63)), dict(n_edges=65, active_after_round1=(63, 64),
                                               skipped_rounds=[])),
    # 10. compaction
    "compact_chunks": (compact_chunks, dict(n_edges=65, n_keypoints=193)),
    "compact_ends": (compact_ends, dict(n_edges=12, n_keypoints=129)),
    # the smallest problem that is optimised at all (:384), and the largest that gets one round (:467)
    "three_edges": (lambda: synth(350, 3, "mixed", noise=0.5), dict(n_edges=3, rounds=1)),
    "nine_edges": (lambda: synth(351, 9, "mixed", noise=0.5), dict(n_edges=9, rounds=1)),
}
PIVOT_CASES = tuple(n for n in CASES if n.startswith("pivots_"))
