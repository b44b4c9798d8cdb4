"""Seeded PoseOptimization inputs shared by the CPU and GPU tests (test
infrastructure): a KITTI-like camera, points at 4-40 m, a true pose within a
few degrees and decimetres of the start pose, pixel noise 0 or 1, 20 % gross
outliers, random octaves with invSigma2 = 1 / 1.44^l."""
from __future__ import annotations

import functools

import numpy as np

import poseopt_ref as ref
from rgbd_cases import KEYPOINT_DTYPE

f32, f64 = np.float32, np.float64

CAM = tuple(f32(v) for v in (718.856, 718.856, 607.1928, 185.2157, 386.1448, 0.5371657))
N_LEVELS = 8
INV_LEVEL_SIGMA2 = np.array([f32(1.0) / f32(1.44 ** l) for l in range(N_LEVELS)], f32)
POSE_DTYPE = np.dtype([("rcw", "<f4", 9), ("tcw", "<f4", 3), ("ow", "<f4", 3)])
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", 3), ("normal", "<f4", 3), ("min_distance", "<f4"),
                            ("max_distance", "<f4"), ("bad", "u1"), ("seen", "u1"),
                            ("has_obs", "u1"), ("_pad", "u1")])
SENTINEL = 0xA5  # outlier slots of keypoints without an edge must keep it


def pose_record(est):
    R, t, ow = ref.pose_from_se3quat(est)
    p = np.zeros(1, POSE_DTYPE)
    p["rcw"], p["tcw"], p["ow"] = R, t, ow
    return p


def make_case(seed, n_kp, n_edges, kind="mixed", noise=1.0, outlier_frac=0.2, twist_scale=1.0,
              at_optimum=False):
    """One problem as the ABI takes it.  kind: mono / stereo / mixed.  The
    edges sit at random keypoint slots; points are a shuffled array with spare
    entries, so point_index is no identity."""
    rng = np.random.default_rng(seed)
    start = ref.se3_mul(ref.se3_exp(list(rng.normal(0, 1, 6) * [.05, .05, .05, .5, .5, .5])),
                        ([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]))
    pose = pose_record(start)
    start = ref.to_se3quat(pose["rcw"][0], pose["tcw"][0])  # as the solver sees the float pose
    uT = [0.0] * 6 if at_optimum else list(
        rng.normal(0, 1, 6) * [.02, .02, .02, .2, .2, .2] * twist_scale)
    truth = ref.se3_mul(ref.se3_exp(uT), start)
    fx, fy, cx, cy, bf = (float(c) for c in CAM[:5])
    n_pts = n_edges + 7
    # camera-frame points of the true pose, mapped back to the world
    # (inside the image, and far enough right that mvuRight stays positive)
    zc = rng.uniform(4, 40, n_pts)
    Pc = np.stack([rng.uniform(-0.6, 0.8, n_pts) * zc, rng.uniform(-0.24, 0.24, n_pts) * zc, zc], 1)
    qi = [-truth[0][0], -truth[0][1], -truth[0][2], truth[0][3]]
    d = Pc - np.array(truth[1])
    Xw = np.stack(ref.quat_rotate(qi, d[:, 0], d[:, 1], d[:, 2]), 1).astype(f32)
    keys = np.zeros(n_kp, KEYPOINT_DTYPE)
    keys["x"] = rng.uniform(0, 1241, n_kp)
    keys["y"] = rng.uniform(0, 376, n_kp)
    keys["size"], keys["class_id"] = 31.0, -1
    keys["octave"] = rng.integers(0, N_LEVELS, n_kp)
    u_right = np.full(n_kp, -1, f32)
    point_index = np.full(n_kp, -1, np.int32)
    slots = np.sort(rng.choice(n_kp, n_edges, replace=False))
    pts = rng.permutation(n_pts)[:n_edges]
    point_index[slots] = pts
    x, y, z = ref.quat_rotate(truth[0], *(Xw[pts].astype(f64).T))
    x, y, z = x + truth[1][0], y + truth[1][1], z + truth[1][2]
    u, v = x / z * fx + cx, y / z * fy + cy
    obs = np.stack([u, v, u - bf / z], 1)
    if noise:
        obs = obs + rng.normal(0, noise, obs.shape)
    bad = rng.random(n_edges) < outlier_frac
    obs[bad] += rng.choice([-1, 1], (int(bad.sum()), 3)) * rng.uniform(25, 60, (int(bad.sum()), 3))
    keys["x"][slots], keys["y"][slots] = obs[:, 0], obs[:, 1]
    st = {"mono": np.zeros(n_edges, bool), "stereo": np.ones(n_edges, bool),
          "mixed": rng.random(n_edges) < 0.5}[kind]
    # a stereo observation needs mvuRight >= 0
    u_right[slots] = np.where(st, np.maximum(obs[:, 2], 0.0), -1.0)
    if kind == "mono":
        u_right = None
    outlier = np.full(n_kp, SENTINEL, np.uint8)
    return dict(keys=keys, u_right=u_right, point_index=point_index, points=Xw, pose=pose,
                outlier=outlier, planted=slots[bad], slots=slots, truth=truth, kind=kind)


def run_ref(c, libm=False, **kw):
    k = c["keys"]
    return ref.pose_optimization(
        np.stack([k["x"], k["y"]], 1), k["octave"], c["u_right"], c["point_index"], c["points"],
        c.get("levels", INV_LEVEL_SIGMA2), c.get("cam", CAM), c["pose"]["rcw"][0], c["pose"]["tcw"][0],
        c["pose"]["ow"][0], c["outlier"], libm=libm, **kw)


# The shared list: (seed, keypoints, edges, kind, noise).  Sizes straddle the
# < 3 and < 10 rules, the kernel's 64-edge chunk and two of its multiples.
_SIZES = (3, 9, 10, 63, 64, 65, 129, 200, 400)
SHARED = [(100 + i, max(12, _SIZES[i % len(_SIZES)] * 5 // 4), _SIZES[i % len(_SIZES)],
           ("mixed", "mono", "stereo")[(i // 2) % 3], float(i % 2))
          for i in range(45)]


@functools.lru_cache(maxsize=None)
def shared_case(i):
    seed, n_kp, n_edges, kind, noise = SHARED[i]
    # every fifth problem starts further out, which is where trials get rejected
    c = make_case(seed, n_kp, n_edges, kind, noise, twist_scale=4.0 if i % 5 == 4 else 1.0)
    return c, run_ref(c)


def shared_results():
    """[(case, reference result)] for the whole list, computed once per process."""
    return [shared_case(i) for i in range(len(SHARED))]


def libm_study():
    """The libm pins measured: the shared list with math.sin / cos / pow against
    the pinned forms.  Returns the counts and the largest pose difference."""
    out = dict(problems=len(SHARED), differing_flags=0, differing_inlier_counts=0,
               differing_poses=0, differing_lm_iterations=0, max_abs_pose_difference=0.0)
    for c, r in shared_results():
        q = run_ref(c, libm=True)
        out["differing_flags"] += int((q["outlier"] != r["outlier"]).sum())
        out["differing_inlier_counts"] += int(q["n_inliers"] != r["n_inliers"])
        out["differing_lm_iterations"] += int(q["lm_iterations"] != r["lm_iterations"])
        a = np.concatenate([q[k] for k in ("rcw", "tcw", "ow")])
        b = np.concatenate([r[k] for k in ("rcw", "tcw", "ow")])
        out["differing_poses"] += int(a.tobytes() != b.tobytes())
        out["max_abs_pose_difference"] = max(out["max_abs_pose_difference"],
                                             float(np.abs(a.astype(f64) - b.astype(f64)).max()))
    return out
