"""Directed inputs of the Sim3Solver device batch (test infrastructure): problems
as tests/sim3_ref.py reads them, and their packing into the slot arrays of
orb_sim3_solver_setup_batch / _iterate_batch (include/orb_abi.h).

A Problem is two keyframes (KeyFrame: octaves, map point index per keypoint,
pose), the shared point arrays they index, vpMatched12 / index1 / index2 over
`stride` slots, and a draw stream whose first iterations follow a `plan`:
'g' draws three inliers, 'b' one inlier and two outliers, a tuple names the
three correspondences.  `tags` names the conditions a problem was built for
(the census of tests/test_sim3_ref.py checks what they claim).
"""
from __future__ import annotations

import math

import numpy as np

from sim3_ref import CORR_DTYPE, RESULT_DTYPE, STATE_DTYPE, KeyFrame, Sim3Solver

f32 = np.float32
RAND_MAX = 2147483647
N_LEVELS = 8
_sf = [f32(1)]
for _ in range(N_LEVELS - 1):
    _sf.append(_sf[-1] * f32(1.2))
LEVEL_SIGMA2 = np.array([s * s for s in _sf], f32)  # mvLevelSigma2 (src/ORBextractor.cc:437)
CAM1 = (500.0, 500.0, 320.0, 240.0)
CAM2 = (520.0, 510.0, 315.0, 245.0)
PROBABILITY, MIN_INLIERS, MAX_ITERATIONS = 0.99, 20, 300
STRIDE = 256
CHUNK = 8  # SIM3_CHUNK of the product build (the positions "first / last of a chunk" refer to it)


def rot(rx, ry, rz):
    """A rotation matrix from an angle-axis vector (float64; inputs only)."""
    th = math.sqrt(rx * rx + ry * ry + rz * rz)
    if th == 0:
        return np.eye(3)
    k = np.array([rx, ry, rz]) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def draws_for(N, triples, rand_max=RAND_MAX):
    """Raw rand() values that make RandomInt pick the given correspondences with
    the swap-with-back removal (src/Sim3Solver.cc:173-184)."""
    out = []
    for tri in triples:
        avail = list(range(N))
        for e in tri:
            pos = avail.index(e)
            d = len(avail)
            r = int((pos + 0.5) * (rand_max + 1.0) / d)
            assert int((float(r) / (float(rand_max) + 1.0)) * d) == pos
            out.append(r)
            avail[pos] = avail[-1]
            avail.pop()
    return out


class Problem:
    def __init__(self, name, kf1, kf2, points, match12, index1, index2, fix_scale, draws,
                 rand_max=RAND_MAX, tags=(), inlier=None, plan=()):
        self.name, self.kf1, self.kf2, self.points = name, kf1, kf2, points
        self.match12, self.index1, self.index2 = match12, index1, index2
        self.fix_scale, self.draws, self.rand_max = fix_scale, draws, rand_max
        self.tags, self.inlier, self.plan = set(tags), inlier, tuple(plan)

    def solver(self, libm=False, switch=None, max_iterations=MAX_ITERATIONS,
               min_inliers=MIN_INLIERS):
        return Sim3Solver(self.kf1, self.kf2, self.match12, self.fix_scale,
                          points_pos=self.points[0], points_bad=self.points[1],
                          index2=self.index2, index1=self.index1, level_sigma2=LEVEL_SIGMA2,
                          K1=CAM1, K2=CAM2, draws=self.draws, rand_max=self.rand_max,
                          probability=PROBABILITY, minInliers=min_inliers,
                          maxIterations=max_iterations, libm=libm, switch=switch)


def make_problem(name, seed, n_corr=40, n_outliers=10, scale=1.0, fix_scale=False,
                 rvec=(0.3, -0.2, 0.1), trans=(0.5, -0.3, 0.2), plan=(), skips=(), stride=STRIDE,
                 with_index1=False, rand_max=RAND_MAX, tags=(), special=None, n_extra=5,
                 max_iterations=MAX_ITERATIONS, exact=False):
    """n_corr kept correspondences (the first n_corr - n_outliers in compact
    order are inliers unless shuffled), one skipped slot per entry of `skips`,
    n_extra unmatched keypoints, interleaved in i1."""
    rng = np.random.default_rng(seed)
    n_skip = len(skips)
    n1 = n_corr + n_skip + n_extra
    assert n1 <= stride
    n2 = min(n1 + 3, stride)
    R12, t12 = rot(*rvec), np.array(trans, float)
    # camera coordinates: X1 = s R X2 + t for inliers
    if exact:  # small integers: every product and sum below is exact in float
        X2 = np.stack([rng.integers(-4, 5, n1), rng.integers(-4, 5, n1),
                       rng.integers(2, 9, n1)], 1).astype(float)
    else:
        X2 = np.stack([rng.uniform(-2, 2, n1), rng.uniform(-1.5, 1.5, n1),
                       rng.uniform(2, 8, n1)], 1)
    X1 = scale * X2 @ R12.T + t12
    # which i1 are kept correspondences, skipped ones, unmatched ones
    roles = np.array(["c"] * n_corr + ["s"] * n_skip + ["u"] * n_extra)
    rng.shuffle(roles)
    if n_skip or n_extra:  # the first slot is never a kept one: mvnIndices1[i] != i
        j = int(np.nonzero(roles != "c")[0][0])
        roles[0], roles[j] = roles[j], roles[0]
    corr_i1 = np.nonzero(roles == "c")[0]
    inlier = np.ones(n_corr, bool)
    if n_outliers:
        inlier[rng.choice(n_corr, n_outliers, replace=False)] = False
    for c, i1 in enumerate(corr_i1):
        if not inlier[c]:
            X1[i1] = [rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(2, 8)]
    if special:
        special(X1, X2, corr_i1, inlier)
    # keyframe poses and world positions: pos = Rcw^T (Xc - tcw)
    Rcw1, tcw1 = (np.eye(3), np.zeros(3)) if exact else (rot(0.1, 0.2, -0.1), np.array([0.3, 0.1, -0.2]))
    Rcw2, tcw2 = (np.eye(3), np.zeros(3)) if exact else (rot(-0.2, 0.1, 0.3), np.array([-0.4, 0.2, 0.1]))
    pos = np.zeros((n1 + n2, 3), f32)
    pos[:n1] = (X1 - tcw1) @ Rcw1
    perm2 = rng.permutation(n2)[:n1]  # keypoint of KF2 that observes the partner of i1
    pos[n1 + perm2] = (X2 - tcw2) @ Rcw2
    bad = np.zeros(n1 + n2, np.uint8)
    pi1 = np.full(stride, -1, np.int32)
    pi1[:n1] = np.arange(n1)
    pi2 = np.full(stride, -1, np.int32)
    pi2[:n2] = n1 + np.arange(n2)
    oct1 = np.zeros(stride, np.int32)
    oct2 = np.zeros(stride, np.int32)
    oct1[:n1] = rng.integers(0, N_LEVELS, n1)
    oct2[:n2] = rng.integers(0, N_LEVELS, n2)
    match12 = np.full(stride, -1, np.int32)
    index2 = np.full(stride, -1, np.int32)
    index1 = np.arange(stride, dtype=np.int32) if with_index1 or any(
        s in ("neg1", "big1") for s in skips) else None
    for i1 in range(n1):
        if roles[i1] != "u":
            match12[i1] = n1 + perm2[i1]
            index2[i1] = perm2[i1]
    for kind, i1 in zip(skips, np.nonzero(roles == "s")[0]):
        if kind == "null_match":
            match12[i1] = -7
        elif kind == "null_mp1":
            pi1[i1] = -1
        elif kind == "bad1":
            bad[i1] = 1
        elif kind == "bad2":
            bad[match12[i1]] = 1
        elif kind == "neg1":
            index1[i1] = -1
        elif kind == "neg2":
            index2[i1] = -3
        elif kind == "bad1_big2":  # skipped as bad before its index is looked at
            bad[i1] = 1
            index2[i1] = stride + 5
        else:
            raise ValueError(kind)
    kf1 = KeyFrame(oct1, pi1, Rcw1.astype(f32).reshape(9), tcw1.astype(f32), n1)
    kf2 = KeyFrame(oct2, pi2, Rcw2.astype(f32).reshape(9), tcw2.astype(f32), n2)
    # the draw stream: the plan first, then random raw values
    ins, outs = list(np.nonzero(inlier)[0]), list(np.nonzero(~inlier)[0])
    triples = []
    for step in plan:
        if step == "g":
            triples.append([int(v) for v in rng.choice(ins, 3, replace=False)])
        elif step == "b":
            triples.append([int(rng.choice(ins))] + [int(v) for v in rng.choice(outs, 2, replace=False)])
        else:
            triples.append(list(step))
    draws = draws_for(n_corr, triples, rand_max)
    n_draw = 3 * max_iterations
    draws = np.array(draws + list(rng.integers(0, rand_max + 1, n_draw - len(draws))), np.uint32)
    return Problem(name, kf1, kf2, (pos, bad), match12, index1, index2, fix_scale, draws, rand_max,
                   tags, inlier, plan)


# ------------------------------------------------------- the directed list
def _borderline(X1, X2, corr_i1, inlier):
    """The last kept correspondence reprojects 3.017 px off in image 1: between
    sqrt(9) and sqrt(9.21) (octave 0 there, a coarse octave in image 2)."""
    i1 = corr_i1[-1]
    X1[i1, 0] += 3.017 * X1[i1, 2] / CAM1[0]


def _identical(X1, X2, corr_i1, inlier):
    for c in (1, 2):
        X1[corr_i1[c]] = X1[corr_i1[0]]
        X2[corr_i1[c]] = X2[corr_i1[0]]


def _collinear(X1, X2, corr_i1, inlier):
    a, b = corr_i1[0], corr_i1[1]
    X2[corr_i1[2]] = 0.5 * (X2[a] + X2[b])
    X1[corr_i1[2]] = 0.5 * (X1[a] + X1[b])


def _z_zero(X1, X2, corr_i1, inlier):
    X1[corr_i1[3], 2] = 0.0


_directed = None


def directed():
    """The directed problems, built once (name -> Problem, insertion-ordered)."""
    global _directed
    if _directed is not None:
        return _directed
    P = []

    def add(*a, **k):
        P.append(make_problem(*a, **k))
        return P[-1]

    # correspondence counts; N <= 20 never succeeds, N == 20 runs one iteration
    for n in (19, 20, 21, 63, 64, 65, 80, 81, 200):
        add(f"n{n}", 100 + n, n_corr=n, n_outliers=0 if n <= 21 else n // 4, plan=("b", "g") if n > 21 else ("g",),
            tags={f"N={n}"})
    add("full_stride", 77, n_corr=STRIDE, n_outliers=60, n_extra=0, plan=("b", "b", "g"),
        tags={"N=stride"})
    # skip branches, each alone and all in one keyframe
    for kind in ("null_match", "null_mp1", "bad1", "bad2", "neg1", "neg2"):
        add(f"skip_{kind}", 200 + len(kind), skips=(kind,) * 3, plan=("g",), tags={f"skip:{kind}"})
    add("skip_all", 231, skips=("null_match", "null_mp1", "bad1", "bad2", "neg1", "neg2", "bad1_big2"),
        plan=("b", "g"), tags={"skip:all", "skip:order"})
    # where the success falls (chunks of CHUNK hypotheses, windows of 5)
    add("first_of_chunk", 301, plan=("b",) * CHUNK + ("g",), tags={"success:first_of_chunk"})
    add("last_of_chunk", 302, plan=("b",) * (CHUNK - 1) + ("g",), tags={"success:last_of_chunk"})
    add("last_of_window", 303, plan=("b",) * 4 + ("g",), tags={"success:last_of_window"})
    # the success on the last iteration SetRansacParameters allows
    P.append(_at_max_its())
    # ties: inliers == best on the second iteration
    P.append(_tie())
    # never succeeds: runs to exhaustion
    add("exhaust", 306, n_corr=30, n_outliers=12, plan=(), tags={"exhaust"})
    # count == min_inliers exactly: the strict > never fires
    # (n20 above); thresholds: one correspondence between the truncated and the double bound
    P.append(_borderline_problem())
    # degenerate samples
    add("identical", 401, special=_identical, plan=((0, 1, 2), "g"), tags={"degenerate:identical"})
    add("collinear", 402, special=_collinear, plan=((0, 1, 2), "g"), tags={"degenerate:collinear"})
    add("zero_rotation", 403, rvec=(0, 0, 0), trans=(0, 0, 0), exact=True, n_outliers=0,
        plan=((0, 1, 2), (3, 4, 5)), tags={"degenerate:zero_rotation"})
    add("z_zero", 404, special=_z_zero, plan=("g",), exact=True, tags={"degenerate:z_zero"})
    # the same four with the scale fixed
    add("identical_fix", 401, special=_identical, plan=((0, 1, 2), "g"), fix_scale=True,
        tags={"degenerate:identical", "fix_scale"})
    add("collinear_fix", 402, special=_collinear, plan=((0, 1, 2), "g"), fix_scale=True,
        tags={"degenerate:collinear", "fix_scale"})
    add("zero_rotation_fix", 403, rvec=(0, 0, 0), trans=(0, 0, 0), exact=True, n_outliers=0,
        plan=((0, 1, 2), (3, 4, 5)), fix_scale=True,
        tags={"degenerate:zero_rotation", "fix_scale"})
    add("z_zero_fix", 404, special=_z_zero, plan=("g",), exact=True, fix_scale=True,
        tags={"degenerate:z_zero", "fix_scale"})
    add("fix_scale", 405, fix_scale=True, scale=1.0, plan=("b", "g"), tags={"fix_scale"})
    add("fix_scale_wrong", 406, fix_scale=True, scale=1.3, n_outliers=0, plan=("g",),
        tags={"fix_scale:scaled_data"})
    add("free_scale", 407, fix_scale=False, scale=1.3, plan=("g",), tags={"free_scale"})
    P.append(_repeat_position())
    add("small_rand_max", 409, rand_max=32767, plan=("b", "g"), with_index1=True,
        tags={"rand_max:32767", "index1"})
    _directed = {p.name: p for p in P}
    assert len(_directed) == len(P)
    return _directed


def _at_max_its():
    # N = 22 with one outlier: epsilon = 20 / 22, four iterations allowed
    p = make_problem("at_max_its", 304, n_corr=22, n_outliers=1, plan=(), tags={"success:at_max_its"})
    n_its = p.solver().mRansacMaxIts
    out = int(np.nonzero(~p.inlier)[0][0])
    ins = [int(v) for v in np.nonzero(p.inlier)[0]]
    bad_t = [out, ins[0], ins[1]]
    triples = [bad_t] * (n_its - 1) + [ins[2:5]]
    d = draws_for(22, triples)
    p.draws[:len(d)] = d
    p.plan = ("b",) * (n_its - 1) + ("g",)
    return p


def _tie():
    # 18 inliers (never more than min_inliers): two different all-inlier samples
    # count the same 18, and the later one is taken on >=
    p = make_problem("tie", 305, n_outliers=22, plan=(), tags={"tie"})
    ins = [int(v) for v in np.nonzero(p.inlier)[0]]
    d = draws_for(40, [ins[0:3], ins[3:6]])
    p.draws[:len(d)] = d
    p.plan = ("g", "g")
    return p


def _borderline_problem():
    # 21 correspondences, all exact but the last: 20 inliers under the truncated
    # threshold (not > 20), 21 under the double one
    p = make_problem("borderline", 307, n_corr=21, n_outliers=0, special=_borderline, n_extra=5,
                     plan=((0, 1, 2),), tags={"threshold:truncated"})
    i1 = int(np.nonzero(p.match12[:p.kf1.nkeys] >= 0)[0][-1])
    p.kf1.octave[i1] = 0                 # sigma2 = 1: bound 9 (9.21 as a double)
    p.kf2.octave[p.index2[i1]] = 5       # a coarse level in image 2: far from its bound
    return p


def _repeat_position():
    # both first draws land on position 0: the second picks the element swapped in
    p = make_problem("repeat_position", 408, plan=(), tags={"draws:repeat_position"})
    N = 40
    r0 = int(0.5 * (RAND_MAX + 1.0) / N)
    r1 = int(0.5 * (RAND_MAX + 1.0) / (N - 1))
    r2 = int(5.5 * (RAND_MAX + 1.0) / (N - 2))
    p.draws[:3] = [r0, r1, r2]
    return p


def malformed():
    """Problems the device must flag (status -1), by kind."""
    out = {}
    for kind in ("index1_big", "index2_big", "octave1_neg", "octave2_big", "draw_big"):
        p = make_problem(f"malformed_{kind}", 500 + len(out), plan=("b", "b", "g"),
                         with_index1=True, rand_max=32767 if kind == "draw_big" else RAND_MAX)
        i1 = int(np.nonzero(p.match12[:p.kf1.nkeys] >= 0)[0][2])
        if kind == "index1_big":
            p.index1[i1] = p.kf1.nkeys
        elif kind == "index2_big":
            p.index2[i1] = p.kf2.nkeys
        elif kind == "octave1_neg":
            p.kf1.octave[p.index1[i1]] = -1
        elif kind == "octave2_big":
            p.kf2.octave[p.index2[i1]] = N_LEVELS
        else:
            p.draws[4] = 32768  # the second iteration's second draw
        p.tags = {f"malformed:{kind}"}
        out[kind] = p
    return out


def mixed(n, seed=9):
    """n problems of mixed sizes (for the batch tests): cheap ones, a success
    within the first few iterations."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        nc = int(rng.choice([19, 20, 25, 40, 64, 90, 130]))
        no = 0 if nc <= 20 else int(nc * rng.choice([0, 0.2, 0.3]))
        plan = ("g",) if no == 0 else tuple(rng.choice(["b", "g"], 2)) + ("g",)
        out.append(make_problem(f"mixed{i}", 1000 + i, n_corr=nc, n_outliers=no, plan=plan,
                                fix_scale=bool(i & 1), scale=1.0 if i & 1 else 1.1,
                                n_extra=int(rng.integers(0, 9))))
    return out


# ------------------------------------------------------------- the packing
class Batch:
    """The device arrays of a list of problems: keyframes and point arrays are
    slots / one shared array, deduplicated by object identity, so problems
    built on the same KeyFrame share its slot."""

    def __init__(self, problems, stride=STRIDE, max_iterations=MAX_ITERATIONS,
                 force_index1=False):
        self.problems, self.stride, self.max_iterations = problems, stride, max_iterations
        n = len(problems)
        slots, slot_of, pbase, npts = [], {}, {}, 0
        for p in problems:
            if id(p.points) not in pbase:
                pbase[id(p.points)] = npts
                npts += len(p.points[0])
        self.points = np.zeros(max(npts, 1), np.dtype(
            [("pos", "<f4", 3), ("normal", "<f4", 3), ("min_distance", "<f4"),
             ("max_distance", "<f4"), ("bad", "u1"), ("seen", "u1"), ("has_obs", "u1"),
             ("_pad", "u1")]))
        for p in problems:
            b = pbase[id(p.points)]
            self.points["pos"][b:b + len(p.points[0])] = p.points[0]
            self.points["bad"][b:b + len(p.points[0])] = p.points[1]
            for kf in (p.kf1, p.kf2):
                if id(kf) not in slot_of:
                    slot_of[id(kf)] = len(slots)
                    slots.append((kf, b))
        ns = len(slots)
        key_dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
        pose_dt = np.dtype([("rcw", "<f4", 9), ("tcw", "<f4", 3), ("ow", "<f4", 3)])
        self.keys = np.zeros((ns, stride), key_dt)
        self.nkeys = np.zeros(ns, np.int32)
        self.point_index = np.full((ns, stride), -1, np.int32)
        self.pose = np.zeros(ns, pose_dt)
        for s, (kf, b) in enumerate(slots):
            self.keys["octave"][s] = kf.octave
            self.nkeys[s] = kf.nkeys
            self.point_index[s] = np.where(kf.point_index >= 0, kf.point_index + b, kf.point_index)
            self.pose["rcw"][s], self.pose["tcw"][s] = kf.rcw, kf.tcw
        self.kf1_slot = np.array([slot_of[id(p.kf1)] for p in problems], np.int32)
        self.kf2_slot = np.array([slot_of[id(p.kf2)] for p in problems], np.int32)
        self.match12 = np.full((n, stride), -1, np.int32)
        self.index2 = np.full((n, stride), -1, np.int32)
        use_i1 = force_index1 or any(p.index1 is not None for p in problems)
        self.index1 = np.tile(np.arange(stride, dtype=np.int32), (n, 1)) if use_i1 else None
        self.draws = np.zeros((n, 3 * max_iterations), np.uint32)
        for i, p in enumerate(problems):
            b = pbase[id(p.points)]
            self.match12[i] = np.where(p.match12 >= 0, p.match12 + b, p.match12)
            self.index2[i] = p.index2
            if p.index1 is not None:
                self.index1[i] = p.index1
            self.draws[i] = p.draws[:3 * max_iterations]
        self.pbase = [pbase[id(p.points)] for p in problems]

    def solvers(self, **kw):
        return [p.solver(max_iterations=self.max_iterations, **kw) for p in self.problems]


__all__ = ["Batch", "Problem", "directed", "malformed", "mixed", "make_problem", "draws_for",
           "CORR_DTYPE", "STATE_DTYPE", "RESULT_DTYPE", "LEVEL_SIGMA2", "CAM1", "CAM2",
           "PROBABILITY", "MIN_INLIERS", "MAX_ITERATIONS", "STRIDE", "RAND_MAX", "N_LEVELS",
           "CHUNK"]
