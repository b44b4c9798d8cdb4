"""Optimizer::PoseOptimization restated in numpy float64 (test infrastructure):
the parity target of k_pose_optimization.

Restates src/Optimizer.cc:243-477 with the g2o parts it reaches.  Scalars are
Python floats (IEEE doubles), per-edge arithmetic is elementwise numpy (IEEE,
operation order as written), and every ordered sum is an explicit sequential
accumulate (np.add.accumulate / np.subtract.accumulate or a loop); np.sum,
np.dot, @ and einsum are never used.

Pins (the same list stands in include/orb_abi.h):
  * sin(theta), cos(theta) of SE3Quat::exp: pinned_sincos_d, the Cody-Waite
    reduction and fdlibm kernels of pinned_sincos returning
    the doubles before any narrowing.  libm=True uses math.sin / math.cos /
    math.pow instead.
  * pow(theta, 3) and pow(2 rho - 1, 3) are (x * x) * x.
  * sqrt and / are IEEE.
  * Eigen is pinned to its documented closed forms with sums left to right:
    Quaterniond(Matrix3d) (trace / largest-diagonal branches), normalize
    (coefficients x, y, z, w squared and summed left to right, each divided by
    the root), quaternion * quaternion, quaternion * vector as
    v + w (2 q x v) + q x (2 q x v), toRotationMatrix, 3x3 products row times
    column summed over k = 0, 1, 2, the fixed-size products of
    constructQuadraticForm left-associated ((A^T Omega) A, ((rho1 A^T) Omega) e)
    with the zero off-diagonal terms of the diagonal Omega dropped,
    information * error as invSigma2 * e_k, and LDLT<MatrixXd>: lower triangle,
    symmetric pivoting on the first largest remaining |diagonal|, unblocked,
    the column divided by a pivot whose magnitude is > 0, isPositive() = no
    negative pivot; solve = P, unit-lower forward substitution, division by
    pivots of magnitude > 1 / DBL_MAX (else 0), back substitution
    x_i -= (sum over ascending j > i of L_ji x_j), P^T.
Unpinned against Eigen / g2o binaries: neither is available to the project.
"""
from __future__ import annotations

import math
import sys

import numpy as np

f32, f64 = np.float32, np.float64
DBL_MAX = sys.float_info.max

# src/Optimizer.cc:283-284: floats; RobustKernel::setDelta (robust_kernel.cpp) squares the double
DELTA_MONO = float(f32(math.sqrt(5.991)))
DELTA_STEREO = float(f32(math.sqrt(7.815)))
CHI2_MONO = f32(5.991)    # :389
CHI2_STEREO = f32(7.815)  # :390


# ------------------------------------------------------------------ pins
def pinned_sincos_d(x: float, trace=None):
    """DESIGN.md App. A.6 without the final narrowing: (sin x, cos x) as doubles.
    trace["quadrants"] collects the quadrant q of every finite argument."""
    if not math.isfinite(x):
        return math.nan, math.nan
    invpio2 = 6.36619772367581382433e-01
    pio2_1, pio2_1t = 1.57079632673412561417e+00, 6.07710050650619224932e-11
    k = float(np.rint(x * invpio2))
    r = (x - k * pio2_1) - k * pio2_1t
    z = r * r
    S1, S2, S3 = -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04
    S4, S5, S6 = 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10
    C1, C2, C3 = 4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05
    C4, C5, C6 = -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11
    ps = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    sn = r + (z * r) * (S1 + z * ps)
    pc = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))
    hz = 0.5 * z
    w = 1.0 - hz
    cs = w + (((1.0 - w) - hz) + z * pc)
    q = int(min(max(k, -2147483648.0), 2147483647.0)) & 3  # the saturating (int)k of the device
    if trace is not None:
        trace["quadrants"].add(q)
    return ((sn, cs), (cs, -sn), (-sn, -cs), (-cs, sn))[q]


def _sqrt(x: float) -> float:
    return float(np.sqrt(f64(x)))  # IEEE, NaN for negatives instead of raising


def _div(a: float, b: float) -> float:
    with np.errstate(all="ignore"):
        return float(f64(a) / f64(b))


# ------------------------------------------------- Eigen closed forms (scalars)
def quat_from_matrix(m, branches=None):
    """Eigen Quaterniond(Matrix3d): returns (x, y, z, w).  branches collects the
    branch taken: "trace", or the index 0 / 1 / 2 of the largest diagonal entry."""
    t = (m[0][0] + m[1][1]) + m[2][2]
    q = [0.0, 0.0, 0.0, 0.0]
    if t > 0.0:
        if branches is not None:
            branches.add("trace")
        t = _sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = _div(0.5, t)
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        if branches is not None:
            branches.add(i)
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = _sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0)
        q[i] = 0.5 * t
        t = _div(0.5, t)
        q[3] = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    return q


def normalize_rotation(q, flips=None, where=None):
    """SE3Quat::normalizeRotation (se3quat.h:280-285).  flips collects `where`
    when the sign is flipped."""
    if q[3] < 0:
        q = [-q[0], -q[1], -q[2], -q[3]]
        if flips is not None:
            flips.add(where)
    n = _sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [_div(q[0], n), _div(q[1], n), _div(q[2], n), _div(q[3], n)]


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [((aw * bx + ax * bw) + ay * bz) - az * by,
            ((aw * by + ay * bw) + az * bx) - ax * bz,
            ((aw * bz + az * bw) + ax * by) - ay * bx,
            ((aw * bw - ax * bx) - ay * by) - az * bz]


def quat_rotate(q, x, y, z):
    """Eigen q * v; x, y, z scalars or arrays."""
    qx, qy, qz, qw = q
    ux = qy * z - qz * y
    uy = qz * x - qx * z
    uz = qx * y - qy * x
    ux = ux + ux
    uy = uy + uy
    uz = uz + uz
    return ((x + qw * ux) + (qy * uz - qz * uy),
            (y + qw * uy) + (qz * ux - qx * uz),
            (z + qw * uz) + (qx * uy - qy * ux))


def quat_to_matrix(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def _mat3mul(a, b):
    return [[(a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j] for j in range(3)]
            for i in range(3)]


def se3_exp(u, libm=False, trace=None):
    """SE3Quat::exp (se3quat.h:223-257): returns (q, t)."""
    o = [u[0], u[1], u[2]]
    up = [u[3], u[4], u[5]]
    theta = _sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2])
    Om = [[0.0, -o[2], o[1]], [o[2], 0.0, -o[0]], [-o[1], o[0], 0.0]]  # se3_ops.hpp:27-38
    Om2 = _mat3mul(Om, Om)
    eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    if theta < 0.00001:
        if trace is not None:
            trace["exp_small"] += 1
        R = [[(eye[i][j] + Om[i][j]) + Om2[i][j] for j in range(3)] for i in range(3)]
        V = R
    else:
        if trace is not None:
            trace["exp_large"] += 1
        if libm:
            s, c = math.sin(theta), math.cos(theta)
            th3 = math.pow(theta, 3)
        else:
            s, c = pinned_sincos_d(theta, trace if trace is not None and "quadrants" in trace else None)
            th3 = (theta * theta) * theta
        a = _div(s, theta)
        b = _div(1.0 - c, theta * theta)
        d = _div(theta - s, th3)
        R = [[(eye[i][j] + a * Om[i][j]) + b * Om2[i][j] for j in range(3)] for i in range(3)]
        V = [[(eye[i][j] + b * Om[i][j]) + d * Om2[i][j] for j in range(3)] for i in range(3)]
    t = [(V[i][0] * up[0] + V[i][1] * up[1]) + V[i][2] * up[2] for i in range(3)]
    full = trace is not None and "quat_step" in trace
    q = quat_from_matrix(R, trace["quat_step"] if full else None)
    return normalize_rotation(q, trace["flips"] if full else None, "exp"), t


def se3_mul(a, b, trace=None):
    """SE3Quat::operator* (se3quat.h:104-110)."""
    qa, ta = a
    qb, tb = b
    r = quat_rotate(qa, tb[0], tb[1], tb[2])
    return (normalize_rotation(quat_mul(qa, qb), None if trace is None else trace["flips"], "mul"),
            [ta[0] + r[0], ta[1] + r[1], ta[2] + r[2]])


def to_se3quat(rcw, tcw, trace=None):
    """Converter::toSE3Quat (src/Converter.cc:39-49), SE3Quat(R, t) (se3quat.h:58-60)."""
    R = [[float(f32(rcw[3 * i + j])) for j in range(3)] for i in range(3)]
    q = quat_from_matrix(R, None if trace is None else trace["quat_start"])
    return (normalize_rotation(q, None if trace is None else trace["flips"], "start"),
            [float(f32(v)) for v in tcw])


def pose_from_se3quat(est):
    """Converter::toCvMat (src/Converter.cc:51-73) and Frame::UpdatePoseMatrices
    (src/Frame.cc:294-300; float products summed left to right, as App. A pins mOw)."""
    q, t = est
    with np.errstate(all="ignore"):
        R = np.array(quat_to_matrix(q), f64).astype(f32)
        tc = np.array(t, f64).astype(f32)
        ow = np.array([-(f32(f32(R[0, i] * tc[0]) + f32(R[1, i] * tc[1])) + f32(R[2, i] * tc[2]))
                       for i in range(3)], f32)
    return R.reshape(9), tc, ow


# ------------------------------------------------------------ LDLT<MatrixXd>
def ldlt_solve(H, b, x_prev, pivots=None, trace=None, variants=()):
    """LinearSolverDense::solve (linear_solver_dense.h:104-112) on the lower
    triangle of the n x n H, n = len(b) (6 here, 7 for tests/sim3opt_ref.py):
    returns (ok, x); x = x_prev when !isPositive().
    trace["pivots"] collects the (k, idx) pairs, trace["pivot_sequences"] (when
    the trace has that key) the whole transposition lists, trace["pivot_ties"]
    counts the steps whose largest |diagonal| is held by more than one
    remaining entry.
    variants (NOT the reference): "tie_last" takes the last of equal
    magnitudes, "no_pivot" never swaps, "half_swap_<k><idx>" leaves the two
    diagonal entries where they were in the swap of that one (k, idx)."""
    n = len(b)
    m = [list(r) for r in H]
    tr = [0] * n
    positive = True
    for k in range(n):
        idx, best = k, abs(m[k][k])
        for i in range(k + 1, n):
            if abs(m[i][i]) > best or ("tie_last" in variants and abs(m[i][i]) == best):
                idx, best = i, abs(m[i][i])
        if "no_pivot" in variants:
            idx = k
        tr[k] = idx
        if trace is not None:
            trace["pivots"].add((k, idx))
            if [abs(m[i][i]) for i in range(k, n)].count(best) > 1:
                trace["pivot_ties"] += 1
        if idx != k:
            for j in range(k):
                m[k][j], m[idx][j] = m[idx][j], m[k][j]
            for r in range(idx + 1, n):
                m[r][k], m[r][idx] = m[r][idx], m[r][k]
            if "half_swap_%d%d" % (k, idx) not in variants:
                m[k][k], m[idx][idx] = m[idx][idx], m[k][k]
            for i in range(k + 1, idx):
                m[i][k], m[idx][i] = m[idx][i], m[i][k]
        if k > 0:
            temp = [m[j][j] * m[k][j] for j in range(k)]
            for i in range(k, n):
                s = m[i][0] * temp[0]
                for j in range(1, k):
                    s = s + m[i][j] * temp[j]
                m[i][k] = m[i][k] - s
        akk = m[k][k]
        if abs(akk) > 0.0:
            for i in range(k + 1, n):
                m[i][k] = _div(m[i][k], akk)
        if akk < 0.0:
            positive = False
    if pivots is not None:
        pivots[:] = tr
    if trace is not None and "pivot_sequences" in trace:
        trace["pivot_sequences"].add(tuple(tr))
    if not positive:
        return False, list(x_prev)
    y = list(b)
    for k in range(n):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    for i in range(n):
        for r in range(i + 1, n):
            y[r] = y[r] - y[i] * m[r][i]
    tol = 1.0 / DBL_MAX
    for i in range(n):
        y[i] = _div(y[i], m[i][i]) if abs(m[i][i]) > tol else 0.0
    for i in range(n - 2, -1, -1):
        s = m[i + 1][i] * y[i + 1]
        for j in range(i + 2, n):
            s = s + m[j][i] * y[j]
        y[i] = y[i] - s
    for k in range(n - 1, -1, -1):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    return True, y


# ------------------------------------------------------------ per-edge passes
def huber(e, delta, strict=False):
    """RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91), elementwise:
    returns (rho0, rho1, inlier branch taken).  strict=True is NOT the
    reference: it compares with < in place of <=."""
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        inl = (e < dsqr) if strict else (e <= dsqr)
        sq = np.sqrt(e)
        return np.where(inl, e, (2 * sq) * delta - dsqr), np.where(inl, 1.0, delta / sq), inl


class _Edges:
    def __init__(self, X, obs, inv, stereo, cam):
        self.X, self.obs, self.inv, self.st = X, obs, inv, stereo
        self.fx, self.fy, self.cx, self.cy, self.bf = (float(f32(c)) for c in cam[:5])
        self.delta = np.where(stereo, DELTA_STEREO, DELTA_MONO)

    def map(self, est):
        """SE3Quat::map (se3quat.h:217-220)."""
        q, t = est
        rx, ry, rz = quat_rotate(q, self.X[:, 0], self.X[:, 1], self.X[:, 2])
        return rx + t[0], ry + t[1], rz + t[2]

    def error(self, est):
        """computeError (types_six_dof_expmap.h:153-157, :184-188) with both
        cam_project forms (.cpp:290-306): returns (e0, e1, e2, chi2)."""
        with np.errstate(all="ignore"):
            x, y, z = self.map(est)
            um = (x / z) * self.fx + self.cx      # project2d, se3_ops.hpp
            vm = (y / z) * self.fy + self.cy
            iz = (1.0 / z).astype(f32).astype(f64)  # const float invz = 1.0f / z (.cpp:300)
            us = (x * iz) * self.fx + self.cx
            vs = (y * iz) * self.fy + self.cy
            rs = us - self.bf * iz
            e0 = self.obs[:, 0] - np.where(self.st, us, um)
            e1 = self.obs[:, 1] - np.where(self.st, vs, vm)
            e2 = np.where(self.st, self.obs[:, 2] - rs, 0.0)
            s = self.inv
            c2 = e0 * (s * e0) + e1 * (s * e1)   # BaseEdge::chi2, base_edge.h
            chi2 = np.where(self.st, c2 + e2 * (s * e2), c2)
        return e0, e1, e2, chi2

    def jacobian(self, est):
        """linearizeOplus (.cpp:266-288, :335-364): A[k][c], row 2 zero for mono."""
        with np.errstate(all="ignore"):
            x, y, z = self.map(est)
            invz = 1.0 / z
            invz_2 = invz * invz
            fx, fy, bf = self.fx, self.fy, self.bf
            zero = np.zeros(len(x))
            A0 = [((x * y) * invz_2) * fx, (-(1 + ((x * x) * invz_2))) * fx, (y * invz) * fx,
                  (-invz) * fx, zero, (x * invz_2) * fx]
            A1 = [(1 + (y * y) * invz_2) * fy, (((-x) * y) * invz_2) * fy, ((-x) * invz) * fy,
                  zero, (-invz) * fy, (y * invz_2) * fy]
            A2 = [A0[0] - (bf * y) * invz_2, A0[1] + (bf * x) * invz_2, A0[2], A0[3], zero,
                  A0[5] - bf * invz_2]
        return [A0, A1, A2]


def _seq_sum(v):
    return float(np.add.accumulate(v)[-1]) if len(v) else 0.0


def pose_optimization(keys_xy, octave, u_right, point_index, points, inv_level_sigma2, cam,
                      rcw, tcw, ow, outlier=None, libm=False, classify_from_final=False,
                      variants=()):
    """Optimizer::PoseOptimization (src/Optimizer.cc:243-477).  Returns a dict:
    rcw, tcw, ow (float32), outlier (uint8, slots without an edge as given),
    n_inliers, n_edges, lm_iterations, rejected_trials and `trace`.
    classify_from_final=True is NOT the reference: it classifies every edge at
    the final estimate, the behaviour the stale-error rule differs from (the
    tests use it to show that the rule matters).  variants names further wrong
    neighbours, none of them the reference either: "classify_ge" (chi2 >= the
    threshold is an outlier), "huber_lt", "stereo_le" (mvuRight <= 0 is
    monocular), "tie_last", "no_pivot" and "half_swap_<k><idx>" (ldlt_solve), "three_edges" (returns
    below four edges), "ten_edges" (one round up to ten edges) and
    "classify_from_final".
    trace also holds: pivots, the set of (k, idx) over all solves,
    pivot_sequences and pivot_ties; quat_start / quat_step, the Quaterniond(Matrix3d) branches of
    toSE3Quat and of exp; flips, where normalizeRotation changed the sign
    ("start", "exp", "mul"); quadrants of pinned_sincos_d; skipped_rounds, the
    rounds whose optimize() had no active edge; max_theta, the largest step angle;
    round_outliers, the edge positions flagged after each round; chi2_first, the
    float32 chi2 values the first round classified."""
    variants = tuple(variants)
    classify_from_final = classify_from_final or "classify_from_final" in variants
    keys_xy = np.asarray(keys_xy, f32).reshape(-1, 2)
    n = len(keys_xy)
    octave = np.asarray(octave, np.int64)
    pidx = np.asarray(point_index, np.int64)
    ur = np.full(n, -1, f32) if u_right is None else np.asarray(u_right, f32)
    out_flags = np.zeros(n, np.uint8) if outlier is None else np.array(outlier, np.uint8)
    pose_in = (np.array(rcw, f32).reshape(9), np.array(tcw, f32).reshape(3),
               np.array(ow, f32).reshape(3))
    trace = dict(rounds=0, lm_iterations=0, rejected_trials=0, term_qmax=0, term_rho0=0, term_nbad=0,
                 term_iterations=0, stale_rounds=0, stale_chi_differs=0, stale_changed_flags=0, outlier_to_inlier=0,
                 exp_small=0, exp_large=0, huber_inlier=False, huber_outlier=False,
                 not_positive=0, n_mono=0, n_stereo=0, ended=[],  # ended: the rule that ended each optimize()
                 pivots=set(), pivot_sequences=set(), pivot_ties=0, quat_start=set(), quat_step=set(), flips=set(),
                 quadrants=set(), skipped_rounds=[], max_theta=0.0, round_outliers=[], chi2_first=None)
    res = dict(rcw=pose_in[0], tcw=pose_in[1], ow=pose_in[2], outlier=out_flags, n_inliers=0,
               n_edges=0, lm_iterations=0, rejected_trials=0, trace=trace)
    ei = np.nonzero(pidx >= 0)[0]  # :290-294, ascending keypoint order
    E = len(ei)
    levels = np.asarray(inv_level_sigma2, f32)
    if E and ((octave[ei] < 0) | (octave[ei] >= len(levels))).any():
        res["n_edges"] = -1  # the ABI's answer to an octave outside [0, n_levels)
        return res
    res["n_edges"] = E
    out_flags[ei] = 0  # :301, :342
    if E < (4 if "three_edges" in variants else 3):  # :384-385
        return res
    with np.errstate(invalid="ignore"):
        stereo = ~((ur[ei] <= 0) if "stereo_le" in variants else (ur[ei] < 0))  # :298
    trace["n_mono"], trace["n_stereo"] = int((~stereo).sum()), int(stereo.sum())
    X = np.asarray(points, f32).reshape(-1, 3)[pidx[ei]].astype(f64)
    obs = np.stack([keys_xy[ei, 0], keys_xy[ei, 1], ur[ei]], 1).astype(f64)
    inv = levels[octave[ei]].astype(f64)
    ed = _Edges(X, obs, inv, stereo, cam)
    thr = np.where(stereo, CHI2_STEREO, CHI2_MONO).astype(f32)
    flags = np.zeros(E, bool)  # mvbOutlier of the edges == their level
    robust = True
    est0 = to_se3quat(rcw, tcw, trace)
    est = est0
    x = [0.0] * 6  # BlockSolver::_x: kept when the solver reports !ok
    n_bad_edges = 0

    def robust_chi2(chi2, act):
        """SparseOptimizer::activeRobustChi2 (sparse_optimizer.cpp:100-114)."""
        if robust:
            r0, r1, inl = huber(chi2, ed.delta, "huber_lt" in variants)
            if act.any():
                trace["huber_inlier"] |= bool(inl[act].any())
                trace["huber_outlier"] |= bool((~inl[act]).any())
        else:
            r0, r1 = chi2, np.ones(E)
        return _seq_sum(r0[act]), r1

    for it in range(4):
        trace["rounds"] += 1
        est = est0  # :397
        act = ~flags  # initializeOptimization(0): the edges at level 0, in insertion order
        last_est = est  # the estimate the active edges' _error was last computed at
        if act.any():  # (optimize() returns at once without active vertices, sparse_optimizer.cpp:356)
            lam, ni, nbad = 0.0, 2.0, 0
            ended = "iterations"
            for i in range(10):  # optimize(10), sparse_optimizer.cpp:376
                trace["lm_iterations"] += 1
                # ---- OptimizationAlgorithmLevenberg::solve (:61-164)
                e0, e1, e2, chi2 = ed.error(est)
                cur, r1 = robust_chi2(chi2, act)
                ini = cur
                A = ed.jacobian(est)  # buildSystem (block_solver.hpp:502-560)
                s = ed.inv
                w = (s * r1) if robust else s  # robustInformation: rho[1] * information
                es = [e0, e1, e2]
                H = [[0.0] * 6 for _ in range(6)]
                b = [0.0] * 6
                with np.errstate(all="ignore"):
                    for r in range(6):
                        for c in range(r + 1):  # the lower triangle LDLT reads
                            t2 = ((A[0][r] * w) * A[0][c] + (A[1][r] * w) * A[1][c])
                            t3 = t2 + (A[2][r] * w) * A[2][c]
                            H[r][c] = _seq_sum(np.where(stereo, t3, t2)[act])
                        if robust:
                            p = [((r1 * A[k][r]) * s) * es[k] for k in range(3)]
                        else:
                            p = [(A[k][r] * s) * es[k] for k in range(3)]
                        t2 = p[0] + p[1]
                        term = np.where(stereo, t2 + p[2], t2)[act]
                        b[r] = float(np.subtract.accumulate(np.concatenate([[0.0], term]))[-1])
                if i == 0:  # computeLambdaInit (:166-180)
                    md = 0.0
                    for j in range(6):
                        a = abs(H[j][j])
                        md = md if a < md else a  # std::max(fabs(h), maxDiagonal)
                    lam, ni, nbad = 1e-5 * md, 2.0, 0
                rho, qmax = 0.0, 0
                while True:
                    backup = est
                    Hl = [list(r) for r in H]
                    for j in range(6):
                        Hl[j][j] = H[j][j] + lam  # setLambda (block_solver.hpp:564-589)
                    ok2, x = ldlt_solve(Hl, b, x, None, trace, variants)
                    if not ok2:
                        trace["not_positive"] += 1
                    theta = _sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
                    if theta > trace["max_theta"]:
                        trace["max_theta"] = theta
                    est = se3_mul(se3_exp(x, libm, trace), est, trace)  # oplusImpl (.h:73-76)
                    _, _, _, chi2t = ed.error(est)
                    last_est = est
                    tmp, _ = robust_chi2(chi2t, act)
                    if not ok2:
                        tmp = DBL_MAX
                    scale = 0.0
                    for j in range(6):  # computeScale (:182-189)
                        scale = scale + x[j] * (lam * x[j] + b[j])
                    scale = scale + 1e-3
                    rho = _div(cur - tmp, scale)
                    if rho > 0 and math.isfinite(tmp):
                        y = 2 * rho - 1
                        alpha = 1.0 - (math.pow(y, 3) if libm else (y * y) * y)
                        alpha = 2.0 / 3.0 if 2.0 / 3.0 < alpha else alpha  # std::min(alpha, upper)
                        sf = alpha if 1.0 / 3.0 < alpha else 1.0 / 3.0     # std::max(lower, alpha)
                        lam = lam * sf
                        ni = 2.0
                        cur = tmp
                    else:
                        lam = lam * ni
                        ni = ni * 2
                        est = backup  # pop(): the vertex, not the edges' _error
                        trace["rejected_trials"] += 1
                    qmax += 1
                    if not (rho < 0 and qmax < 10):
                        break
                if qmax == 10 or rho == 0:
                    ended = "qmax" if qmax == 10 else "rho0"
                    break
                if (ini - cur) * 1e3 < ini:
                    nbad += 1
                else:
                    nbad = 0
                if nbad >= 3:
                    ended = "nbad"
                    break
            trace["term_" + ended] += 1
            trace["ended"].append(ended)
        else:
            trace["skipped_rounds"].append(it)
        # ---- classification (:402-465): active edges from their last _error,
        # level-1 edges recomputed at the final estimate (:411-414)
        _, _, _, chi_last = ed.error(last_est)
        _, _, _, chi_fin = ed.error(est)
        with np.errstate(all="ignore"):
            chi = (chi_fin if classify_from_final else np.where(act, chi_last, chi_fin)).astype(f32)
            new = (chi >= thr) if "classify_ge" in variants else (chi > thr)
            if it == 0:
                trace["chi2_first"] = chi.copy()
            if last_est is not est and act.any():
                trace["stale_rounds"] += 1
                trace["stale_chi_differs"] += int(
                    (chi_fin.astype(f32).view(np.uint32) != chi.view(np.uint32))[act].sum())
                trace["stale_changed_flags"] += int(((chi_fin.astype(f32) > thr) != new)[act].sum())
        trace["outlier_to_inlier"] += int((flags & ~new).sum())
        flags = new
        trace["round_outliers"].append(tuple(int(e) for e in np.nonzero(new)[0]))
        n_bad_edges = int(new.sum())
        if it == 2:
            robust = False  # :433-435
        if E < (11 if "ten_edges" in variants else 10):  # :467
            break
    out_flags[ei] = flags
    R, tc, o = pose_from_se3quat(est)
    res.update(rcw=R, tcw=tc, ow=o, outlier=out_flags, n_inliers=E - n_bad_edges,
               lm_iterations=trace["lm_iterations"], rejected_trials=trace["rejected_trials"])
    return res
