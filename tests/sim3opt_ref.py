"""Optimizer::OptimizeSim3 restated in numpy float64 (test infrastructure): the
parity target of k_optimize_sim3.

Restates src/Optimizer.cc:1130-1326 with the g2o parts it reaches
(types/sim3.h, types_seven_dof_expmap.h, core/base_binary_edge.hpp:50-200,
solvers/linear_solver_dense.h and the OptimizationAlgorithmLevenberg /
SparseOptimizer::optimize rules tests/poseopt_ref.py already restates).
Scalars are Python floats (IEEE doubles), per-edge arithmetic is elementwise
numpy (IEEE, operation order as written), and every ordered sum is an explicit
sequential accumulate (np.add.accumulate from +0.0); np.sum, np.dot, @ and
einsum are never used.

Pins (the same list stands in include/orb_abi.h and DESIGN.md 4.12).  The Eigen
closed forms (Quaterniond(Matrix3d), quaternion * quaternion, quaternion *
vector, toRotationMatrix, 3x3 products), the LDLT<MatrixXd> rules (here n = 7)
and the Levenberg-Marquardt rules are those of tests/poseopt_ref.py.
  O1  P3D1c, P3D2c = Rcw * X + tcw in float (the Sim3 solver's pin P1), then
      widened.
  O2  Jacobians are numeric (base_binary_edge.hpp:131-200): column d =
      (1.0 / (2 * 1e-9)) * (e(+1e-9 e_d) - e(-1e-9 e_d)), each through
      oplusImpl: Sim3(update) * estimate.  _error is restored afterwards.
  O3  constructQuadraticForm of a binary edge whose `to` vertex alone is free
      (:91-113): omega_r = -(Omega e), omega_r *= rho[1], b += B^T omega_r
      ((B_0q r_0) + (B_1q r_1)), A += (B^T (rho[1] Omega)) B ((B_0q w) B_0p +
      (B_1q w) B_1p, w = rho[1] * invSigma2), the zero off-diagonal terms of
      the diagonal Omega dropped; the lower triangle is accumulated.
  O4  The active edges add in insertion order e12(i), e21(i), e12(i'),
      e21(i'), ... over ascending i; a removed pair adds +0.0.
  O5  An edge is classified from the error of the last trial, rejected or
      not; chi2() > th2 compares the double chi2 with the float th2 widened;
      deltaHuber is the float sqrt(th2) widened; Huber's inlier test is <=.
  O6  oplusImpl with fix_scale writes update[6] = 0 into the caller's array:
      column 6 is the difference of two equal evaluations, and the solver's
      x[6] is zeroed before computeScale reads it.
  O7  Sim3(Vector7d) (sim3.h:70-142): branches |sigma| < 1e-5 x theta < 1e-5,
      R = (I + Omega) + Omega^2 or (I + (sin / theta) Omega) + ((1 - cos) /
      (theta theta)) Omega^2, A, B, C as written, W = ((A Omega) + (B Omega^2))
      + (C I), t = W upsilon; Quaterniond(R) is never normalised, nor are
      operator*, map or inverse(); inverse() = (r.conjugate(),
      r.conjugate() * ((-1. / s) * t), 1. / s); project is two divisions by z.
  O8  The second optimize starts at iteration 0: lambda from the 7 diagonals,
      ni = 2; the solver's x is kept across both.
  O9  exp = pinned_exp (fdlibm e_exp.c from IEEE operations alone); sin and
      cos = pinned_sincos_d; sqrt and / are IEEE.
libm=True uses math.exp / math.sin / math.cos / math.pow instead.
Unpinned against Eigen / g2o binaries: neither is available to the project.
"""
from __future__ import annotations

import math

import numpy as np

from poseopt_ref import (DBL_MAX, _div, _mat3mul, _sqrt, huber, ldlt_solve, pinned_sincos_d,
                         quat_from_matrix, quat_mul, quat_rotate, quat_to_matrix)
from sim3_ref import _bits, _from_bits

f32, f64 = np.float32, np.float64

VARIANTS = ("unary_assoc", "forward_diff", "normalize_quat", "chi2_float", "huber_lt",
            "classify_from_final", "e21_first", "tie_last")

OPT_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_corr", "<i4"), ("n_bad", "<i4"),
                             ("n_inliers", "<i4"), ("q", "<f8", 4), ("t", "<f8", 3), ("s", "<f8"),
                             ("R", "<f4", 9), ("t_f", "<f4", 3), ("s_f", "<f4"), ("_pad", "<i4")])
assert OPT_RESULT_DTYPE.itemsize == 136


# ------------------------------------------------------------------ pins
def pinned_exp(x: float) -> float:
    """fdlibm e_exp.c from IEEE operations alone (orb_device.h pinned_exp), the
    same operation sequence."""
    o_threshold, u_threshold = 7.09782712893383973096e+02, -7.45133219101941108420e+02
    ln2HI, ln2LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    invln2, twom1000 = 1.44269504088896338700e+00, 9.33263618503218878990e-302
    P1, P2, P3 = 1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05
    P4, P5 = -1.65339022054652515390e-06, 4.13813679705723846039e-08
    bits = _bits(x)
    hx, lx = bits >> 32, bits & 0xFFFFFFFF
    xsb = (hx >> 31) & 1
    hx &= 0x7FFFFFFF
    if hx >= 0x40862E42:  # |x| >= 709.78
        if hx >= 0x7FF00000:
            if ((hx & 0xFFFFF) | lx) != 0:
                return x + x  # NaN
            return x if xsb == 0 else 0.0  # exp(+-inf) = inf, 0
        if x > o_threshold:
            return math.inf  # huge * huge
        if x < u_threshold:
            return 0.0  # twom1000 * twom1000
    hi = lo = 0.0
    k = 0
    if hx > 0x3FD62E42:  # |x| > 0.5 ln2
        if hx < 0x3FF0A2B2:  # |x| < 1.5 ln2
            hi = x - (-ln2HI) if xsb else x - ln2HI
            lo = -ln2LO if xsb else ln2LO
            k = 1 - xsb - xsb
        else:
            k = int(invln2 * x + (-0.5 if xsb else 0.5))  # truncation toward zero
            t = float(k)
            hi = x - t * ln2HI
            lo = t * ln2LO
        x = hi - lo
    elif hx < 0x3E300000:  # |x| < 2^-28
        return 1.0 + x
    t = x * x
    c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))))
    if k == 0:
        return 1.0 - ((x * c) / (c - 2.0) - x)
    y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi)
    if k >= -1021:
        return _from_bits(_bits(y) + (k << 52))
    return _from_bits(_bits(y) + ((k + 1000) << 52)) * twom1000


def _libm_exp(x: float) -> float:
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


# ------------------------------------------------------------- g2o::Sim3
# a Sim3 is (q = [x, y, z, w], t = [x, y, z], s)
def _normalize(q):
    n = _sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [_div(q[0], n), _div(q[1], n), _div(q[2], n), _div(q[3], n)]


def sim3_exp(u, libm=False, trace=None, where="step", variants=()):
    """Sim3(const Vector7d&) (sim3.h:70-142)."""
    o0, o1, o2 = u[0], u[1], u[2]
    up = [u[3], u[4], u[5]]
    sigma = u[6]
    theta = _sqrt((o0 * o0 + o1 * o1) + o2 * o2)
    Om = [[0.0, -o2, o1], [o2, 0.0, -o0], [-o1, o0, 0.0]]
    Om2 = _mat3mul(Om, Om)
    eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    s = _libm_exp(sigma) if libm else pinned_exp(sigma)
    eps = 0.00001
    small_s, small_t = abs(sigma) < eps, theta < eps
    if trace is not None:
        trace["exp_args"].add(_bits(sigma))
        trace["exp_" + where].add((small_s, small_t))
    sn = cs = 0.0
    if small_t:
        R = [[(eye[i][j] + Om[i][j]) + Om2[i][j] for j in range(3)] for i in range(3)]
    else:
        if libm:
            sn, cs = (math.sin(theta), math.cos(theta)) if math.isfinite(theta) else (math.nan, math.nan)
        else:
            sn, cs = pinned_sincos_d(theta)
        a, b = _div(sn, theta), _div(1 - cs, theta * theta)
        R = [[(eye[i][j] + a * Om[i][j]) + b * Om2[i][j] for j in range(3)] for i in range(3)]
    if small_s:
        C = 1.0
        if small_t:
            A, B = 1. / 2., 1. / 6.
        else:
            theta2 = theta * theta
            A = _div(1 - cs, theta2)
            B = _div(theta - sn, theta2 * theta)
    else:
        C = _div(s - 1, sigma)
        if small_t:
            sigma2 = sigma * sigma
            A = _div((sigma - 1) * s + 1, sigma2)
            B = _div((0.5 * sigma2 - sigma + 1) * s, sigma2 * sigma)
        else:
            a, b = s * sn, s * cs
            theta2, sigma2 = theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = _div(a * sigma + (1 - b) * theta, theta * c)
            B = _div((C - _div((b - 1) * sigma + a * theta, c)) * 1., theta2)
    q = quat_from_matrix(R, None if trace is None else trace["quat_" + where])
    if "normalize_quat" in variants:
        q = _normalize(q)
    W = [[(A * Om[i][j] + B * Om2[i][j]) + C * eye[i][j] for j in range(3)] for i in range(3)]
    t = [(W[i][0] * up[0] + W[i][1] * up[1]) + W[i][2] * up[2] for i in range(3)]
    return q, t, s


def sim3_mul(a, b, variants=()):
    """Sim3::operator* (sim3.h:266-272)."""
    qa, ta, sa = a
    qb, tb, sb = b
    q = quat_mul(qa, qb)
    if "normalize_quat" in variants:
        q = _normalize(q)
    r = quat_rotate(qa, tb[0], tb[1], tb[2])
    return q, [sa * r[0] + ta[0], sa * r[1] + ta[1], sa * r[2] + ta[2]], sa * sb


def sim3_inverse(a):
    """Sim3::inverse (sim3.h:233-236)."""
    q, t, s = a
    qc = [-q[0], -q[1], -q[2], q[3]]
    c = _div(-1., s)
    r = quat_rotate(qc, c * t[0], c * t[1], c * t[2])
    return qc, [r[0], r[1], r[2]], _div(1., s)


def sim3_from_start(R, t, s, trace=None, variants=()):
    """g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s)."""
    m = [[float(f32(R[3 * i + j])) for j in range(3)] for i in range(3)]
    q = quat_from_matrix(m, None if trace is None else trace["quat_start"])
    if "normalize_quat" in variants:
        q = _normalize(q)
    return q, [float(f32(v)) for v in t], float(f32(s))


def edge_error(est, X, obs, K):
    """computeError (types_seven_dof_expmap.h:138-145, :160-167) at the estimate
    (or inverse) est: obs - cam_map(project(est.map(X))), elementwise."""
    q, t, s = est
    with np.errstate(all="ignore"):
        rx, ry, rz = quat_rotate(q, X[:, 0], X[:, 1], X[:, 2])
        x = s * rx + t[0]
        y = s * ry + t[1]
        z = s * rz + t[2]
        e0 = obs[:, 0] - ((x / z) * K[0] + K[2])
        e1 = obs[:, 1] - ((y / z) * K[1] + K[3])
    return e0, e1


def _chi2(e0, e1, s):
    with np.errstate(all="ignore"):
        return e0 * (s * e0) + e1 * (s * e1)


def _seq(a12, a21, act, e21_first=False):
    """The ordered sum over the active edges: e12(i), e21(i), e12(i'), ... from +0.0."""
    n = int(act.sum())
    v = np.empty(2 * n + 1, f64)
    v[0] = 0.0
    first, second = (a21, a12) if e21_first else (a12, a21)
    v[1::2] = first[act]
    v[2::2] = second[act]
    with np.errstate(all="ignore"):
        return float(np.add.accumulate(v)[-1])


def new_trace():
    return dict(exp_step=set(), exp_perturb=set(), quat_start=set(), quat_step=set(),
                quat_perturb=set(), exp_args=set(), pivots=set(), pivot_ties=0, ended=[],
                iterations=[], rejected_trials=0, not_positive=0, n_bad=0, gate=None,
                huber_inlier=False, huber_outlier=False, final_chi2=[], stale_rounds=0,
                skipped=dict(null_match=0, null_mp1=0, bad=0, i2_negative=0))


def optimize_sim3(keys1_xy, octave1, point_index1, pose1, keys2_xy, octave2, pose2, points_pos,
                  points_bad, match12, index2, start, inv_level_sigma2, K1, K2, th2, fix_scale,
                  n1=None, n2=None, libm=False, variants=()):
    """Optimizer::OptimizeSim3 (src/Optimizer.cc:1130-1326).  pose1 / pose2:
    (rcw 9, tcw 3); start: (R 9, t 3, scale) floats.  Returns a dict: status,
    n_corr, n_bad, n_inliers, q, t, s, R, t_f, s_f, match12 (the updated copy)
    and `trace`.  variants names wrong neighbours, none of them the reference
    (VARIANTS)."""
    variants = tuple(variants)
    assert all(v in VARIANTS for v in variants)
    keys1_xy = np.asarray(keys1_xy, f32).reshape(-1, 2)
    keys2_xy = np.asarray(keys2_xy, f32).reshape(-1, 2)
    n1 = len(keys1_xy) if n1 is None else int(n1)
    n2 = len(keys2_xy) if n2 is None else int(n2)
    levels = np.asarray(inv_level_sigma2, f32)
    pos = np.asarray(points_pos, f32).reshape(-1, 3)
    match = np.array(match12, np.int32)
    trace = new_trace()
    est0 = sim3_from_start(start[0], start[1], start[2], trace, variants)

    def result(status, n_corr, n_bad, n_in, est):
        q, t, s = est
        with np.errstate(all="ignore"):
            R = np.array(quat_to_matrix(q), f64).astype(f32).reshape(9)
            tf = np.array(t, f64).astype(f32)
            sf = f32(f64(s))
        return dict(status=status, n_corr=n_corr, n_bad=n_bad, n_inliers=n_in, q=np.array(q, f64),
                    t=np.array(t, f64), s=float(s), R=R, t_f=tf, s_f=sf, match12=match, trace=trace)

    # ---- the pairs, in ascending i (:1183-1262)
    idx, i2s, m1s, m2s = [], [], [], []
    for i in range(n1):
        m2 = int(match[i])
        if m2 < 0:
            trace["skipped"]["null_match"] += 1
            continue
        m1 = int(point_index1[i])
        if m1 < 0:
            trace["skipped"]["null_mp1"] += 1
            continue
        if points_bad[m1] or points_bad[m2]:
            trace["skipped"]["bad"] += 1
            continue
        i2 = int(index2[i])
        if i2 < 0:
            trace["skipped"]["i2_negative"] += 1
            continue
        if i2 >= n2 or not (0 <= int(octave1[i]) < len(levels)) or \
                not (0 <= int(octave2[i2]) < len(levels)):
            match = np.array(match12, np.int32)
            return result(-1, 0, 0, 0, est0)
        idx.append(i)
        i2s.append(i2)
        m1s.append(m1)
        m2s.append(m2)
    E = len(idx)
    idx = np.asarray(idx, np.int64)
    i2s = np.asarray(i2s, np.int64)

    def transform(pose, X):  # pin O1
        r, t = np.asarray(pose[0], f32).reshape(9), np.asarray(pose[1], f32).reshape(3)
        with np.errstate(all="ignore"):
            return np.stack([((r[3 * k] * X[:, 0] + r[3 * k + 1] * X[:, 1]) + r[3 * k + 2] * X[:, 2])
                             + t[k] for k in range(3)], 1)

    X1 = transform(pose1, pos[np.asarray(m1s, np.int64)].reshape(-1, 3)).astype(f64).reshape(-1, 3)
    X2 = transform(pose2, pos[np.asarray(m2s, np.int64)].reshape(-1, 3)).astype(f64).reshape(-1, 3)
    obs1 = keys1_xy[idx].astype(f64).reshape(-1, 2)
    obs2 = keys2_xy[i2s].astype(f64).reshape(-1, 2)
    inv1 = levels[np.asarray(octave1, np.int64)[idx]].astype(f64)
    inv2 = levels[np.asarray(octave2, np.int64)[i2s]].astype(f64)
    Kd1 = [float(f32(v)) for v in K1[:4]]
    Kd2 = [float(f32(v)) for v in K2[:4]]
    th2f = f32(th2)
    th2d = float(th2f)
    delta = float(f32(np.sqrt(f64(th2f))))  # const float deltaHuber = sqrt(th2) (:1179)
    fix_scale = bool(fix_scale)
    e21_first = "e21_first" in variants
    removed = np.zeros(E, bool)
    est = est0
    last = est
    x = [0.0] * 7  # BlockSolver::_x
    n_bad = 0

    def errors(e):
        a0, a1 = edge_error(e, X2, obs1, Kd1)                 # e12: x1 = S12 * X2
        b0, b1 = edge_error(sim3_inverse(e), X1, obs2, Kd2)   # e21: x2 = S21 * X1
        return a0, a1, b0, b1

    def robust(c12, c21, act):
        r12 = huber(c12, delta, "huber_lt" in variants)
        r21 = huber(c21, delta, "huber_lt" in variants)
        if act.any():
            inl = np.concatenate([r12[2][act], r21[2][act]])
            trace["huber_inlier"] |= bool(inl.any())
            trace["huber_outlier"] |= bool((~inl).any())
        return _seq(r12[0], r21[0], act, e21_first), r12[1], r21[1]

    def oplus(e, u):
        """VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69): u is
        changed in place."""
        if fix_scale:
            u[6] = 0.0
        return u

    for rnd in range(2):
        iters = 5 if rnd == 0 else (10 if n_bad > 0 else 5)  # :1266, :1289-1301
        act = ~removed
        if act.any():  # (optimize() returns at once without active vertices)
            lam, ni, nbad_steps = 0.0, 2.0, 0
            ended = "iterations"
            cur = 0.0
            done = 0
            for i in range(iters):
                done += 1
                a0, a1, b0, b1 = errors(est)
                c12, c21 = _chi2(a0, a1, inv1), _chi2(b0, b1, inv2)
                cur, rho12, rho21 = robust(c12, c21, act)
                ini = cur
                # linearizeOplus (base_binary_edge.hpp:131-200), pin O2
                scalar = 1.0 / (2 * 1e-9)
                J12 = [[None] * 7, [None] * 7]
                J21 = [[None] * 7, [None] * 7]
                for d in range(7):
                    ev = []
                    for step in (1e-9, -1e-9):
                        u = [0.0] * 7
                        u[d] = step
                        oplus(est, u)
                        pe = sim3_mul(sim3_exp(u, libm, trace, "perturb", variants), est, variants)
                        ev.append(errors(pe))
                    with np.errstate(all="ignore"):
                        if "forward_diff" in variants:
                            base = (a0, a1, b0, b1)
                            cols = [(1.0 / 1e-9) * (ev[0][k] - base[k]) for k in range(4)]
                        else:
                            cols = [scalar * (ev[0][k] - ev[1][k]) for k in range(4)]
                    J12[0][d], J12[1][d], J21[0][d], J21[1][d] = cols
                # constructQuadraticForm (:91-113), pin O3
                H = [[0.0] * 7 for _ in range(7)]
                b = [0.0] * 7
                with np.errstate(all="ignore"):
                    w12, w21 = rho12 * inv1, rho21 * inv2
                    r12 = [(-(inv1 * a0)) * rho12, (-(inv1 * a1)) * rho12]
                    r21 = [(-(inv2 * b0)) * rho21, (-(inv2 * b1)) * rho21]
                    for q in range(7):
                        if "unary_assoc" in variants:
                            t12 = -(((rho12 * J12[0][q]) * inv1) * a0 + ((rho12 * J12[1][q]) * inv1) * a1)
                            t21 = -(((rho21 * J21[0][q]) * inv2) * b0 + ((rho21 * J21[1][q]) * inv2) * b1)
                        else:
                            t12 = J12[0][q] * r12[0] + J12[1][q] * r12[1]
                            t21 = J21[0][q] * r21[0] + J21[1][q] * r21[1]
                        b[q] = _seq(t12, t21, act, e21_first)
                        for p in range(q + 1):
                            h12 = (J12[0][q] * w12) * J12[0][p] + (J12[1][q] * w12) * J12[1][p]
                            h21 = (J21[0][q] * w21) * J21[0][p] + (J21[1][q] * w21) * J21[1][p]
                            H[q][p] = _seq(h12, h21, act, e21_first)
                if i == 0:  # computeLambdaInit (:166-180)
                    md = 0.0
                    for j in range(7):
                        a = abs(H[j][j])
                        md = md if a < md else a
                    lam, ni, nbad_steps = 1e-5 * md, 2.0, 0
                rho, qmax = 0.0, 0
                while True:
                    backup = est
                    Hl = [list(r) for r in H]
                    for j in range(7):
                        Hl[j][j] = H[j][j] + lam
                    ok2, x = ldlt_solve(Hl, b, x, None, trace, variants)
                    if not ok2:
                        trace["not_positive"] += 1
                    oplus(est, x)  # pin O6: the solver's array
                    est = sim3_mul(sim3_exp(x, libm, trace, "step", variants), est, variants)
                    last = est
                    t0, t1, t2, t3 = errors(est)
                    tmp, _, _ = robust(_chi2(t0, t1, inv1), _chi2(t2, t3, inv2), act)
                    if not ok2:
                        tmp = DBL_MAX
                    scale = 0.0
                    for j in range(7):  # computeScale (:182-189)
                        scale = scale + x[j] * (lam * x[j] + b[j])
                    scale = scale + 1e-3
                    rho = _div(cur - tmp, scale)
                    if rho > 0 and math.isfinite(tmp):
                        y = 2 * rho - 1
                        alpha = 1.0 - (math.pow(y, 3) if libm else (y * y) * y)
                        alpha = 2.0 / 3.0 if 2.0 / 3.0 < alpha else alpha
                        sf = alpha if 1.0 / 3.0 < alpha else 1.0 / 3.0
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
                    nbad_steps += 1
                else:
                    nbad_steps = 0
                if nbad_steps >= 3:
                    ended = "nbad"
                    break
            trace["ended"].append(ended)
            trace["iterations"].append(done)
            trace["final_chi2"].append(cur)
            if last is not est:
                trace["stale_rounds"] += 1
        # ---- the check (:1268-1287, :1303-1319), pin O5
        at = est if "classify_from_final" in variants else last
        a0, a1, b0, b1 = errors(at)
        c12, c21 = _chi2(a0, a1, inv1), _chi2(b0, b1, inv2)
        with np.errstate(all="ignore"):
            if "chi2_float" in variants:
                bad = (c12.astype(f32) > th2f) | (c21.astype(f32) > th2f)
            else:
                bad = (c12 > th2d) | (c21 > th2d)
        bad &= act
        match[idx[bad]] = -1
        removed |= bad
        if rnd == 0:
            n_bad = int(bad.sum())
            trace["n_bad"] = n_bad
            if E - n_bad < 10:  # :1295-1296
                trace["gate"] = "early"
                return result(0, E, n_bad, 0, est0)
            trace["gate"] = "second_%d" % (10 if n_bad > 0 else 5)
        else:
            n_in = int((act & ~bad).sum())
    return result(0, E, n_bad, n_in, est)


def result_record(res) -> np.ndarray:
    """The orb_sim3_opt_result_t the device writes for `res`."""
    r = np.zeros(1, OPT_RESULT_DTYPE)
    for k in ("status", "n_corr", "n_bad", "n_inliers", "q", "t", "s", "R", "t_f", "s_f"):
        r[k][0] = res[k]
    return r
