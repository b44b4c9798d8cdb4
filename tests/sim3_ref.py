"""Sim3Solver (src/Sim3Solver.cc, include/Sim3Solver.h) restated in Python (test
infrastructure): the parity target of k_sim3_setup and k_sim3_iterate.

A `Sim3Solver` class with the reference's method names (the constructor,
SetRansacParameters, iterate, find, ComputeCentroid, ComputeSim3, CheckInliers,
Project, FromCameraToImage and the three getters).  Scalars are Python floats
(IEEE doubles) or np.float32 exactly where the reference has double or float;
the per-correspondence arithmetic of Project / CheckInliers is elementwise
numpy float32 (IEEE, operation order as written); every sum is explicit and
ordered; np.dot, @ and np.linalg are never used.  The RANSAC draws are an
input: raw rand() values, entry 3 * it + j for lifetime iteration `it`, draw j.

Pins (the same list stands in include/orb_abi.h and DESIGN.md 4.9; OpenCV
itself is not available to the project: unpinned against a real OpenCV).
Float expressions are evaluated as written, no contraction.
 P1  Rcw * X + tcw (constructor, Project): ((r0 x + r1 y) + r2 z) + t in
     float, the project's existing pin; 1 / z, x * invz, fx * x + cx in float.
 P2  scalar * Mat and Mat / scalar: the double scalar narrowed to float, then
     v * s + 0.0f per element (cvtScale_).  C / P.cols is
     c * (float)(1.0 / 3) + 0.0f; 2 * ang * vec / norm(vec) has
     s = (float)((2.0 * ang) * (1.0 / norm)); sR = R * ms12i;
     sRinv = R^T * (float)(1.0 / (double)ms12i).
 P3  cv::reduce(P, C, 1, CV_REDUCE_SUM) over three columns:
     (p0 + p2) + p1 in float (reduceC_'s two accumulators).
 P4  A * B.t() (M = Pr2 * Pr1.t()): per element a double accumulator from 0,
     k ascending, exact double products, narrowed once to float.
 P5  A * B of 3 x 3 floats without a transpose (P3 = R * Pr2):
     (a0 b0 + a1 b1) + a2 b2 in float.
 P6  N11..N44: the float expressions as written, left to right (the doubles
     that hold them narrow back to the same floats).
 P7  cv::eigen on the symmetric 4 x 4 float matrix: OpenCV 3.x's
     JacobiImpl_<float>, step by step: V = I, W = diag(A); indR[k] = the first
     largest |A[k][m]|, m > k; indC[k] = the first largest |A[i][k]|, i < k;
     up to 30 n^2 = 480 sweeps of: the pivot (k, l) = the first largest of
     |A[i][indR[i]]|, i = 0..n-2, then of |A[indC[i]][i]|, i = 1..n-1
     (strictly larger replaces); p = A[k][l]; stop when |p| <= FLT_EPSILON;
     y = (float)((W[l] - W[k]) * 0.5); t = |y| + hypot(p, y); s = hypot(p, t);
     c = t / s; s = p / s; t = (p / t) * p; y < 0 negates s and t;
     A[k][l] = 0; W[k] -= t; W[l] += t; rotate(a, b) = (a c - b s, a s + b c)
     over (A[i][k], A[i][l]) i < k, (A[k][i], A[i][l]) k < i < l,
     (A[k][i], A[l][i]) i > l, and (V[k][i], V[l][i]) all i; indR and indC
     recomputed for k and l only.  Then a selection sort, descending (swap
     with the first largest remaining, strict <), eigenvectors as rows.
     hypot(a, b) = (float)sqrt((double)a * a + (double)b * b).
 P8  cv::norm(vec): sqrt(((0 + v0 v0) + v1 v1) + v2 v2), products and sums in
     double; cv::norm returns that double.
 P9  atan2 on doubles: fdlibm's e_atan2.c over s_atan.c, built from IEEE
     operations alone (pinned_atan2), no libm call on either side.
 P10 cv::Rodrigues, vector to matrix, in double: theta = sqrt((rx rx + ry ry)
     + rz rz); theta < DBL_EPSILON gives I; else c, s = pinned_sincos_d(theta),
     c1 = 1 - c, r *= 1 / theta, R_ij = (c I_ij + c1 r_i r_j) + s [r]x_ij,
     each narrowed to float.
 P11 Mat::dot: a double accumulator over the elements row-major, unrolled by
     four: r += ((p0 + p1) + p2) + p3 per group, then r += p one at a time,
     with exact double products (nom over nine elements, err over two).
 P12 cv::pow(P3, 2): x * x in float; den adds those floats into a double,
     row-major; ms12i = (float)(nom / den).
 P13 the folded O1 - ms12i * mR12i * O2 (one gemm): u_k = (R_k0 o0 + R_k1 o1)
     + R_k2 o2 in float, t_k = (float)((double)u_k * -(double)ms12i +
     (double)O1_k).
 P14 tinv = -sRinv * mt12i: 0.0f - ((a0 t0 + a1 t1) + a2 t2) in float.
 P15 pow(epsilon, 3) = (x * x) * x in double; log = pinned_log; sin and cos =
     pinned_sincos_d; sqrt and / are IEEE.
 P16 thresholds: (float)(uint64_t)(9.210 * (double)sigma2).
libm=True uses math.atan2 / math.sin / math.cos / math.log / math.pow /
math.hypot instead of P9, P10's sincos, P15 and P7's hypot.
"""
from __future__ import annotations

import math
import struct

import numpy as np

from poseopt_ref import pinned_sincos_d

f32, f64 = np.float32, np.float64
FLT_EPSILON = f32(1.1920928955078125e-07)
DBL_EPSILON = 2.2204460492503131e-16

# rule switches (tests/test_sim3_ref.py): each replaces one reference rule by a
# plausible wrong one
SWITCHES = ("best_gt", "min_ge", "thr_double", "draw_replace", "inliers_compact",
            "nomore_on_success", "ignore_fix_scale", "skip_order")


def _bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _from_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b & 0xFFFFFFFFFFFFFFFF))[0]


def _hi(x: float) -> int:
    h = _bits(x) >> 32
    return h - (1 << 32) if h & 0x80000000 else h


def _div(a: float, b: float) -> float:
    with np.errstate(all="ignore"):
        return float(f64(a) / f64(b))


def _sqrt(x: float) -> float:
    with np.errstate(all="ignore"):
        return float(np.sqrt(f64(x)))


def _mul(a: float, b: float) -> float:
    with np.errstate(all="ignore"):
        return float(f64(a) * f64(b))


def _to_f32(x: float):
    with np.errstate(all="ignore"):
        return f32(f64(x))


# ------------------------------------------------------------------ pins
def pinned_log(x: float) -> float:
    """DESIGN.md App. A.7 (orb_device.h pinned_log), the same operation sequence."""
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    L1, L2, L3 = 6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01
    L4, L5, L6 = 2.222219843214978396e-01, 1.818357216161805012e-01, 1.531383769920937332e-01
    L7 = 1.479819860511658591e-01
    if not (x > 0.0):
        return -math.inf if x == 0.0 else math.nan
    if x == math.inf:
        return x
    bits = _bits(x)
    hx = bits >> 32
    lx = bits & 0xFFFFFFFF
    k = (hx >> 20) - 1023
    hx &= 0x000FFFFF
    i = (hx + 0x95F64) & 0x100000
    m = _from_bits(((hx | (i ^ 0x3FF00000)) << 32) | lx)
    k += i >> 20
    f = m - 1.0
    dk = float(k)
    if (0x000FFFFF & (2 + hx)) < 3:
        if f == 0.0:
            return 0.0 if k == 0 else dk * ln2_hi + dk * ln2_lo
        R = f * f * (0.5 - 0.33333333333333333 * f)
        return f - R if k == 0 else dk * ln2_hi - ((R - dk * ln2_lo) - f)
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (L2 + w * (L4 + w * L6))
    t2 = z * (L1 + w * (L3 + w * (L5 + w * L7)))
    R = t2 + t1
    if ((hx - 0x6147A) | (0x6B851 - hx)) > 0:
        hf = 0.5 * f * f
        if k == 0:
            return f - (hf - s * (hf + R))
        return dk * ln2_hi - ((hf - (s * (hf + R) + dk * ln2_lo)) - f)
    if k == 0:
        return f - s * (f - R)
    return dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f)


_ATANHI = (4.63647609000806093515e-01, 7.85398163397448278999e-01,
           9.82793723247329054082e-01, 1.57079632679489655800e+00)
_ATANLO = (2.26987774529616870924e-17, 3.06161699786838301793e-17,
           1.39033110312309984516e-17, 6.12323399573676603587e-17)
_AT = (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01,
       -1.11111104054623557880e-01, 9.09088713343650656196e-02, -7.69187620504482999495e-02,
       6.66107313738753120669e-02, -5.83357013379057348645e-02, 4.97687799461593236017e-02,
       -3.65315727442169155270e-02, 1.62858201153657823623e-02)


def pinned_atan(x: float) -> float:
    """fdlibm s_atan.c (P9)."""
    hx = _hi(x)
    ix = hx & 0x7FFFFFFF
    if ix >= 0x44100000:
        if x != x:
            return x + x
        return _ATANHI[3] + _ATANLO[3] if hx > 0 else -_ATANHI[3] - _ATANLO[3]
    if ix < 0x3FDC0000:
        if ix < 0x3E200000:
            return x
        idn = -1
    else:
        x = abs(x)
        if ix < 0x3FF30000:
            if ix < 0x3FE60000:
                idn = 0
                x = (2.0 * x - 1.0) / (2.0 + x)
            else:
                idn = 1
                x = (x - 1.0) / (x + 1.0)
        elif ix < 0x40038000:
            idn = 2
            x = (x - 1.5) / (1.0 + 1.5 * x)
        else:
            idn = 3
            x = -1.0 / x
    z = x * x
    w = z * z
    aT = _AT
    s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))))
    s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))))
    if idn < 0:
        return x - x * (s1 + s2)
    r = _ATANHI[idn] - ((x * (s1 + s2) - _ATANLO[idn]) - x)
    return -r if hx < 0 else r


def pinned_atan2(y: float, x: float) -> float:
    """fdlibm e_atan2.c (P9)."""
    pi, pi_o_2 = 3.1415926535897931160e+00, 1.5707963267948965580e+00
    pi_o_4, pi_lo = 7.8539816339744827900e-01, 1.2246467991473531772e-16
    if x != x or y != y:
        return x + y
    hx, hy = _hi(x), _hi(y)
    ix, iy = hx & 0x7FFFFFFF, hy & 0x7FFFFFFF
    if x == 1.0:
        return pinned_atan(y)
    m = (1 if hy < 0 else 0) | (2 if hx < 0 else 0)
    if y == 0.0:
        return y if m in (0, 1) else (pi if m == 2 else -pi)
    if x == 0.0:
        return -pi_o_2 if hy < 0 else pi_o_2
    if abs(x) == math.inf:
        if abs(y) == math.inf:
            return (pi_o_4, -pi_o_4, 3.0 * pi_o_4, -3.0 * pi_o_4)[m]
        return (0.0, -0.0, pi, -pi)[m]
    if abs(y) == math.inf:
        return -pi_o_2 if hy < 0 else pi_o_2
    k = (iy - ix) >> 20
    if k > 60:
        z = pi_o_2 + 0.5 * pi_lo
    elif hx < 0 and k < -60:
        z = 0.0
    else:
        z = pinned_atan(abs(_div(y, x)))
    if m == 0:
        return z
    if m == 1:
        return -z
    if m == 2:
        return pi - (z - pi_lo)
    return (z - pi_lo) - pi


def _hypot(a, b, libm=False):
    """P7's hypot on floats."""
    if libm:
        return _to_f32(math.hypot(float(a), float(b)))
    return _to_f32(_sqrt(_mul(float(a), float(a)) + _mul(float(b), float(b))))


def jacobi_eigen4(N, libm=False):
    """cv::eigen on a symmetric 4 x 4 float matrix (P7): returns (W, V, sweeps),
    eigenvalues descending and eigenvectors as the rows of V, all np.float32."""
    n = 4
    A = [[f32(N[i][j]) for j in range(n)] for i in range(n)]
    V = [[f32(1) if i == j else f32(0) for j in range(n)] for i in range(n)]
    W = [f32(0)] * n
    indR = [0] * n
    indC = [0] * n

    def row_max(k):
        m = k + 1
        mv = abs(A[k][m])
        for i in range(k + 2, n):
            val = abs(A[k][i])
            if mv < val:
                mv, m = val, i
        return m

    def col_max(k):
        m = 0
        mv = abs(A[0][k])
        for i in range(1, k):
            val = abs(A[i][k])
            if mv < val:
                mv, m = val, i
        return m

    for k in range(n):
        W[k] = A[k][k]
        if k < n - 1:
            indR[k] = row_max(k)
        if k > 0:
            indC[k] = col_max(k)
    sweeps = 0
    with np.errstate(all="ignore"):
        for _ in range(n * n * 30):
            k = 0
            mv = abs(A[0][indR[0]])
            for i in range(1, n - 1):
                val = abs(A[i][indR[i]])
                if mv < val:
                    mv, k = val, i
            l = indR[k]
            for i in range(1, n):
                val = abs(A[indC[i]][i])
                if mv < val:
                    mv, k, l = val, indC[i], i
            p = A[k][l]
            if abs(p) <= FLT_EPSILON:
                break
            sweeps += 1
            y = _to_f32(float(W[l] - W[k]) * 0.5)
            t = abs(y) + _hypot(p, y, libm)
            s = _hypot(p, t, libm)
            c = t / s
            s = p / s
            t = (p / t) * p
            if y < 0:
                s, t = -s, -t
            A[k][l] = f32(0)
            W[k] = W[k] - t
            W[l] = W[l] + t

            def rot(a0, b0):
                return a0 * c - b0 * s, a0 * s + b0 * c

            for i in range(k):
                A[i][k], A[i][l] = rot(A[i][k], A[i][l])
            for i in range(k + 1, l):
                A[k][i], A[i][l] = rot(A[k][i], A[i][l])
            for i in range(l + 1, n):
                A[k][i], A[l][i] = rot(A[k][i], A[l][i])
            for i in range(n):
                V[k][i], V[l][i] = rot(V[k][i], V[l][i])
            for idx in (k, l):
                if idx < n - 1:
                    indR[idx] = row_max(idx)
                if idx > 0:
                    indC[idx] = col_max(idx)
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            V[m], V[k] = V[k], V[m]
    return W, V, sweeps


def rodrigues(rvec, libm=False):
    """cv::Rodrigues, vector to matrix (P10): 3 floats -> 3 x 3 np.float32."""
    rx, ry, rz = (float(v) for v in rvec)
    theta = _sqrt((_mul(rx, rx) + _mul(ry, ry)) + _mul(rz, rz))
    if theta < DBL_EPSILON:
        return [[f32(1) if i == j else f32(0) for j in range(3)] for i in range(3)]
    if libm and math.isfinite(theta):
        sn, cs = math.sin(theta), math.cos(theta)
    else:
        sn, cs = pinned_sincos_d(theta)
    c1 = 1.0 - cs
    itheta = _div(1.0, theta)
    r = (_mul(rx, itheta), _mul(ry, itheta), _mul(rz, itheta))
    rxm = ((0.0, -r[2], r[1]), (r[2], 0.0, -r[0]), (-r[1], r[0], 0.0))
    R = []
    for i in range(3):
        row = []
        for j in range(3):
            e = 1.0 if i == j else 0.0
            with np.errstate(all="ignore"):
                v = float((f64(cs) * f64(e) + f64(c1) * (f64(r[i]) * f64(r[j]))) +
                          f64(sn) * f64(rxm[i][j]))
            row.append(_to_f32(v))
        R.append(row)
    return R


def max_error(sigma2) -> np.float32:
    """P16: the size_t threshold as the float the comparison converts it to."""
    return f32(int(9.210 * float(f32(sigma2))))


def random_int(r: int, rand_max: int, d: int) -> int:
    """DUtils::Random::RandomInt(0, d - 1) on the raw rand() value r."""
    return int((float(r) / (float(rand_max) + 1.0)) * d)


def ransac_iterations(N: int, probability: float, min_inliers: int, max_iterations: int,
                      libm=False) -> int:
    """SetRansacParameters (:117-141): mRansacMaxIts (N >= min_inliers)."""
    if min_inliers == N:
        n_it = 1
    else:
        with np.errstate(all="ignore"):
            epsilon = f32(min_inliers) / f32(N)
        e = float(epsilon)
        if libm:
            q = math.ceil(math.log(1.0 - probability) / math.log(1.0 - math.pow(e, 3)))
        else:
            q = math.ceil(_div(pinned_log(1.0 - probability), pinned_log(1.0 - (e * e) * e)))
        n_it = max_iterations if q >= max_iterations else int(q)
    return max(1, min(n_it, max_iterations))


# ------------------------------------------------------------ the solver
class KeyFrame:
    """What Sim3Solver reads of a KeyFrame: mvKeysUn's octaves, the map point
    index per keypoint (< 0: NULL), the pose (rcw row-major 9, tcw 3) and the
    count of valid keypoint slots."""

    def __init__(self, octave, point_index, rcw, tcw, nkeys=None):
        self.octave = np.asarray(octave, np.int32)
        self.point_index = np.asarray(point_index, np.int32)
        self.rcw = np.asarray(rcw, f32).reshape(9)
        self.tcw = np.asarray(tcw, f32).reshape(3)
        self.nkeys = len(self.octave) if nkeys is None else int(nkeys)


class Sim3Solver:
    def __init__(self, pKF1: KeyFrame, pKF2: KeyFrame, vpMatched12, bFixScale, *, points_pos,
                 points_bad, index2, index1=None, level_sigma2, K1, K2, draws, rand_max=2147483647,
                 probability=0.99, minInliers=20, maxIterations=300, libm=False, switch=None):
        assert switch is None or switch in SWITCHES
        self.libm, self.switch = libm, switch
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.mbFixScale = bool(bFixScale)
        self.status = 0
        self.best_iteration = 0
        self.draws = np.asarray(draws, np.uint32)
        self.rand_max = int(rand_max)
        self.K1 = [f32(v) for v in K1]
        self.K2 = [f32(v) for v in K2]
        level_sigma2 = np.asarray(level_sigma2, f32)
        n_levels = len(level_sigma2)
        self.mN1 = min(max(pKF1.nkeys, 0), len(vpMatched12))
        n2 = min(max(pKF2.nkeys, 0), len(pKF2.octave))
        pos = np.asarray(points_pos, f32)

        self.mvnIndices1, X1, X2, e1, e2 = [], [], [], [], []
        for i1 in range(self.mN1):
            m2 = int(vpMatched12[i1])
            if m2 < 0:
                continue
            m1 = int(pKF1.point_index[i1])
            k1 = i1 if index1 is None else int(index1[i1])
            k2 = int(index2[i1])
            if self.switch == "skip_order":
                # the indices checked (and so read) before NULL pMP1 and isBad()
                if k1 < 0 or k2 < 0:
                    continue
                if k1 >= self.mN1 or k2 >= n2:
                    self.status = -1
                    break
            if m1 < 0:
                continue
            if points_bad[m1] or points_bad[m2]:
                continue
            if k1 < 0 or k2 < 0:
                continue
            if k1 >= self.mN1 or k2 >= n2:
                self.status = -1
                break
            o1, o2 = int(pKF1.octave[k1]), int(pKF2.octave[k2])
            if not (0 <= o1 < n_levels and 0 <= o2 < n_levels):
                self.status = -1
                break
            if self.switch == "thr_double":
                e1.append(9.210 * float(level_sigma2[o1]))
                e2.append(9.210 * float(level_sigma2[o2]))
            else:
                e1.append(max_error(level_sigma2[o1]))
                e2.append(max_error(level_sigma2[o2]))
            self.mvnIndices1.append(i1)
            X1.append(self._transform(pKF1.rcw, pKF1.tcw, pos[m1]))
            X2.append(self._transform(pKF2.rcw, pKF2.tcw, pos[m2]))
        if self.status < 0:
            self.mvnIndices1, X1, X2, e1, e2 = [], [], [], [], []
        self.mvX3Dc1 = np.asarray(X1, f32).reshape(-1, 3)
        self.mvX3Dc2 = np.asarray(X2, f32).reshape(-1, 3)
        self.mvnMaxError1 = np.asarray(e1, f64 if self.switch == "thr_double" else f32)
        self.mvnMaxError2 = np.asarray(e2, f64 if self.switch == "thr_double" else f32)
        self.mvP1im1 = self.FromCameraToImage(self.mvX3Dc1, self.K1)
        self.mvP2im2 = self.FromCameraToImage(self.mvX3Dc2, self.K2)
        self.mvbBestInliers = np.zeros(len(self.mvnIndices1), bool)
        self.mBestT12 = np.zeros((4, 4), f32)
        self.mBestRotation = np.zeros((3, 3), f32)
        self.mBestTranslation = np.zeros(3, f32)
        self.mBestScale = f32(0)
        self.SetRansacParameters(probability, minInliers, maxIterations)

    @staticmethod
    def _transform(rcw, tcw, x):
        """Rcw * X + tcw (P1)."""
        with np.errstate(all="ignore"):
            return [((rcw[3 * k] * x[0] + rcw[3 * k + 1] * x[1]) + rcw[3 * k + 2] * x[2]) + tcw[k]
                    for k in range(3)]

    def SetRansacParameters(self, probability=0.99, minInliers=20, maxIterations=300):
        self.mRansacProb = float(probability)
        self.mRansacMinInliers = int(minInliers)
        self.N = len(self.mvnIndices1)
        self.mvbInliersi = np.zeros(self.N, bool)
        if self.status < 0 or self.N < self.mRansacMinInliers:
            self.mRansacMaxIts = 0  # never read (:151-156)
        else:
            self.mRansacMaxIts = ransac_iterations(self.N, self.mRansacProb,
                                                   self.mRansacMinInliers, int(maxIterations),
                                                   self.libm)
        self.mnIterations = 0

    # ------------------------------------------------------------- iterate
    def iterate(self, nIterations):
        """Returns (T12 or None, bNoMore, vbInliers, nInliers); .iterations_run
        holds nCurrentIterations."""
        bNoMore = False
        vbInliers = np.zeros(self.mN1, bool)
        nInliers = 0
        self.iterations_run = 0
        if self.status < 0 or self.N < self.mRansacMinInliers:
            return None, True, vbInliers, nInliers
        nCurrentIterations = 0
        while self.mnIterations < self.mRansacMaxIts and nCurrentIterations < nIterations:
            it = self.mnIterations
            rs = [int(self.draws[3 * it + j]) for j in range(3)]
            if any(r > self.rand_max for r in rs):  # malformed: the iteration is not run
                self.status = -1
                self.iterations_run = nCurrentIterations
                return None, True, vbInliers, nInliers
            nCurrentIterations += 1
            self.mnIterations += 1
            vAvailableIndices = list(range(self.N))
            idx3 = []
            for j in range(3):
                randi = random_int(rs[j], self.rand_max, len(vAvailableIndices))
                idx3.append(vAvailableIndices[randi])
                if self.switch != "draw_replace":
                    vAvailableIndices[randi] = vAvailableIndices[-1]
                    vAvailableIndices.pop()
            P3Dc1i = [[self.mvX3Dc1[idx3[c]][r] for c in range(3)] for r in range(3)]
            P3Dc2i = [[self.mvX3Dc2[idx3[c]][r] for c in range(3)] for r in range(3)]
            self.ComputeSim3(P3Dc1i, P3Dc2i)
            self.CheckInliers()
            better = self.mnInliersi > self.mnBestInliers if self.switch == "best_gt" \
                else self.mnInliersi >= self.mnBestInliers
            if better:
                self.mvbBestInliers = self.mvbInliersi.copy()
                self.mnBestInliers = self.mnInliersi
                self.mBestT12 = np.array(self.mT12i, f32)
                self.mBestRotation = np.array(self.mR12i, f32)
                self.mBestTranslation = np.array(self.mt12i, f32)
                self.mBestScale = self.ms12i
                self.best_iteration = self.mnIterations
                enough = self.mnInliersi >= self.mRansacMinInliers if self.switch == "min_ge" \
                    else self.mnInliersi > self.mRansacMinInliers
                if enough:
                    nInliers = self.mnInliersi
                    for i in range(self.N):
                        if self.mvbInliersi[i]:
                            if self.switch == "inliers_compact":
                                vbInliers[i] = True
                            else:
                                vbInliers[self.mvnIndices1[i]] = True
                    self.iterations_run = nCurrentIterations
                    if self.switch == "nomore_on_success":
                        bNoMore = self.mnIterations >= self.mRansacMaxIts
                    return self.mBestT12.copy(), bNoMore, vbInliers, nInliers
        self.iterations_run = nCurrentIterations
        if self.mnIterations >= self.mRansacMaxIts:
            bNoMore = True
        return None, bNoMore, vbInliers, nInliers

    def find(self):
        T, _, vbInliers12, nInliers = self.iterate(self.mRansacMaxIts)
        return T, vbInliers12, nInliers

    # --------------------------------------------------------- ComputeSim3
    @staticmethod
    def ComputeCentroid(P):
        """P[row][col] -> (Pr, C) (P3, P2)."""
        third = _to_f32(1.0 / 3.0)
        with np.errstate(all="ignore"):
            C = [((P[r][0] + P[r][2]) + P[r][1]) * third + f32(0) for r in range(3)]
            Pr = [[P[r][c] - C[r] for c in range(3)] for r in range(3)]
        return Pr, C

    def ComputeSim3(self, P1, P2):
        libm = self.libm
        Pr1, O1 = self.ComputeCentroid(P1)
        Pr2, O2 = self.ComputeCentroid(P2)
        # Step 2 (P4)
        M = [[None] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(3):
                acc = 0.0
                for k in range(3):
                    with np.errstate(all="ignore"):
                        acc = float(f64(acc) + f64(Pr2[i][k]) * f64(Pr1[j][k]))
                M[i][j] = _to_f32(acc)
        # Step 3 (P6)
        with np.errstate(all="ignore"):
            N11 = M[0][0] + M[1][1] + M[2][2]
            N12 = M[1][2] - M[2][1]
            N13 = M[2][0] - M[0][2]
            N14 = M[0][1] - M[1][0]
            N22 = M[0][0] - M[1][1] - M[2][2]
            N23 = M[0][1] + M[1][0]
            N24 = M[2][0] + M[0][2]
            N33 = -M[0][0] + M[1][1] - M[2][2]
            N34 = M[1][2] + M[2][1]
            N44 = -M[0][0] - M[1][1] + M[2][2]
        N = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34],
             [N14, N24, N34, N44]]
        # Step 4 (P7 P8 P9 P2 P10)
        _, evec, _ = jacobi_eigen4(N, libm)
        q0, q1, q2, q3 = (float(v) for v in evec[0])
        nrm = _sqrt(((0.0 + _mul(q1, q1)) + _mul(q2, q2)) + _mul(q3, q3))
        if libm and math.isfinite(nrm) and math.isfinite(q0):
            ang = math.atan2(nrm, q0)
        else:
            ang = pinned_atan2(nrm, q0)
        sc = _to_f32(_mul(2.0 * ang, _div(1.0, nrm)))
        with np.errstate(all="ignore"):
            vec = [f32(q) * sc + f32(0) for q in (q1, q2, q3)]
        R = rodrigues(vec, libm)
        self.mR12i = R
        # Step 5 (P5), Step 6 (P11 P12)
        with np.errstate(all="ignore"):
            P3 = [[(R[i][0] * Pr2[0][j] + R[i][1] * Pr2[1][j]) + R[i][2] * Pr2[2][j]
                   for j in range(3)] for i in range(3)]
            if not self.mbFixScale or self.switch == "ignore_fix_scale":
                pr = [f64(Pr1[i // 3][i % 3]) * f64(P3[i // 3][i % 3]) for i in range(9)]
                nom = f64(0)
                nom = nom + (((pr[0] + pr[1]) + pr[2]) + pr[3])
                nom = nom + (((pr[4] + pr[5]) + pr[6]) + pr[7])
                nom = nom + pr[8]
                den = f64(0)
                for i in range(9):
                    den = den + f64(P3[i // 3][i % 3] * P3[i // 3][i % 3])
                self.ms12i = f32(nom / den)
            else:
                self.ms12i = f32(1.0)
            s = self.ms12i
            # Step 7 (P13)
            t = []
            for k in range(3):
                u = (R[k][0] * O2[0] + R[k][1] * O2[1]) + R[k][2] * O2[2]
                t.append(f32(f64(u) * -f64(s) + f64(O1[k])))
            self.mt12i = t
            # Step 8 (P2 P14)
            T12 = [[f32(0)] * 4 for _ in range(4)]
            sinv = f32(f64(1.0) / f64(s))
            sRinv = [[None] * 3 for _ in range(3)]
            for i in range(3):
                for j in range(3):
                    T12[i][j] = R[i][j] * s + f32(0)
                    sRinv[i][j] = R[j][i] * sinv + f32(0)
                T12[i][3] = t[i]
            T12[3][3] = f32(1)
            self.mT12i = T12
            tinv = [f32(0) - ((sRinv[k][0] * t[0] + sRinv[k][1] * t[1]) + sRinv[k][2] * t[2])
                    for k in range(3)]
            self.mT21i = (sRinv, tinv)

    # -------------------------------------------------------- CheckInliers
    def CheckInliers(self):
        sR = [[self.mT12i[i][j] for j in range(3)] for i in range(3)]
        t12 = [self.mT12i[i][3] for i in range(3)]
        vP2im1 = self.Project(self.mvX3Dc2, sR, t12, self.K1)
        vP1im2 = self.Project(self.mvX3Dc1, self.mT21i[0], self.mT21i[1], self.K2)
        with np.errstate(all="ignore"):
            d1 = (self.mvP1im1 - vP2im1).astype(f64)
            d2 = (vP1im2 - self.mvP2im2).astype(f64)
            err1 = ((0.0 + d1[:, 0] * d1[:, 0]) + d1[:, 1] * d1[:, 1]).astype(f32)
            err2 = ((0.0 + d2[:, 0] * d2[:, 0]) + d2[:, 1] * d2[:, 1]).astype(f32)
            self.mvbInliersi = (err1 < self.mvnMaxError1) & (err2 < self.mvnMaxError2)
        self.mnInliersi = int(np.count_nonzero(self.mvbInliersi))

    @staticmethod
    def Project(vP3Dw, Rcw, tcw, K):
        """(:396-417), elementwise over the points (P1)."""
        X = np.asarray(vP3Dw, f32).reshape(-1, 3)
        x, y, z = X[:, 0], X[:, 1], X[:, 2]
        with np.errstate(all="ignore"):
            c = [((f32(Rcw[k][0]) * x + f32(Rcw[k][1]) * y) + f32(Rcw[k][2]) * z) + f32(tcw[k])
                 for k in range(3)]
            invz = f32(1) / c[2]
            px, py = c[0] * invz, c[1] * invz
            return np.stack([K[0] * px + K[2], K[1] * py + K[3]], axis=1).astype(f32)

    @staticmethod
    def FromCameraToImage(vP3Dc, K):
        """(:419-437)."""
        X = np.asarray(vP3Dc, f32).reshape(-1, 3)
        with np.errstate(all="ignore"):
            invz = f32(1) / X[:, 2]
            px, py = X[:, 0] * invz, X[:, 1] * invz
            return np.stack([K[0] * px + K[2], K[1] * py + K[3]], axis=1).astype(f32)

    def GetEstimatedRotation(self):
        return self.mBestRotation.copy()

    def GetEstimatedTranslation(self):
        return self.mBestTranslation.copy()

    def GetEstimatedScale(self):
        return self.mBestScale

    # ------------------------------------------ the device records' bytes
    def corr_records(self):
        """orb_sim3_corr_t per kept correspondence (include/orb_abi.h)."""
        rec = np.zeros(self.N, CORR_DTYPE)
        if self.N:
            rec["index1"] = self.mvnIndices1
            rec["x1"], rec["x2"] = self.mvX3Dc1, self.mvX3Dc2
            rec["p1"], rec["p2"] = self.mvP1im1, self.mvP2im2
            rec["max_err1"], rec["max_err2"] = self.mvnMaxError1, self.mvnMaxError2
            rec["best_inlier"] = self.mvbBestInliers
        return rec

    def state_record(self):
        """orb_sim3_state_t."""
        s = np.zeros(1, STATE_DTYPE)[0]
        s["status"], s["n1"] = self.status, self.mN1
        if self.status < 0 and self.N == 0:
            return s  # malformed in the constructor: every other field 0
        s["n"] = self.N
        s["max_its"], s["iterations"] = self.mRansacMaxIts, self.mnIterations
        s["best_inliers"], s["best_iteration"] = self.mnBestInliers, self.best_iteration
        s["min_inliers"], s["fix_scale"] = self.mRansacMinInliers, int(self.mbFixScale)
        s["best_scale"] = self.mBestScale
        s["best_R"] = np.asarray(self.mBestRotation, f32).reshape(9)
        s["best_t"] = np.asarray(self.mBestTranslation, f32).reshape(3)
        s["best_T12"] = np.asarray(self.mBestT12, f32).reshape(16)
        s["k1"], s["k2"] = self.K1, self.K2
        return s

    def result_record(self, T, bNoMore, nInliers):
        """orb_sim3_result_t of the last iterate."""
        r = np.zeros(1, RESULT_DTYPE)[0]
        r["has_sim3"], r["no_more"] = int(T is not None), int(bNoMore)
        r["n_inliers"], r["iterations_run"] = nInliers, self.iterations_run
        if T is not None:
            r["T12"] = np.asarray(T, f32).reshape(16)
            r["R"] = np.asarray(self.mBestRotation, f32).reshape(9)
            r["t"] = np.asarray(self.mBestTranslation, f32).reshape(3)
            r["scale"] = self.mBestScale
        return r


CORR_DTYPE = np.dtype([("index1", "<i4"), ("x1", "<f4", 3), ("x2", "<f4", 3), ("p1", "<f4", 2),
                       ("p2", "<f4", 2), ("max_err1", "<f4"), ("max_err2", "<f4"),
                       ("best_inlier", "u1"), ("_pad", "u1", 3)])
STATE_DTYPE = np.dtype([("status", "<i4"), ("n1", "<i4"), ("n", "<i4"), ("max_its", "<i4"),
                        ("iterations", "<i4"), ("best_inliers", "<i4"),
                        ("best_iteration", "<i4"), ("min_inliers", "<i4"), ("fix_scale", "<i4"),
                        ("best_scale", "<f4"), ("best_R", "<f4", 9), ("best_t", "<f4", 3),
                        ("best_T12", "<f4", 16), ("k1", "<f4", 4), ("k2", "<f4", 4)])
RESULT_DTYPE = np.dtype([("has_sim3", "<i4"), ("no_more", "<i4"), ("n_inliers", "<i4"),
                         ("iterations_run", "<i4"), ("T12", "<f4", 16), ("R", "<f4", 9),
                         ("t", "<f4", 3), ("scale", "<f4")])
assert CORR_DTYPE.itemsize == 56 and STATE_DTYPE.itemsize == 184 and RESULT_DTYPE.itemsize == 132
