"""LocalMapping::CreateNewMapPoints' gate and loop body, KeyFrame::
ComputeSceneMedianDepth and the new point's MapPoint::UpdateNormalAndDepth
restated in Python (test infrastructure): the parity target of k_median_depth
and k_new_points.

Scalars are Python floats (IEEE doubles) or np.float32 exactly where the
reference has double or float; every widening is float(x), every narrowing
f32(x); every sum is explicit and ordered; np.dot, @ and np.linalg are never
used.  File:line citations are the reference's (src/LocalMapping.cc unless
named).

Pins (the same list stands in include/orb_abi.h and DESIGN.md 4.10; all
unpinned against a real OpenCV).  Float expressions as written, no
contraction; P-numbers are the Sim3 solver's pins (tests/sim3_ref.py).
 N1  Mat::dot of two 3-vectors (P11 below four elements): ((0 + p0) + p1) +
     p2 with exact double products; row.dot(x) + t adds the float t widened,
     in double, and narrows once: z of the median, x1 y1 z1 x2 y2 z2.
 N2  xn = ((u - cx) * invfx, (v - cy) * invfy, 1); ray = Rwc * xn as 3 x 3 by
     3 x 1 float products summed left to right: (rcw[i] x + rcw[3 + i] y) +
     rcw[6 + i] * 1.0f.
 N3  cv::norm (P8): the sqrt of a double sum, returned as a double.
     cosParallaxRays = (float)(dot / (norm1 * norm2)), all in double (N1).
 N4  cos(2 * atan2(mb / 2, depth)) on floats: a = (float)pinned_atan2 of the
     widened mb / 2.0f and depth; (float) of pinned_sincos_d's cosine of the
     widened 2.0f * a.  profiles/newpoints_libm.json counts how often glibc's
     atan2f / cosf differ.
 N5  A.row(r) = xn * T.row(2) - T.row(r) (addWeighted, beta = -1, gamma = 0):
     (xn * T2k + Trk * -1.0f) + 0.0f per element, in float.
 N6  cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) on 4 x 4 float: OpenCV
     3.x JacobiSVDImpl_<float> on At (row i of At = column i of A).  W[i] = the
     double sum of squares of row i, k ascending from 0; Vt = I.  At most
     max(m, 30) = 30 sweeps over the pairs i < j in order; p = the double dot
     of rows i and j; the pair is skipped when |p| <= eps * sqrt(a * b), eps =
     (double)(2 * FLT_EPSILON), a = W[i], b = W[j]; p *= 2; beta = a - b;
     gamma = hypot(p, beta) = sqrt(p * p + beta * beta) in double (P7's
     hypot, not narrowed); beta < 0: s = (float)sqrt(((gamma - beta) * 0.5) /
     gamma), c = (float)(p / ((gamma * s) * 2)); otherwise c =
     (float)sqrt((gamma + beta) / (gamma * 2)), s = (float)(p / ((gamma * c) *
     2)); both rows of At and of Vt rotate in float: t0 = c * x + s * y, t1 =
     (-s) * x + c * y; a and b are re-summed in double from the rotated rows;
     the loop stops after a sweep without a rotation; W[i] = sqrt of the
     re-summed squares; selection sort, descending: swap with the first later
     maximum under strict <, the rows of Vt moving along.  Only vt.row(3) is
     used; U's normalisation is not reproduced.
 N7  x3D = v[0..2] / v[3] is Mat / double scalar, P2's statement: v * (float)
     (1.0 / (double)v3) + 0.0f (adopted, as cvtScale_ evaluates it); one
     correctly rounded float divide per element is the rejected alternative.
     normali / cv::norm(normali) likewise: v * (float)(1.0 / norm) + 0.0f;
     normal / n with n = 2: v * (float)(1.0 / 2.0) + 0.0f.
 N8  UnprojectStereo: the statement of orb_unproject_stereo.
 N9  double constants: (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2,
     the three-term float sum (ex ex + ey ey) + er er against 7.8 *
     (double)sigma2; invz = (float)(1.0 / (double)z); cosParallaxRays <
     0.9998 and baseline / median < 0.01 compared in double; u = (fx * x) *
     invz + cx, u_r = u - mbf * invz in float; cosParallaxRays + 1 in float.
 N10 dist = (float)cv::norm(x3D - Ow) (N3); ratioDist = dist2 / dist1,
     ratioOctave = sf[o1] / sf[o2], ratioFactor = 1.5f * sf[1], max_distance =
     dist1 * sf[o1], min_distance = max_distance / sf[n_levels - 1]: float.
libm=True uses glibc's atan2f / cosf for N4 and math.hypot for N6's gamma.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import math
import struct

import numpy as np

from poseopt_ref import pinned_sincos_d
from sim3_ref import pinned_atan2

f32 = np.float32
FLT_EPSILON = f32(1.1920928955078125e-07)

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"),
                            ("max_distance", "<f4"), ("bad", "u1"), ("seen", "u1"),
                            ("has_obs", "u1"), ("_pad", "u1")])
POSE_DTYPE = np.dtype([("rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("ow", "<f4", (3,))])
NEW_POINT_INFO_DTYPE = np.dtype([("gated", "<i4"), ("overflow", "<i4"), ("n_new", "<i4"),
                                 ("first_point", "<i4"), ("counts", "<i4", (12,))])
assert NEW_POINT_INFO_DTYPE.itemsize == 64 and MAP_POINT_DTYPE.itemsize == 36

(NOT_TRIED, NO_MATCH, ACCEPTED, LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST,
 SCALE_RATIO, UNDEFINED) = range(12)
NSTATUS = 12
STATUS_NAMES = ("not_tried", "no_match", "accepted", "low_parallax", "w_zero", "z1", "z2",
                "reproj1", "reproj2", "zero_dist", "scale_ratio", "undefined")
HAS_X3D = (ACCEPTED, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST, SCALE_RATIO)

# rule switches (tests/test_newpoints_ref.py): each replaces one reference rule
# by a plausible wrong one
# (0.9998, 0.01, 5.991 * sigma2 and 7.8 * sigma2 are not floats: < and <= agree
# there, so those gates are switched to the float comparison instead, or not at all)
SWITCHES = ("gate_stereo_le", "gate_mono_float", "no_else_if", "kf2_own_bf", "sort_nonstrict",
            "eps_single", "sweep_cap_2", "descending_order", "z1_lt", "z2_lt", "rays_le",
            "rays_ge0", "ratio_le")


def _libm():
    L = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for name, n in (("atan2f", 2), ("cosf", 1)):
        fn = getattr(L, name)
        fn.restype = ctypes.c_float
        fn.argtypes = [ctypes.c_float] * n
    return L


_LIBM = None


def f32_bits(x) -> int:
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def f32_from_bits(b: int):
    return f32(struct.unpack("<f", struct.pack("<I", b & 0xFFFFFFFF))[0])


def f32_next(x, up=True):
    """The adjacent float32 above (below) x, by bit pattern."""
    return np.nextafter(f32(x), f32(np.inf) if up else f32(-np.inf), dtype=f32)


def _div(a: float, b: float) -> float:
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(x: float) -> float:
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(x)))


def dot3(a, b) -> float:
    """N1: Mat::dot of two float 3-vectors, in double."""
    return ((0.0 + float(a[0]) * float(b[0])) + float(a[1]) * float(b[1])) + float(a[2]) * float(b[2])


def row_dot(r, t, x):
    """N1: Rcw.row(k).dot(x3Dt) + tcw.at<float>(k), narrowed once."""
    return f32(dot3(r, x) + float(t))


def norm3(v) -> float:
    """N3: cv::norm of a float 3-vector (a double)."""
    return _sqrt(dot3(v, v))


def cos_stereo(mb, depth, libm=False):
    """N4: cos(2*atan2(mb/2, depth)) (:371, :373)."""
    global _LIBM
    half = f32(mb) / f32(2.0)
    if libm:
        if _LIBM is None:
            _LIBM = _libm()
        a = f32(_LIBM.atan2f(float(half), float(f32(depth))))
        return f32(_LIBM.cosf(float(f32(2.0) * a)))
    a = f32(pinned_atan2(float(half), float(f32(depth))))
    return f32(pinned_sincos_d(float(f32(2.0) * a))[1])


# ------------------------------------------------------------------- N6
def svd_vt(A, libm=False, sw=frozenset(), trace=None):
    """cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) on a 4 x 4 float A
    (:391): returns (W (4 doubles, descending), Vt (4 x 4 float32), sweeps).
    trace (a dict) receives 'beta_neg', 'beta_pos', 'skipped' (pairs under the
    epsilon), 'ties' (equal singular values met by the sort), 'rotations'."""
    n = 4
    At = [[f32(A[k][i]) for k in range(n)] for i in range(n)]  # row i of At = column i of A
    Vt = [[f32(1) if i == j else f32(0) for j in range(n)] for i in range(n)]
    tr = trace if trace is not None else {}
    for key in ("beta_neg", "beta_pos", "skipped", "ties", "rotations"):
        tr.setdefault(key, 0)

    def sumsq(row):
        sd = 0.0
        for k in range(n):
            sd += float(row[k]) * float(row[k])
        return sd

    W = [sumsq(At[i]) for i in range(n)]
    eps = float(FLT_EPSILON) if "eps_single" in sw else float(f32(2) * FLT_EPSILON)
    max_iter = 2 if "sweep_cap_2" in sw else 30
    sweeps = 0
    with np.errstate(all="ignore"):
        for _ in range(max_iter):
            changed = False
            sweeps += 1
            for i in range(n - 1):
                for j in range(i + 1, n):
                    Ai, Aj = At[i], At[j]
                    a, b = W[i], W[j]
                    p = 0.0
                    for k in range(n):
                        p += float(Ai[k]) * float(Aj[k])
                    if abs(p) <= eps * _sqrt(a * b):
                        tr["skipped"] += 1
                        continue
                    p *= 2.0
                    beta = a - b
                    gamma = math.hypot(p, beta) if libm else _sqrt(p * p + beta * beta)
                    if beta < 0:
                        tr["beta_neg"] += 1
                        delta = (gamma - beta) * 0.5
                        s = f32(_sqrt(_div(delta, gamma)))
                        c = f32(_div(p, (gamma * float(s)) * 2.0))
                    else:
                        tr["beta_pos"] += 1
                        c = f32(_sqrt(_div(gamma + beta, gamma * 2.0)))
                        s = f32(_div(p, (gamma * float(c)) * 2.0))
                    ms = -s
                    na = nb = 0.0
                    for k in range(n):
                        t0 = c * Ai[k] + s * Aj[k]
                        t1 = ms * Ai[k] + c * Aj[k]
                        Ai[k], Aj[k] = t0, t1
                        na += float(t0) * float(t0)
                        nb += float(t1) * float(t1)
                    W[i], W[j] = na, nb
                    changed = True
                    tr["rotations"] += 1
                    Vi, Vj = Vt[i], Vt[j]
                    for k in range(n):
                        t0 = c * Vi[k] + s * Vj[k]
                        t1 = ms * Vi[k] + c * Vj[k]
                        Vi[k], Vj[k] = t0, t1
            if not changed:
                break
    W = [_sqrt(sumsq(At[i])) for i in range(n)]
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] == W[k]:
                tr["ties"] += 1
            if (W[j] <= W[k]) if "sort_nonstrict" in sw else (W[j] < W[k]):
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            Vt[i], Vt[j] = Vt[j], Vt[i]
    return W, Vt, sweeps


# ------------------------------------------------- KeyFrame.cc:658-694
def depth_key(z) -> int:
    """The total order of float bit patterns the device sorts by (-0 before +0)."""
    b = f32_bits(z)
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)


def scene_median_depth(point_index, pose, points_pos, q=2):
    """KeyFrame::ComputeSceneMedianDepth(q): (median float32 or NaN, count)."""
    rcw, tcw = pose["rcw"], pose["tcw"]
    depths = []
    for idx in point_index:
        if idx >= 0:  # :680
            depths.append(row_dot(rcw[6:9], tcw[2], points_pos[idx]))  # :685 (N1)
    if not depths:
        return f32(np.nan), 0
    depths.sort(key=depth_key)  # :691
    return depths[(len(depths) - 1) // q], len(depths)  # :693


# ------------------------------------------------------- the loop body
def unproject_stereo(kp, depth, pose, cam):
    """KeyFrame::UnprojectStereo (src/KeyFrame.cc:640-656; N8)."""
    fx, fy, cx, cy = (f32(v) for v in cam[:4])
    invfx, invfy = f32(1.0) / fx, f32(1.0) / fy
    z = f32(depth)
    x = (f32(kp["x"]) - cx) * z * invfx
    y = (f32(kp["y"]) - cy) * z * invfy
    r, ow = pose["rcw"], pose["ow"]
    return [((r[i] * x + r[3 + i] * y) + r[6 + i] * z) + ow[i] for i in range(3)]


def triangulate_match(kp1, ur1, d1, kp2, ur2, d2, pose1, pose2, cam1, cam2, sf, sig, libm=False,
                      sw=frozenset(), trace=None, svd=None):
    """One iteration of the loop (:341-512): (status, x3D or None).  trace (a
    dict) receives 'branch' ('tri', 'st1', 'st2'), the SVD trace and the
    deciding quantities.  svd replaces svd_vt (a test reaches :395 directly)."""
    tr = trace if trace is not None else {}
    n_levels = len(sf)
    o1, o2 = int(kp1["octave"]), int(kp2["octave"])
    if not (0 <= o1 < n_levels and 0 <= o2 < n_levels):
        return UNDEFINED, None
    ur1, ur2 = f32(ur1), f32(ur2)
    st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)  # :350, :354
    d1, d2 = f32(d1), f32(d2)
    if (st1 and not d1 > 0) or (st2 and not d2 > 0):
        return UNDEFINED, None
    fx1, fy1, cx1, cy1, bf1, mb1 = (f32(v) for v in cam1)
    fx2, fy2, cx2, cy2, bf2, mb2 = (f32(v) for v in cam2)
    invfx1, invfy1, invfx2, invfy2 = f32(1) / fx1, f32(1) / fy1, f32(1) / fx2, f32(1) / fy2
    R1, t1, ow1 = pose1["rcw"], pose1["tcw"], pose1["ow"]
    R2, t2, ow2 = pose2["rcw"], pose2["tcw"], pose2["ow"]
    u1, v1, u2, v2 = f32(kp1["x"]), f32(kp1["y"]), f32(kp2["x"]), f32(kp2["y"])
    with np.errstate(all="ignore"):
        # :358-364 (N2, N3)
        xn1 = ((u1 - cx1) * invfx1, (v1 - cy1) * invfy1)
        xn2 = ((u2 - cx2) * invfx2, (v2 - cy2) * invfy2)
        ray1 = [(R1[i] * xn1[0] + R1[3 + i] * xn1[1]) + R1[6 + i] * f32(1) for i in range(3)]
        ray2 = [(R2[i] * xn2[0] + R2[3 + i] * xn2[1]) + R2[6 + i] * f32(1) for i in range(3)]
        cos_rays = f32(_div(dot3(ray1, ray2), norm3(ray1) * norm3(ray2)))
        # :366-375 (N4)
        cs = cos_rays + f32(1)
        cs1 = cs2 = cs
        if st1:
            cs1 = cos_stereo(mb1, d1, libm)
            if "no_else_if" in sw and st2:
                cs2 = cos_stereo(mb2, d2, libm)
        elif st2:
            cs2 = cos_stereo(mb2, d2, libm)
        cs = cs2 if cs2 < cs1 else cs1  # std::min
        tr.update(cos_rays=cos_rays, cos_stereo=cs, cos_stereo1=cs1, cos_stereo2=cs2)
        below = (cos_rays <= cs) if "rays_le" in sw else (cos_rays < cs)
        positive = (cos_rays >= 0) if "rays_ge0" in sw else (cos_rays > 0)
        lowpar = float(cos_rays) < 0.9998
        if below and positive and (st1 or st2 or lowpar):  # :380
            tr["branch"] = "tri"
            T1 = [[R1[0], R1[1], R1[2], t1[0]], [R1[3], R1[4], R1[5], t1[1]],
                  [R1[6], R1[7], R1[8], t1[2]]]
            T2 = [[R2[0], R2[1], R2[2], t2[0]], [R2[3], R2[4], R2[5], t2[1]],
                  [R2[6], R2[7], R2[8], t2[2]]]
            A = [[(xn * T[2][k] + T[r][k] * f32(-1)) + f32(0) for k in range(4)]  # :384-387 (N5)
                 for xn, T, r in ((xn1[0], T1, 0), (xn1[1], T1, 1), (xn2[0], T2, 0),
                                  (xn2[1], T2, 1))]
            tr["A"] = A
            W, Vt, sweeps = (svd or svd_vt)(A, libm, sw, tr)  # :391
            tr.update(W=W, Vt=Vt, sweeps=sweeps)
            v = Vt[3]
            if v[3] == 0:  # :395
                return W_ZERO, None
            inv = f32(_div(1.0, float(v[3])))  # :399 (N7)
            x3d = [v[k] * inv + f32(0) for k in range(3)]
        elif st1 and cs1 < cs2:  # :403
            tr["branch"] = "st1"
            x3d = unproject_stereo(kp1, d1, pose1, cam1)
        elif st2 and cs2 < cs1:  # :408
            tr["branch"] = "st2"
            x3d = unproject_stereo(kp2, d2, pose2, cam2)
        else:
            return LOW_PARALLAX, None  # :414
        # :420-426
        z1 = row_dot(R1[6:9], t1[2], x3d)
        tr["z1"] = z1
        if (z1 < 0) if "z1_lt" in sw else (z1 <= 0):
            return Z1, x3d
        z2 = row_dot(R2[6:9], t2[2], x3d)
        tr["z2"] = z2
        if (z2 < 0) if "z2_lt" in sw else (z2 <= 0):
            return Z2, x3d

        def reproj(R, t, z, fx, fy, cx, cy, u, v, st, ur, bf, sigma2):
            x = row_dot(R[0:3], t[0], x3d)
            y = row_dot(R[3:6], t[1], x3d)
            invz = f32(_div(1.0, float(z)))
            pu = fx * x * invz + cx
            pv = fy * y * invz + cy
            ex, ey = pu - u, pv - v
            if not st:
                err, th = ex * ex + ey * ey, 5.991 * float(sigma2)
            else:
                er = (pu - bf * invz) - ur
                err, th = ex * ex + ey * ey + er * er, 7.8 * float(sigma2)
            return err, th, float(err) > th

        # :431-460
        err, th, out = reproj(R1, t1, z1, fx1, fy1, cx1, cy1, u1, v1, st1, ur1, bf1, sig[o1])
        tr.update(err1=err, th1=th)
        if out:
            return REPROJ1, x3d
        # :464-487: mpCurrentKeyFrame->mbf (:480)
        err, th, out = reproj(R2, t2, z2, fx2, fy2, cx2, cy2, u2, v2, st2, ur2,
                              bf2 if "kf2_own_bf" in sw else bf1, sig[o2])
        tr.update(err2=err, th2=th)
        if out:
            return REPROJ2, x3d
        # :492-512 (N10)
        dist1 = f32(norm3([x3d[i] - ow1[i] for i in range(3)]))
        dist2 = f32(norm3([x3d[i] - ow2[i] for i in range(3)]))
        if dist1 == 0 or dist2 == 0:
            return ZERO_DIST, x3d
        ratio_dist = dist2 / dist1
        ratio_octave = f32(sf[o1]) / f32(sf[o2])
        ratio_factor = f32(1.5) * f32(sf[1])  # :275
        tr.update(ratio_dist=ratio_dist, ratio_octave=ratio_octave, ratio_factor=ratio_factor)
        if "ratio_le" in sw:
            bad = ratio_dist * ratio_factor <= ratio_octave or ratio_dist >= ratio_octave * ratio_factor
        else:
            bad = ratio_dist * ratio_factor < ratio_octave or ratio_dist > ratio_octave * ratio_factor
        if bad:
            return SCALE_RATIO, x3d
    return ACCEPTED, x3d


def new_point_record(x3d, pose1, pose2, o1, sf):
    """MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:349-402) for the
    observations {KF1, KF2}, reference keyframe KF1 (N7, N10)."""
    rec = np.zeros(1, MAP_POINT_DTYPE)[0]
    with np.errstate(all="ignore"):
        a = [x3d[i] - pose1["ow"][i] for i in range(3)]
        b = [x3d[i] - pose2["ow"][i] for i in range(3)]
        na, nb = norm3(a), norm3(b)
        ia, ib = f32(_div(1.0, na)), f32(_div(1.0, nb))
        half = f32(1.0 / 2.0)
        normal = [((f32(0) + (a[i] * ia + f32(0))) + (b[i] * ib + f32(0))) * half + f32(0)
                  for i in range(3)]
        max_d = f32(na) * f32(sf[o1])
        min_d = max_d / f32(sf[len(sf) - 1])
    rec["pos"], rec["normal"] = x3d, normal
    rec["min_distance"], rec["max_distance"] = min_d, max_d
    rec["has_obs"] = 1
    return rec


def gate(pose1, pose2, cam2, monocular, median, sw=frozenset()):
    """:289-311: True when the pair is skipped."""
    with np.errstate(all="ignore"):
        baseline = f32(norm3([pose2["ow"][i] - pose1["ow"][i] for i in range(3)]))  # :293-295
        if not monocular:
            mb2 = f32(cam2[5])
            return bool(baseline <= mb2) if "gate_stereo_le" in sw else bool(baseline < mb2)
        median = f32(median)
        if median != median:
            return True
        ratio = baseline / median
        return bool(ratio < f32(0.01)) if "gate_mono_float" in sw else float(ratio) < 0.01  # :309


def create_new_map_points(kf1, kf2, match12, median, cam1, cam2, sf, sig, monocular, points,
                          cursor, status, x3d, pairs, libm=False, sw=frozenset(), traces=None):
    """The gate and body for one (KF1, KF2) pair.  kf: dict(keys, u_right, depth
    (both None: monocular keyframe), point_index, pose).  Updates, in place and
    as the device does: both point_index arrays, points (len = point_capacity),
    status (n1 bytes), x3d (n1 x 3), pairs (n1 x 2).  Returns (info record, the
    cursor after the call)."""
    info = np.zeros(1, NEW_POINT_INFO_DTYPE)[0]
    n1, n2 = len(kf1["keys"]), len(kf2["keys"])
    if gate(kf1["pose"], kf2["pose"], cam2, monocular, median, sw):
        info["gated"], info["first_point"] = 1, cursor
        status[:n1] = NOT_TRIED
        return info, cursor
    res = []
    for i1 in range(n1):
        idx2 = int(match12[i1])
        if idx2 < 0:
            res.append((NO_MATCH, None))
            continue
        if idx2 >= n2:
            res.append((UNDEFINED, None))
            continue
        tr = {} if traces is not None else None
        ur1 = kf1["u_right"][i1] if kf1["u_right"] is not None else -1.0
        d1 = kf1["depth"][i1] if kf1["depth"] is not None else -1.0
        ur2 = kf2["u_right"][idx2] if kf2["u_right"] is not None else -1.0
        d2 = kf2["depth"][idx2] if kf2["depth"] is not None else -1.0
        res.append(triangulate_match(kf1["keys"][i1], ur1, d1, kf2["keys"][idx2], ur2, d2,
                                     kf1["pose"], kf2["pose"], cam1, cam2, sf, sig, libm, sw, tr))
        if traces is not None:
            tr["i1"], tr["status"] = i1, res[-1][0]
            traces.append(tr)
    n_new = sum(1 for s, _ in res if s == ACCEPTED)
    if cursor < 0 or cursor + n_new > len(points):
        info["overflow"] = 1
        return info, cursor
    order = range(n1 - 1, -1, -1) if "descending_order" in sw else range(n1)
    k = 0
    for i1 in order:
        s, x = res[i1]
        status[i1] = s
        info["counts"][s] += 1
        if s in HAS_X3D:
            x3d[i1] = x
        if s == ACCEPTED:  # :516-534
            idx2 = int(match12[i1])
            pid = cursor + k
            points[pid] = new_point_record(x, kf1["pose"], kf2["pose"],
                                           int(kf1["keys"][i1]["octave"]), sf)
            pairs[k] = (i1, idx2)
            kf1["point_index"][i1] = pid  # :522
            kf2["point_index"][idx2] = pid  # :524
            k += 1
    info["n_new"], info["first_point"] = n_new, cursor
    return info, cursor + n_new
