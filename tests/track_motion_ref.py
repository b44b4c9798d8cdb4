"""numpy float32 restatement of what surrounds SearchByProjection(CurrentFrame,
LastFrame) in Tracking::TrackWithMotionModel (test infrastructure, CPU only).

The matcher itself stays with the C++ oracle (oracle.match_projection_frame,
one call per problem, a second for a retry); this module builds the
orb_last_mp_t records that call needs from poses and world points, and
restates the loops around it, each as the reference writes it:

  project / tlc      src/ORBmatcher.cc:1472-1505
  forward_backward   src/ORBmatcher.cc:1482-1484
  with_retry         src/Tracking.cc:1044-1052
  discard_outliers   src/Tracking.cc:1060-1083
  mark_seen          src/Tracking.cc:1333-1354 (Tracking::SearchLocalPoints' first loop)

Every float operation is a single float32 operation in the order the reference
(cv::Mat float products: ((r0 x + r1 y) + r2 z), then + t) evaluates it.
"""
import numpy as np

f32 = np.float32

KEYPOINT_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
     ("octave", "<i4"), ("class_id", "<i4")])
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"),
                            ("max_distance", "<f4"), ("bad", "u1"), ("seen", "u1"),
                            ("has_obs", "u1"), ("_pad", "u1")])
POSE_DTYPE = np.dtype([("rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("ow", "<f4", (3,))])
LAST_MP_DTYPE = np.dtype([("xc", "<f4"), ("yc", "<f4"), ("invzc", "<f4"), ("last_octave", "<i4"),
                          ("last_angle", "<f4"), ("valid", "u1"), ("has_obs", "u1"),
                          ("_pad", "u1", 2), ("mp_id", "<i4")])
INFO_DTYPE = np.dtype([("n_matches", "<i4"), ("n_matches_first_pass", "<i4"), ("retried", "<i4"),
                       ("forward", "<i4"), ("backward", "<i4")])
DISCARD_DTYPE = np.dtype([("n_matches", "<i4"), ("n_matches_map", "<i4"), ("n_discarded", "<i4")])


def pose(R=None, t=None, ow=None):
    """A POSE_DTYPE record; ow is left as given (the matcher never reads it)."""
    rec = np.zeros(1, POSE_DTYPE)
    rec["rcw"] = (np.eye(3) if R is None else np.asarray(R)).astype(f32).reshape(1, 9)
    rec["tcw"] = (np.zeros(3) if t is None else np.asarray(t)).astype(f32).reshape(1, 3)
    rec["ow"] = (np.full(3, np.nan) if ow is None else np.asarray(ow)).astype(f32).reshape(1, 3)
    return rec


def _rt(p):
    p = np.asarray(p, POSE_DTYPE).reshape(-1)[0]
    return p["rcw"].astype(f32).reshape(3, 3), p["tcw"].astype(f32)


def _row(R, r, x, y, z, t):
    """((r0 x + r1 y) + r2 z) + t in float32."""
    return f32(f32(f32(f32(R[r, 0] * x) + f32(R[r, 1] * y)) + f32(R[r, 2] * z)) + t)


def twc(pose_cur):
    """twc = -Rcw.t() * tcw (src/ORBmatcher.cc:1475), as Frame::UpdatePoseMatrices' mOw."""
    R, t = _rt(pose_cur)
    out = np.zeros(3, f32)
    for i in range(3):
        out[i] = -f32(f32(f32(R[0, i] * t[0]) + f32(R[1, i] * t[1])) + f32(R[2, i] * t[2]))
    return out


def tlc(pose_cur, pose_last):
    """tlc = Rlw * twc + tlw (src/ORBmatcher.cc:1477-1480)."""
    c = twc(pose_cur)
    Rl, tl = _rt(pose_last)
    return np.array([_row(Rl, r, c[0], c[1], c[2], tl[r]) for r in range(3)], f32)


def forward_backward(pose_cur, pose_last, mb, mono):
    """(bForward, bBackward), both strict (src/ORBmatcher.cc:1482-1484)."""
    z = tlc(pose_cur, pose_last)[2]
    return bool(z > f32(mb) and not mono), bool(-z > f32(mb) and not mono)


def project(pose_cur, pos):
    """x3Dc = Rcw * x3Dw + tcw; (xc, yc, invzc) with invzc = 1.0 / z narrowed to
    float (src/ORBmatcher.cc:1500-1505)."""
    R, t = _rt(pose_cur)
    x, y, z = (f32(v) for v in pos)
    xc, yc, zc = (_row(R, r, x, y, z, t[r]) for r in range(3))
    with np.errstate(divide="ignore"):
        invzc = f32(np.float64(1.0) / np.float64(zc))  # the reference's double division
        assert invzc.tobytes() == f32(f32(1.0) / zc).tobytes() or np.isnan(invzc)
    return xc, yc, invzc


def last_records(pose_cur, last_keys, last_point_index, last_outlier, points, mp_desc):
    """The orb_last_mp_t records and descriptors of SearchByProjection(F, LastF)
    for a last frame given as keypoints, map-point indices (negative = NULL) and
    outlier flags (None = none): valid = pMP && !mvbOutlier[i], mp_id = the
    point's index (so the oracle's kp_match holds indices)."""
    n = len(last_keys)
    idx = np.asarray(last_point_index, np.int32)
    pts = np.asarray(points, MAP_POINT_DTYPE)
    mp_desc = np.asarray(mp_desc, np.uint8).reshape(-1, 32)
    last = np.zeros(n, LAST_MP_DTYPE)
    desc = np.zeros((n, 32), np.uint8)
    for i in range(n):
        last[i]["last_octave"] = last_keys[i]["octave"]
        last[i]["last_angle"] = last_keys[i]["angle"]
        last[i]["mp_id"] = -1
        if idx[i] < 0:                                            # if(pMP)
            continue
        if last_outlier is not None and last_outlier[i]:          # if(!mvbOutlier[i])
            continue
        mp = pts[idx[i]]
        xc, yc, invzc = project(pose_cur, mp["pos"])
        last[i]["xc"], last[i]["yc"], last[i]["invzc"] = xc, yc, invzc
        last[i]["valid"] = 1
        last[i]["has_obs"] = 1 if mp["has_obs"] else 0
        last[i]["mp_id"] = idx[i]
        desc[i] = mp_desc[idx[i]]
    return last, desc


def with_retry(match, th, retry_below):
    """Tracking's retry (src/Tracking.cc:1044-1052): match(th) -> (nmatches,
    kp_match); fewer than retry_below matches (retry_below > 0) reruns from
    cleared outputs with 2 * th.  Returns (kp_match, n_matches, n_first, retried)."""
    n, km = match(f32(th))
    first = n
    retried = 0
    if retry_below > 0 and n < retry_below:
        n, km = match(f32(f32(2.0) * f32(th)))
        retried = 1
    return km, n, first, retried


def search(o, prob, cam, scale, width, height, th, mono, check_ori, retry_below):
    """One problem of the batch on the CPU: (kp_match, INFO_DTYPE record).  prob:
    keys, desc, u_right (None), locked (None), pose_cur, pose_last, last_keys,
    last_point_index, last_outlier (None), points, mp_desc."""
    last, last_desc = last_records(prob["pose_cur"], prob["last_keys"], prob["last_point_index"],
                                   prob.get("last_outlier"), prob["points"], prob["mp_desc"])
    z = float(tlc(prob["pose_cur"], prob["pose_last"])[2])
    fwd, bwd = forward_backward(prob["pose_cur"], prob["pose_last"], cam[5], mono)
    keys = np.asarray(prob["keys"], KEYPOINT_DTYPE)

    def match(t):
        if len(keys) == 0:
            return 0, np.zeros(0, np.int32)
        return o.match_projection_frame(keys, prob["desc"], scale, width, height, last, last_desc,
                                        cam, z, float(t), int(mono), int(check_ori),
                                        prob.get("locked"), prob.get("u_right"))

    km, n, first, retried = with_retry(match, th, retry_below)
    info = np.zeros(1, INFO_DTYPE)[0]
    info["n_matches"], info["n_matches_first_pass"], info["retried"] = n, first, retried
    info["forward"], info["backward"] = fwd, bwd
    return np.asarray(km, np.int32), info


def discard_outliers(kp_match, outlier, points, n_matches, mark_seen):
    """src/Tracking.cc:1060-1083, then (mark_seen) :1333-1354, on copies:
    (kp_match, outlier, points, DISCARD_DTYPE record)."""
    km = np.array(kp_match, np.int32, copy=True)
    ol = np.array(outlier, np.uint8, copy=True)
    pts = np.array(points, MAP_POINT_DTYPE, copy=True)
    nmatches, nmatches_map, ndisc = int(n_matches), 0, 0
    for i in range(len(km)):
        if km[i] >= 0:                       # if(mCurrentFrame.mvpMapPoints[i])
            if ol[i]:                        # if(mCurrentFrame.mvbOutlier[i])
                p = km[i]
                km[i] = -1                   # mvpMapPoints[i] = NULL
                ol[i] = 0                    # mvbOutlier[i] = false
                if mark_seen:
                    pts[p]["seen"] = 1       # pMP->mnLastFrameSeen = mCurrentFrame.mnId
                nmatches -= 1
                ndisc += 1
            elif pts[km[i]]["has_obs"]:      # Observations() > 0
                nmatches_map += 1
    if mark_seen:
        for i in range(len(km)):             # SearchLocalPoints' first loop
            if km[i] >= 0:
                if pts[km[i]]["bad"]:
                    km[i] = -1               # *vit = NULL
                else:
                    pts[km[i]]["seen"] = 1   # mnLastFrameSeen = mCurrentFrame.mnId
    out = np.zeros(1, DISCARD_DTYPE)[0]
    out["n_matches"], out["n_matches_map"], out["n_discarded"] = nmatches, nmatches_map, ndisc
    return km, ol, pts, out


# ------------------------------------------------------------ problem builders
def keys_from_last(last):
    """Last-frame keypoints carrying the octave and angle of orb_last_mp_t records."""
    k = np.zeros(len(last), KEYPOINT_DTYPE)
    k["octave"], k["angle"] = last["last_octave"], last["last_angle"]
    k["class_id"] = -1
    return k


def problem_from_records(keys, desc, last, last_desc, tlc_z, locked=None, u_right=None):
    """The batch entry's inputs for a problem stated as orb_last_mp_t records at
    the identity current pose: point i sits at (xc, yc, 1 / invzc), which the
    identity projects back to the records bit for bit when 1 / invzc is exact
    (asserted by the CPU tests for every generator used); the last pose is the
    identity rotation with tlw = (0, 0, tlc_z), so tlc = tlw."""
    last = np.asarray(last, LAST_MP_DTYPE)
    n = len(last)
    pts = np.zeros(max(n, 1), MAP_POINT_DTYPE)
    with np.errstate(divide="ignore"):
        z = (f32(1.0) / last["invzc"]).astype(f32)
    z[~last["valid"].astype(bool)] = 1.0
    pts["pos"][:n, 0], pts["pos"][:n, 1], pts["pos"][:n, 2] = last["xc"], last["yc"], z
    pts["has_obs"][:n] = last["has_obs"]
    idx = np.where(last["valid"] != 0, np.arange(n), -1).astype(np.int32)
    mp_desc = np.zeros((max(n, 1), 32), np.uint8)
    mp_desc[:n] = np.asarray(last_desc, np.uint8).reshape(-1, 32)
    return dict(keys=np.asarray(keys, KEYPOINT_DTYPE), desc=np.asarray(desc, np.uint8).reshape(-1, 32),
                u_right=u_right, locked=locked, pose_cur=pose(), pose_last=pose(t=(0, 0, tlc_z)),
                last_keys=keys_from_last(last), last_point_index=idx, last_outlier=None,
                points=pts, mp_desc=mp_desc)
