"""Reference side of the device-batched SearchForTriangulation
(orb_search_for_triangulation_batch): packs keyframe "sides" into the slot arrays
the entry reads (bow_batch_ref.pack_slots plus whole keypoints, mvuRight and the
poses), and derives what the entry must return for a (KF1 slot, KF2 slot, F12)
problem from those same arrays, read as its contract says: counts clamped,
FeatureVectors validated, has_mp from point_index, Cw / R2w / t2w from the pose
records, then the C++ oracle's search_for_triangulation.  No GPU.

A side is bow_batch_ref's (desc, angle, fv, pidx) plus keys (KEYPOINT_DTYPE),
u_right (n,) float32 and pose (one POSE_DTYPE record)."""
import numpy as np

import bow_batch_ref as B
import matcher_edge_cases as E
import scenarios as S

f32 = np.float32
KEYPOINT_DTYPE, POSE_DTYPE = B.KEYPOINT_DTYPE, E.POSE_DTYPE
INFO_DTYPE = np.dtype([("n_matches", "<i4"), ("n_accepted", "<i4"), ("n_common_nodes", "<i4"),
                       ("n_tried", "<i4"), ("n_shared2", "<i4"), ("n_undefined", "<i4")])
INFO_FIELDS = INFO_DTYPE.names
MALFORMED = (-1, 0, 0, 0, 0, 0)


def pose_rec(R=E.EYE, t=E.ZERO3, ow=None):
    rec = np.zeros(1, POSE_DTYPE)[0]
    R, t = np.asarray(R, f32).reshape(3, 3), np.asarray(t, f32)
    rec["rcw"], rec["tcw"] = R.reshape(9), t
    rec["ow"] = S._camera_center(R, t) if ow is None else np.asarray(ow, f32)
    return rec


def side(kf, fv, pose, pidx=None):
    """A keyframe dict of the oracle's form (keys, desc, u_right, has_mp) as a side;
    has_mp becomes a point index (any non-negative value says "has a point")."""
    keys = np.ascontiguousarray(kf["keys"], KEYPOINT_DTYPE)
    if pidx is None:
        pidx = np.where(np.asarray(kf["has_mp"]) != 0, 7 + np.arange(len(keys)), -1)
    s = B.side(kf["desc"], keys["angle"], fv, pidx)
    s.update(keys=keys, u_right=np.ascontiguousarray(kf["u_right"], f32), pose=pose)
    return s


def from_tri_case(c):
    """matcher_edge_cases.tri_case / hist_bow(form="kf"): (side1, side2, F12).  The
    case's Cw is KF1's centre, KF2's pose is the identity."""
    return (side(c["kf1"], c["fv1"], pose_rec(ow=c["Cw"])), side(c["kf2"], c["fv2"], pose_rec()),
            np.asarray(c["F12"], f32).reshape(9))


def from_keyframes(oracle, k1, k2, pidx1=None, pidx2=None):
    """A scenarios.keyframe_pair: natural FeatureVectors, F12 = scenarios.fundamental."""
    mk = lambda k, pidx: side(dict(k, has_mp=np.zeros(len(k["keys"]), np.uint8)),
                              oracle.feature_vector(S.vocab_nodes(k["desc"])),
                              pose_rec(k["Rw"], k["tw"], k["ow"]), pidx)
    n1, n2 = len(k1["keys"]), len(k2["keys"])
    return (mk(k1, np.full(n1, -1, np.int32) if pidx1 is None else pidx1),
            mk(k2, np.full(n2, -1, np.int32) if pidx2 is None else pidx2),
            S.fundamental(k1, k2).reshape(9))


def empty_side(pose=None):
    kf = dict(keys=np.zeros(0, KEYPOINT_DTYPE), desc=np.zeros((0, 32), np.uint8),
              u_right=np.zeros(0, f32), has_mp=np.zeros(0, np.uint8))
    return side(kf, B.empty_fv(), pose_rec() if pose is None else pose)


# ------------------------------------------------------------------- packing
def pack_slots(sides, stride, with_u_right=True):
    a = B.pack_slots(sides, stride)
    K = len(sides)
    a["u_right"] = np.full(K * stride, np.nan, f32) if with_u_right else None
    a["pose"] = np.zeros(K, POSE_DTYPE)
    a["keys"]["octave"] = 1 << 20     # junk past the counts
    for k, s in enumerate(sides):
        n, b = len(s["desc"]), k * stride
        a["keys"][b:b + n] = s["keys"]
        if with_u_right:
            a["u_right"][b:b + n] = s["u_right"]
        a["pose"][k] = s["pose"]
    return a


def unpack_side(a, k, stride):
    s, bad = B.unpack_side(a, k, stride)
    n, b = len(s["desc"]), k * stride
    s["keys"] = a["keys"][b:b + n]
    s["u_right"] = np.full(n, -1.0, f32) if a["u_right"] is None else a["u_right"][b:b + n]
    s["pose"] = a["pose"][k]
    return s, bad


# ----------------------------------------------------------------- reference
def _hamming(a, b):
    return int(np.unpackbits(a ^ b).sum())


def expected(oracle, s1, s2, f12, cam, scale, sigma2, only_stereo, check_ori, second=None):
    """(match12 over KF1's keypoints, info tuple) of one well-formed problem.
    second: a function with oracle.search_for_triangulation's signature that
    replaces it (the restatement in pyref)."""
    search = second or oracle.search_for_triangulation
    n_levels = len(scale)
    has1, has2 = s1["pidx"] >= 0, s2["pidx"] >= 0
    st1, st2 = s1["u_right"] >= 0, s2["u_right"] >= 0
    oct2 = s2["keys"]["octave"]
    undef2 = (oct2 < 0) | (oct2 >= n_levels)
    nodes1, offs1, feats1 = s1["fv"]
    nodes2, offs2, feats2 = s2["fv"]
    pos2 = {int(v): k for k, v in enumerate(nodes2)}
    common = [(a, pos2[int(v)]) for a, v in enumerate(nodes1) if int(v) in pos2]
    ok1 = ~has1 & (st1 | (not only_stereo))
    ok2 = ~has2 & (st2 | (not only_stereo))
    tried = undefined = 0
    for a, b in common:
        l1 = feats1[offs1[a]:offs1[a + 1]]
        l2 = feats2[offs2[b]:offs2[b + 1]]
        tried += int(ok1[l1].sum())
        u2 = [j for j in l2 if undef2[j] and ok2[j]]
        if u2:
            undefined += sum(_hamming(s1["desc"][i], s2["desc"][j]) <= 50
                             for i in l1 if ok1[i] for j in u2)
    # a candidate with an octave the tables do not have is skipped: for the
    # reference it is a keypoint that already has a point
    keys2 = s2["keys"].copy()
    keys2["octave"][undef2] = 0
    kf = lambda s, keys, has: dict(keys=keys, desc=s["desc"], scale=scale, width=E.W,
                                   height=E.H, u_right=s["u_right"], has_mp=has.astype(np.uint8))
    args = (kf(s1, s1["keys"], has1), kf(s2, keys2, has2 | undef2), sigma2, f12, cam,
            s1["pose"]["ow"], s2["pose"]["rcw"], s2["pose"]["tcw"],
            (nodes1, offs1, feats1), (nodes2, offs2, feats2), bool(only_stereo))
    n, m12 = search(*args, bool(check_ori))
    n_acc = search(*args, False)[0] if check_ori else n
    _, counts = np.unique(m12[m12 >= 0], return_counts=True)
    shared = int(counts[counts >= 2].sum())
    return m12, (int(n), int(n_acc), len(common), tried, shared, undefined)


def expected_slot(oracle, a, k1, k2, f12, stride, cam, scale, sigma2, only_stereo, check_ori,
                  second=None):
    """The same for slots k1, k2 of packed arrays, with the malformed-slot rule."""
    s1, bad1 = unpack_side(a, k1, stride)
    s2, bad2 = unpack_side(a, k2, stride)
    if bad1 or bad2:
        return np.full(len(s1["desc"]), -1, np.int32), MALFORMED
    return expected(oracle, s1, s2, f12, cam, scale, sigma2, only_stereo, check_ori, second)


def shared_count(m12):
    _, counts = np.unique(m12[m12 >= 0], return_counts=True)
    return int(counts[counts >= 2].sum())


def check(m12, info, p, n, want_row, want_info, sentinel, tag=""):
    got = tuple(int(info[p][f]) for f in INFO_FIELDS)
    bad = np.nonzero(m12[p, :n] != want_row)[0]
    assert len(bad) == 0, (tag, p, bad[:8], m12[p, :n][bad[:8]], want_row[bad[:8]])
    assert got == tuple(want_info), (tag, p, got, want_info)
    assert (m12[p, n:] == sentinel).all(), (tag, p, "slots past the count were written")
