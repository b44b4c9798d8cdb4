"""Reference side of the device-batched SearchByBoW(KF, F) (orb_match_bow_batch):
packs keyframe / frame "sides" into the slot arrays the entry reads, and derives
what the entry must return for a problem from those same arrays, read as its
contract says (counts clamped, FeatureVectors validated, then the C++ oracle's
match_bow per problem).  No GPU.

A side is a dict: desc (n, 32) uint8, angle (n,) float32, fv = (node ids
ascending, CSR offsets, feature indices); a keyframe side adds pidx (n,) int32,
the index of mvpMapPoints[i] in the problem's point array (negative: NULL).
A problem is dict(kf=side, f=side, points=MAP_POINT_DTYPE array or None)."""
import numpy as np

KEYPOINT_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
     ("octave", "<i4"), ("class_id", "<i4")])
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"),
                            ("max_distance", "<f4"), ("bad", "u1"), ("seen", "u1"),
                            ("has_obs", "u1"), ("_pad", "u1")])
INFO_DTYPE = np.dtype([("n_matches", "<i4"), ("n_accepted", "<i4"), ("n_common_nodes", "<i4"),
                       ("n_tried", "<i4"), ("enough", "<i4")])
INFO_FIELDS = INFO_DTYPE.names
MALFORMED = (-1, 0, 0, 0, 0)


# ------------------------------------------------------------------ problems
def side(desc, angle, fv, pidx=None):
    s = dict(desc=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32),
             angle=np.ascontiguousarray(angle, np.float32),
             fv=(np.ascontiguousarray(fv[0], np.uint32), np.ascontiguousarray(fv[1], np.int32),
                 np.ascontiguousarray(fv[2], np.uint32)))
    if pidx is not None:
        s["pidx"] = np.ascontiguousarray(pidx, np.int32)
    return s


def from_bow(c):
    """A scenarios.bow_pair / matcher_edge_cases.bow_case dict as a problem: the
    MapPoint ids are the point indices, the bad flags go to those records."""
    mp = np.asarray(c["kf_mp"], np.int32)
    pts = np.zeros(int(mp.max(initial=-1)) + 1, MAP_POINT_DTYPE)
    pts["pos"] = np.nan   # only `bad` may be read
    if c.get("kf_bad") is not None:
        pts["bad"][mp[mp >= 0]] = np.asarray(c["kf_bad"], np.uint8)[mp >= 0]
    return dict(kf=side(c["kf_desc"], c["kf_angle"], c["kf_fv"], mp),
                f=side(c["f_desc"], c["f_angle"], c["f_fv"]), points=pts)


def empty_fv():
    return (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32))


# ------------------------------------------------------------------- packing
def pack_slots(sides, stride):
    """Slot k of `sides` at k * stride (desc x 32, fv_offs at k * (stride + 1));
    everything past a slot's counts is junk that must not be read as data:
    NaN keypoints, 0xFFFFFFFF feature indices, offsets of -7."""
    K = len(sides)
    a = dict(keys=np.zeros(K * stride, KEYPOINT_DTYPE), desc=np.zeros((K * stride, 32), np.uint8),
             nkeys=np.zeros(K, np.int32), pidx=np.full(K * stride, -1, np.int32),
             fv_nodes=np.full(K * stride, 0xFFFFFFFF, np.uint32),
             fv_offs=np.full(K * (stride + 1), -7, np.int32),
             fv_feats=np.full(K * stride, 0xFFFFFFFF, np.uint32), n_fv_nodes=np.zeros(K, np.int32))
    for f in ("x", "y", "size", "angle", "response"):
        a["keys"][f] = np.nan
    a["desc"][:] = 0x5A
    for k, s in enumerate(sides):
        n, b = len(s["desc"]), k * stride
        nodes, offs, feats = s["fv"]
        assert n <= stride and len(nodes) <= stride and len(feats) <= stride
        a["keys"]["angle"][b:b + n] = s["angle"]
        a["desc"][b:b + n] = s["desc"]
        a["nkeys"][k] = n
        if "pidx" in s:
            a["pidx"][b:b + n] = s["pidx"]
        a["fv_nodes"][b:b + len(nodes)] = nodes
        a["fv_offs"][k * (stride + 1):k * (stride + 1) + len(offs)] = offs
        a["fv_feats"][b:b + len(feats)] = feats
        a["n_fv_nodes"][k] = len(nodes)
    return a


def pack_points(point_arrays, mp_stride=None):
    """Per-problem point arrays at p * mp_stride."""
    mp_stride = mp_stride or max(1, max(len(p) for p in point_arrays))
    pts = np.zeros(len(point_arrays) * mp_stride, MAP_POINT_DTYPE)
    pts["pos"] = np.nan
    for p, a in enumerate(point_arrays):
        pts[p * mp_stride:p * mp_stride + len(a)] = a
    return pts, mp_stride


def unpack_side(a, k, stride):
    """(side with the counts clamped as the entry clamps them, malformed?) of slot k."""
    n = int(min(max(int(a["nkeys"][k]), 0), stride))
    nn = int(min(max(int(a["n_fv_nodes"][k]), 0), n))
    b = k * stride
    offs = a["fv_offs"][k * (stride + 1):k * (stride + 1) + nn + 1].astype(np.int64)
    feats = a["fv_feats"][b:b + stride]
    bad = False
    if nn > 0:
        bad = bool(offs[0] < 0 or (np.diff(offs) < 0).any() or (offs > n).any())
        if not bad:
            bad = bool((feats[offs[0]:offs[nn]] >= n).any())
    s = side(a["desc"][b:b + n], a["keys"]["angle"][b:b + n],
             (a["fv_nodes"][b:b + nn], offs.astype(np.int32), feats), a["pidx"][b:b + n])
    return s, bad


# ----------------------------------------------------------------- reference
def expected(oracle, prob, nnratio, check_ori, min_matches=0):
    """(kp_match over the frame's keypoints, info tuple) of one well-formed problem."""
    kf, f, pts = prob["kf"], prob["f"], prob.get("points")
    pidx = kf["pidx"]
    has = pidx >= 0
    kf_mp = np.where(has, pidx, -1).astype(np.int32)
    bad = np.zeros(len(pidx), np.uint8)
    if pts is not None:
        bad[has] = pts["bad"][pidx[has]]
    args = (kf["desc"], kf["angle"], kf_mp, bad, kf["fv"], f["desc"], f["angle"], f["fv"], nnratio)
    n, fm = oracle.match_bow(*args, check_ori)
    n_acc = oracle.match_bow(*args, False)[0] if check_ori else n
    knodes, koffs, kfeats = kf["fv"]
    common = np.nonzero(np.isin(knodes, f["fv"][0]))[0]
    usable = has & (bad == 0)
    tried = sum(int(usable[kfeats[koffs[a]:koffs[a + 1]]].sum()) for a in common)
    enough = int(n >= min_matches)
    if not enough:
        fm = np.full(len(fm), -1, np.int32)
    return fm, (int(n), int(n_acc), len(common), tried, enough)


def expected_slot(oracle, kf_arrays, ks, f_arrays, fs, stride, points, nnratio, check_ori,
                  min_matches=0):
    """The same for keyframe slot ks against frame slot fs of packed arrays, with
    the malformed-slot rule: n_matches -1, the other fields 0, kp_match all -1
    over the clamped count."""
    kf, kbad = unpack_side(kf_arrays, ks, stride)
    f, fbad = unpack_side(f_arrays, fs, stride)
    if kbad or fbad:
        return np.full(len(f["desc"]), -1, np.int32), MALFORMED
    return expected(oracle, dict(kf=kf, f=f, points=points), nnratio, check_ori, min_matches)


def thin_to(oracle, prob, n, nnratio, check_ori, seed=0):
    """A copy of `prob` with keyframe map points dropped in a seeded order until
    the reference returns exactly n matches."""
    q = dict(prob, kf=dict(prob["kf"], pidx=prob["kf"]["pidx"].copy()))
    pidx = q["kf"]["pidx"]
    cur = expected(oracle, q, nnratio, check_ori)[1][0]
    for i in np.random.default_rng(seed).permutation(np.nonzero(pidx >= 0)[0]):
        if cur <= n:
            break
        keep = pidx[i]
        pidx[i] = -1
        got = expected(oracle, q, nnratio, check_ori)[1][0]
        if got < n:
            pidx[i] = keep   # this one took more than one match with it
        else:
            cur = got
    assert cur == n, (cur, n)
    return q


def check(km, info, p, n, want_km, want_info, sentinel, tag=""):
    """Problem p of the outputs (km (P, stride), info (P,) INFO_DTYPE) against the reference."""
    got = tuple(int(info[p][f]) for f in INFO_FIELDS)
    bad = np.nonzero(km[p, :n] != want_km)[0]
    assert len(bad) == 0, (tag, p, bad[:8], km[p, :n][bad[:8]], want_km[bad[:8]])
    assert got == tuple(want_info), (tag, p, got, want_info)
    assert (km[p, n:] == sentinel).all(), (tag, p, "slots past the count were written")
