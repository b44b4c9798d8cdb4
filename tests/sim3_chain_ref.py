"""Reference side of the two matcher batches of LoopClosing::ComputeSim3
(orb_match_bow_kf_batch, orb_search_by_sim3_batch): derives what the entries
must return for a problem from the packed slot arrays, read as their contracts
say (counts clamped, FeatureVectors validated, the inlier filter, the
already-matched masks, the merge), with the C++ oracle's search_by_bow_kf /
search_by_sim3 as the matcher; `second=` swaps in pyref's restatements.  No GPU.

Slots are bow_batch_ref.pack_slots / tri_batch_ref.pack_slots arrays; a side is
tri_batch_ref's (desc, angle, fv, pidx, keys, pose).  Tests keep each keyframe's
non-negative point_index entries distinct, so index2 is the position of the id."""
import numpy as np

import bow_batch_ref as B
import matcher_edge_cases as E
import pyref
import tri_batch_ref as T

f32 = np.float32
BOW_FIELDS = B.INFO_FIELDS
BOW_MALFORMED = B.MALFORMED
SEARCH_INFO_DTYPE = np.dtype([("n_found", "<i4"), ("n_kept", "<i4"), ("n_total", "<i4"),
                              ("n_best12", "<i4"), ("n_best21", "<i4")])
SEARCH_FIELDS = SEARCH_INFO_DTYPE.names
SIM3_RESULT_DTYPE = np.dtype([("has_sim3", "<i4"), ("no_more", "<i4"), ("n_inliers", "<i4"),
                              ("iterations_run", "<i4"), ("T12", "<f4", (16,)),
                              ("R", "<f4", (9,)), ("t", "<f4", (3,)), ("scale", "<f4")])


# ------------------------------------------------------------- BoW(KF, KF)
def _bad_of(pidx, points):
    bad = np.zeros(len(pidx), np.uint8)
    if points is not None:
        has = pidx >= 0
        bad[has] = points["bad"][pidx[has]]
    return bad


def rows_from_ids(m12, pidx2):
    """index2 of a row of point ids: the position of the id in KF2's point_index."""
    pos = {int(v): i for i, v in enumerate(pidx2) if v >= 0}
    assert len(pos) == int((pidx2 >= 0).sum()), "point_index entries of a keyframe must be distinct"
    return np.array([pos[int(m)] if m >= 0 else -1 for m in m12], np.int32)


def gate(m12, index2, n, min_matches):
    """ComputeSim3's nmatches < 20 gate through empty rows."""
    if n >= min_matches:
        return m12, index2, 1
    return np.full(len(m12), -1, np.int32), np.full(len(m12), -1, np.int32), 0


def bow_kf_expected(oracle, s1, s2, points, nnratio, check_ori, min_matches=0, second=None):
    """(match12, index2, info tuple) of one well-formed problem."""
    search = second or oracle.search_by_bow_kf
    p1, p2 = s1["pidx"], s2["pidx"]
    mp1 = np.where(p1 >= 0, p1, -1).astype(np.int32)
    mp2 = np.where(p2 >= 0, p2, -1).astype(np.int32)
    bad1, bad2 = _bad_of(p1, points), _bad_of(p2, points)
    args = (s1["desc"], s1["angle"], mp1, bad1, s1["fv"], s2["desc"], s2["angle"], mp2, bad2,
            s2["fv"], nnratio)
    n, m12 = search(*args, bool(check_ori))
    n_acc = search(*args, False)[0] if check_ori else n
    nodes1, offs1, feats1 = s1["fv"]
    common = np.nonzero(np.isin(nodes1, s2["fv"][0]))[0]
    usable = (p1 >= 0) & (bad1 == 0)
    tried = sum(int(usable[feats1[offs1[a]:offs1[a + 1]]].sum()) for a in common)
    m12 = np.asarray(m12, np.int32)
    m12, ix2, enough = gate(m12, rows_from_ids(m12, p2), int(n), min_matches)
    return m12, ix2, (int(n), int(n_acc), len(common), tried, enough)


def bow_kf_expected_slot(oracle, arr, k1, k2, stride, points, nnratio, check_ori, min_matches=0,
                         second=None):
    """The same for slots k1, k2 of packed arrays, with the malformed-slot rule."""
    s1, bad1 = B.unpack_side(arr, k1, stride)
    s2, bad2 = B.unpack_side(arr, k2, stride)
    if bad1 or bad2:
        none = np.full(len(s1["desc"]), -1, np.int32)
        return none, none.copy(), BOW_MALFORMED
    return bow_kf_expected(oracle, s1, s2, points, nnratio, check_ori, min_matches, second)


def thin_kf1_to(oracle, s1, s2, points, n, nnratio, check_ori, seed=0):
    """A copy of side s1 with map points dropped in a seeded order until the
    reference returns exactly n matches (bow_batch_ref.thin_to for this matcher)."""
    q = dict(s1, pidx=s1["pidx"].copy())
    pidx = q["pidx"]
    count = lambda: bow_kf_expected(oracle, q, s2, points, nnratio, check_ori)[2][0]
    cur = count()
    for i in np.random.default_rng(seed).permutation(np.nonzero(pidx >= 0)[0]):
        if cur <= n:
            break
        keep = pidx[i]
        pidx[i] = -1
        got = count()
        if got < n:
            pidx[i] = keep   # this one took more than one match with it
        else:
            cur = got
    assert cur == n, (cur, n)
    return q


def check_bow(m12, ix2, info, p, n, want, sentinel, tag=""):
    want_m12, want_ix2, want_info = want
    got = tuple(int(info[p][f]) for f in BOW_FIELDS)
    for name, row, ref in (("match12", m12, want_m12), ("index2", ix2, want_ix2)):
        bad = np.nonzero(row[p, :n] != ref)[0]
        assert len(bad) == 0, (tag, name, p, bad[:8], row[p, :n][bad[:8]], ref[bad[:8]])
        assert (row[p, n:] == sentinel).all(), (tag, name, p, "slots past the count were written")
    assert got == tuple(want_info), (tag, p, got, want_info)


# ------------------------------------------------------------- SearchBySim3
def filter_rows(m12, ix2, inliers):
    """Step 1 (src/LoopClosing.cc:338-343): entries that are not inliers become NULL."""
    m12, ix2 = np.array(m12, np.int32), np.array(ix2, np.int32)
    if inliers is not None:
        out = np.asarray(inliers)[:len(m12)] == 0
        m12[out] = -1
        ix2[out] = -1
    return m12, ix2


def already_masks(m12, ix2, n2):
    """Step 2 (src/ORBmatcher.cc:1245-1258); an index2 outside [0, n2) is ignored."""
    a1 = (m12 >= 0).astype(np.uint8)
    a2 = np.zeros(n2, np.uint8)
    j = ix2[(m12 >= 0) & (ix2 >= 0) & (ix2 < n2)]
    a2[j] = 1
    return a1, a2


def merge(m12, ix2, new12, pidx2):
    """Step 7: the rows with this call's matches written in."""
    m12, ix2 = m12.copy(), ix2.copy()
    add = new12 >= 0
    m12[add] = pidx2[new12[add]]
    ix2[add] = new12[add]
    return m12, ix2


def kf_dict(s, points, mp_desc, already, host):
    pidx = s["pidx"]
    safe = np.maximum(pidx, 0)
    n = len(pidx)
    return dict(keys=s["keys"], desc=s["desc"], scale=host["scale"], width=host["width"],
                height=host["height"], Rw=np.asarray(s["pose"]["rcw"], f32).reshape(3, 3),
                tw=np.asarray(s["pose"]["tcw"], f32),
                mps=points[safe] if n else points[:0],
                valid=(pidx >= 0).astype(np.uint8), already=already,
                mp_desc=mp_desc[safe] if n else mp_desc[:0])


def directions(k1, k2, cam, s12, R12, t12, th, log_scale):
    """vnMatch1 and vnMatch2 (the two one-way rows the oracle does not return)
    from pyref's primitives, as pyref.search_by_sim3 states them."""
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    R12 = np.asarray(R12, f32).reshape(3, 3)
    sR12 = np.array([[f32(float(s12) * float(R12[r, c])) for c in range(3)] for r in range(3)])
    sR21 = np.array([[f32((1.0 / float(s12)) * float(R12[c, r])) for c in range(3)]
                     for r in range(3)])
    t21 = np.array([-(f32(f32(sR21[r, 0] * f32(t12[0])) + f32(sR21[r, 1] * f32(t12[1])))
                      + f32(sR21[r, 2] * f32(t12[2]))) for r in range(3)], f32)
    n_levels = len(k1["scale"])

    def direction(A, Bk, sR, tt):
        cells, invW, invH = pyref.grid_cells(Bk["keys"], Bk["width"], Bk["height"])
        out = np.full(len(A["keys"]), -1, np.int32)
        for i, mp in enumerate(A["mps"]):
            if not A["valid"][i] or A["already"][i] or mp["bad"]:
                continue
            Pb = pyref._xf(sR, tt, pyref._xf(A["Rw"], A["tw"], mp["pos"]))
            if Pb[2] < 0:
                continue
            invz = f32(1.0 / float(Pb[2]))
            u = f32(f32(fx * f32(Pb[0] * invz)) + cx)
            v = f32(f32(fy * f32(Pb[1] * invz)) + cy)
            if not pyref._in_kf(u, v, Bk["width"], Bk["height"]):
                continue
            dist = pyref._norm(Pb)
            if dist < f32(f32(0.8) * mp["min_distance"]) or dist > f32(f32(1.2) * mp["max_distance"]):
                continue
            lvl = pyref._level(mp["max_distance"], dist, log_scale, n_levels)
            bd, bi = pyref._best(Bk["keys"], Bk["desc"], cells, invW, invH, A["mp_desc"][i], u, v,
                                 f32(f32(th) * f32(Bk["scale"][lvl])), lvl - 1, lvl, init=1 << 31)
            if bd <= 100:
                out[i] = bi
        return out

    return direction(k1, k2, sR21, t21), direction(k2, k1, sR12, np.asarray(t12, f32))


def sim3_expected(oracle, s1, s2, points, mp_desc, m12, ix2, inliers, sim3, host, second=None):
    """(match12, index2, new12, info tuple) of one problem that is not skipped.
    host: dict(cam, width, height, scale, log_scale, th); sim3: a
    SIM3_RESULT_DTYPE record.  The one-way counts come from `directions`, whose
    agreement must be the matcher's row."""
    n1, n2 = len(s1["desc"]), len(s2["desc"])
    m12, ix2 = filter_rows(np.asarray(m12)[:n1], np.asarray(ix2)[:n1], inliers)
    a1, a2 = already_masks(m12, ix2, n2)
    k1 = kf_dict(s1, points, mp_desc, a1, host)
    k2 = kf_dict(s2, points, mp_desc, a2, host)
    s12, R12, t12 = f32(sim3["scale"]), np.asarray(sim3["R"], f32), np.asarray(sim3["t"], f32)
    if second is None:
        nf, new12 = oracle.search_by_sim3(k1, k2, host["cam"], s12, R12, t12, host["th"],
                                          host["log_scale"])
    else:
        nf, new12 = second(k1, k2, host["cam"], s12, R12, t12, host["th"], host["log_scale"],
                           len(host["scale"]))
    new12 = np.asarray(new12, np.int32)
    v1, v2 = directions(k1, k2, host["cam"], s12, R12, t12, host["th"], host["log_scale"])
    mutual = np.array([j if j >= 0 and v2[j] == i else -1 for i, j in enumerate(v1)], np.int32)
    assert np.array_equal(mutual, new12), "the one-way rows disagree with the matcher's row"
    kept = int((m12 >= 0).sum())
    out12, outx2 = merge(m12, ix2, new12, s2["pidx"])
    return out12, outx2, new12, (int(nf), kept, kept + int(nf), int((v1 >= 0).sum()),
                                 int((v2 >= 0).sum()))


def sim3_expected_slot(oracle, arr, k1, k2, stride, points, mp_desc, m12, ix2, inliers, sim3,
                       host, active=1, second=None):
    """The same for slots k1, k2 of tri_batch_ref.pack_slots arrays; None for a
    skipped problem (has_sim3 == 0 or active == 0)."""
    if not active or not int(sim3["has_sim3"]):
        return None
    s1, _ = T.unpack_side(arr, k1, stride)
    s2, _ = T.unpack_side(arr, k2, stride)
    return sim3_expected(oracle, s1, s2, points, mp_desc, m12, ix2, inliers, sim3, host, second)


def sim3_record(R=E.EYE, t=E.ZERO3, s=1.0, has=1):
    rec = np.zeros(1, SIM3_RESULT_DTYPE)[0]
    rec["has_sim3"], rec["scale"] = has, f32(s)
    rec["R"], rec["t"] = np.asarray(R, f32).reshape(9), np.asarray(t, f32)
    return rec


def side_from_sim3_kf(kf, pidx, fv=None):
    """A by_sim3 keyframe dict (keys, desc, Rw, tw) as a tri_batch_ref side with
    the given point_index."""
    keys = np.ascontiguousarray(kf["keys"], B.KEYPOINT_DTYPE)
    s = B.side(kf["desc"], keys["angle"], fv or B.empty_fv(), pidx)
    s.update(keys=keys, u_right=np.full(len(keys), -1.0, f32),
             pose=T.pose_rec(kf["Rw"], kf["tw"]))
    return s


def problem_from_case(c):
    """A matcher_edge_cases by_sim3 case as (side1, side2, points, mp_desc, match12,
    index2): the points of both keyframes in one array (KF1's first); `valid`
    becomes point_index, `already` becomes entries of the rows (KF1's already
    flags name, in order, the already-flagged keypoints of KF2; a flag left over
    on KF1 is a match to a point KF2 does not observe, index2 -1)."""
    k1, k2 = c["kf1"], c["kf2"]
    n1, n2 = len(k1["keys"]), len(k2["keys"])
    points = np.concatenate([np.asarray(k1["mps"], B.MAP_POINT_DTYPE),
                             np.asarray(k2["mps"], B.MAP_POINT_DTYPE)])
    mp_desc = np.concatenate([np.asarray(k1["mp_desc"], np.uint8).reshape(-1, 32),
                              np.asarray(k2["mp_desc"], np.uint8).reshape(-1, 32)])
    p1 = np.where(np.asarray(k1["valid"]) != 0, np.arange(n1), -1).astype(np.int32)
    p2 = np.where(np.asarray(k2["valid"]) != 0, np.arange(n2) + n1, -1).astype(np.int32)
    m12, ix2 = np.full(n1, -1, np.int32), np.full(n1, -1, np.int32)
    al1 = np.nonzero(np.asarray(k1["already"]) != 0)[0]
    al2 = np.nonzero((np.asarray(k2["already"]) != 0) & (p2 >= 0))[0]
    for i, j in zip(al1, al2):
        m12[i], ix2[i] = p2[j], j
    for i in al1[len(al2):]:     # matched to a point that KF2 does not observe
        m12[i], ix2[i] = n1, -1
    return side_from_sim3_kf(k1, p1), side_from_sim3_kf(k2, p2), points, mp_desc, m12, ix2


def check_sim3(rows, info, p, n, before, want, sentinel, tag=""):
    """Problem p of the outputs (rows: dict match12 / index2 / new12 of (P, stride)
    arrays; info (P,) SEARCH_INFO_DTYPE) against the reference; want None: the
    problem was skipped and every byte of it is as `before` (the same dict) left it."""
    if want is None:
        for k in rows:
            assert np.array_equal(rows[k][p], before[k][p]), (tag, k, p, "a skipped row was written")
        assert bytes(info[p].tobytes()) == bytes([sentinel & 0xFF]) * info.dtype.itemsize, \
            (tag, p, "a skipped info record was written")
        return
    for k, ref in zip(("match12", "index2", "new12"), want[:3]):
        if k not in rows:
            continue
        bad = np.nonzero(rows[k][p, :n] != ref)[0]
        assert len(bad) == 0, (tag, k, p, bad[:8], rows[k][p, :n][bad[:8]], ref[bad[:8]])
        assert np.array_equal(rows[k][p, n:], before[k][p, n:]), \
            (tag, k, p, "slots past the count were written")
    got = tuple(int(info[p][f]) for f in SEARCH_FIELDS)
    assert got == tuple(want[3]), (tag, p, got, want[3])


# ------------------------------------------------------------- the chain scene
def loop_scene(oracle, s12=1.1, rotated=False, nf=500, seed=5, p2_frac=None):
    """A loop candidate KF2 and a current keyframe KF1 that sees KF2's map through
    the similarity X1c = s12 R12 X2c + t12 (test_gpu_sim3's chain scene for
    s12 = 1.1, not rotated: KF1 sees the same image, its descriptors are KF2's
    with 3 % of the bits flipped; rotated: KF1's keypoints at the projections of
    X1c).  Returns ((side1, side2), points, mp_desc, host, the exact Sim3 record);
    KF1's points are entries [0, n), KF2's [n, 2n)."""
    import scenarios as S
    rng = np.random.default_rng(seed)
    R2, t2, _ = S.pose(rng)
    kf2 = S.keyframe(oracle, 3, 0, R2, t2, rng, nf=nf)
    n = len(kf2["keys"])
    R1, t1, _ = S.pose(rng)
    bits = np.unpackbits(kf2["desc"], axis=1) ^ (rng.random((n, 256)) < 0.03)
    desc1 = np.packbits(bits.astype(np.uint8), axis=1)
    R12 = (S._rot(0.0, 0.0, 0.02) if rotated else np.eye(3)).astype(f32)
    t12 = np.array([0.1, -0.05, 0.2] if rotated else [0, 0, 0], f32)
    X2 = (kf2["mps"]["pos"].astype(np.float64) @ R2.astype(np.float64).T) + t2
    X1 = s12 * (X2 @ R12.astype(np.float64).T) + t12
    keys1 = kf2["keys"].copy()
    if rotated:
        fx, fy, cx, cy = S.camera()[:4]
        keys1["x"] = (fx * X1[:, 0] / X1[:, 2] + cx).astype(f32)
        keys1["y"] = (fy * X1[:, 1] / X1[:, 2] + cy).astype(f32)
    mps1 = kf2["mps"].copy()
    mps1["pos"] = ((X1 - t1.astype(np.float64)) @ R1.astype(np.float64)).astype(f32)
    mps1["max_distance"] *= f32(s12)
    mps1["min_distance"] *= f32(s12)
    p1 = np.where(kf2["valid"] > 0, np.arange(n), -1).astype(np.int32)
    keep2 = kf2["valid"] > 0 if p2_frac is None else rng.random(n) < p2_frac
    p2 = np.where(keep2, np.arange(n) + n, -1).astype(np.int32)
    fv = lambda d: oracle.feature_vector(S.vocab_nodes(d))
    s1 = side_from_sim3_kf(dict(keys=keys1, desc=desc1, Rw=R1, tw=t1), p1, fv(desc1))
    s2 = side_from_sim3_kf(dict(keys=kf2["keys"], desc=kf2["desc"], Rw=R2, tw=t2), p2,
                           fv(kf2["desc"]))
    points = np.concatenate([mps1, kf2["mps"]])
    mp_desc = np.concatenate([kf2["mp_desc"], kf2["mp_desc"]])
    host = dict(cam=S.camera(), width=kf2["width"], height=kf2["height"], scale=kf2["scale"],
                sigma2=np.asarray(kf2["sigma2"], f32), inv_sigma2=np.asarray(kf2["inv_sigma2"], f32),
                log_scale=E.LS, th=7.5)
    return (s1, s2), points, mp_desc, host, sim3_record(R12, t12, s12)


def chain_scene(oracle, nf=500):
    """The current keyframe (slot 0) and three loop candidates: slot 1 the loop
    scene's KF2; slot 2 the same keyframe observing few points (SearchByBoW
    returns fewer than 20: gated); slot 3 the same keyframe over a map whose
    points lie elsewhere (enough BoW matches, no Sim3 with 20 inliers)."""
    (s1, s2), points, mp_desc, host, _ = loop_scene(oracle, nf=nf)
    n = len(s2["desc"])
    rng = np.random.default_rng(17)
    few = dict(s2, pidx=np.where(rng.random(n) < 0.04, s2["pidx"], -1).astype(np.int32))
    wrong_pts = points[n:2 * n].copy()
    wrong_pts["pos"] = (wrong_pts["pos"] + rng.uniform(-6, 6, (n, 3))).astype(f32)
    wrong = dict(s2, pidx=np.where(s2["pidx"] >= 0, s2["pidx"] + n, -1).astype(np.int32))
    points = np.concatenate([points, wrong_pts])
    mp_desc = np.concatenate([mp_desc, mp_desc[n:2 * n]])
    draws = rng.integers(0, 2147483648, (3, 900)).astype(np.uint32)
    return [s1, s2, few, wrong], [(0, 1), (0, 2), (0, 3)], points, mp_desc, host, draws


def chain_reference(oracle, sides, pairs, points, mp_desc, host, draws, rounds=2, optimise=True,
                    second=None):
    """The host loop of ComputeSim3 per candidate: oracle.search_by_bow_kf with the
    20-match gate -> sim3_ref.Sim3Solver -> per round iterate(5), then, with a
    Sim3, the inlier filter, oracle.search_by_sim3, the merge and
    sim3opt_ref.optimize_sim3.  Returns per candidate a dict: bow (rows and info),
    state0, rounds (list of dict: result, inliers, search, opt), match12, index2
    (the final rows) and state (the solver's last state record).  second: (BoW
    matcher, Sim3 matcher) of pyref in place of the oracle's."""
    import sim3_ref
    import sim3opt_ref
    out = []
    cam = host["cam"]
    for c, (k1, k2) in enumerate(pairs):
        s1, s2 = sides[k1], sides[k2]
        m12, ix2, binfo = bow_kf_expected(oracle, s1, s2, points, 0.75, True, 20,
                                          second[0] if second else None)
        kf = lambda s: sim3_ref.KeyFrame(s["keys"]["octave"], s["pidx"], s["pose"]["rcw"],
                                         s["pose"]["tcw"])
        solver = sim3_ref.Sim3Solver(kf(s1), kf(s2), m12, False, points_pos=points["pos"],
                                     points_bad=points["bad"], index2=ix2,
                                     level_sigma2=host["sigma2"], K1=cam[:4], K2=cam[:4],
                                     draws=draws[c])
        rec = dict(bow=(m12.copy(), ix2.copy(), binfo), state0=solver.state_record(), rounds=[])
        for _ in range(rounds):
            T, no_more, vb, n_in = solver.iterate(5)
            res = np.atleast_1d(solver.result_record(T, no_more, n_in))[0]
            rr = dict(result=res, inliers=np.asarray(vb).astype(np.uint8), search=None, opt=None)
            if int(res["has_sim3"]):
                m12, ix2, new12, sinfo = sim3_expected(oracle, s1, s2, points, mp_desc, m12, ix2,
                                                       rr["inliers"], res, host,
                                                       second[1] if second else None)
                rr["search"] = (m12.copy(), ix2.copy(), new12, sinfo)
                if optimise:
                    xy = lambda s: np.stack([s["keys"]["x"], s["keys"]["y"]], 1)
                    pose = lambda s: (s["pose"]["rcw"], s["pose"]["tcw"])
                    r = sim3opt_ref.optimize_sim3(
                        xy(s1), s1["keys"]["octave"], s1["pidx"], pose(s1), xy(s2),
                        s2["keys"]["octave"], pose(s2), points["pos"], points["bad"], m12, ix2,
                        (res["R"], res["t"], res["scale"]), host["inv_sigma2"], cam[:4], cam[:4],
                        10.0, False)
                    rr["opt"] = sim3opt_ref.result_record(r)[0]
                    if r["status"] == 0:
                        m12 = np.asarray(r["match12"], np.int32).copy()
            rec["rounds"].append(rr)
        rec.update(match12=m12, index2=ix2, state=solver.state_record())
        out.append(rec)
    return out
