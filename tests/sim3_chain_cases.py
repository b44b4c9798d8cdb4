"""Inputs of the ComputeSim3 matcher batches' tests, shared by the GPU tests
(test_gpu_bow_kf_batch.py, test_gpu_sim3_search_batch.py) and the CPU test that
holds the oracle-based reference against the pyref-based one on every one of
them (test_sim3_chain_ref.py).  No GPU.

A BoW set is dict(sides, pairs, points, nnratio, ori, min_matches, stride, edit);
a search set is dict(sides, probs, points, mp_desc, host, stride, with_inliers,
with_active).  `bow_refs` / `search_refs` derive what the entries must return
for a set from the packed slot arrays (tests/sim3_chain_ref.py)."""
import functools

import numpy as np

import bow_batch_ref as B
import matcher_edge_cases as E
import scenarios as S
import sim3_chain_ref as R
import tri_batch_ref as T

f32 = np.float32
EDGE_HOST = dict(cam=E.CAM, width=E.W, height=E.H, scale=E.SCALE, log_scale=E.LS, th=7.5)


# ============================================================== BoW(KF, KF)
def sides_of(c):
    """A bow_kf case (matcher_edge_cases.bow_case("kf", ...)) as two sides and the
    shared point array: the MapPoint ids become point indices."""
    mp1, mp2 = np.asarray(c["mp1"], np.int32), np.asarray(c["mp2"], np.int32)
    pts = np.zeros(int(max(mp1.max(initial=-1), mp2.max(initial=-1))) + 1, B.MAP_POINT_DTYPE)
    pts["pos"] = np.nan   # only `bad` may be read
    for mp, bad in ((mp1, c["bad1"]), (mp2, c["bad2"])):
        if bad is not None:
            pts["bad"][mp[mp >= 0]] = np.asarray(bad, np.uint8)[mp >= 0]
    return (B.side(c["d1"], c["a1"], c["fv1"], mp1), B.side(c["d2"], c["a2"], c["fv2"], mp2), pts)


def tri_as_bow(c):
    """hist_bow(form="kf") is a SearchForTriangulation case: the same descriptors,
    angles and FeatureVectors with a MapPoint behind every keypoint."""
    k1, k2 = c["kf1"], c["kf2"]
    n1, n2 = len(k1["desc"]), len(k2["desc"])
    return dict(d1=k1["desc"], a1=k1["keys"]["angle"], mp1=np.arange(n1, dtype=np.int32),
                bad1=None, fv1=c["fv1"], d2=k2["desc"], a2=k2["keys"]["angle"],
                mp2=(np.arange(n2) + n1).astype(np.int32), bad2=None, fv2=c["fv2"])


@functools.lru_cache(maxsize=None)
def bow_edge(name):
    if name == "nodes":
        return sides_of(E.bow_case("kf"))
    if name == "ties":
        return sides_of(E.bow_case("kf", ties=True))
    return sides_of(tri_as_bow(E.hist_bow(name, form="kf")))


@functools.lru_cache(maxsize=None)
def bow_natural(oracle, seed=0, nf=400):
    """scenarios.bow_pair read as two keyframes, with points (some bad, some
    NULL) on both sides."""
    c = S.bow_pair(oracle, seed, nf=nf)
    rng = np.random.default_rng(7)
    n1, n2 = len(c["kf_desc"]), len(c["f_desc"])
    mp1 = np.where(c["kf_mp"] >= 0, np.arange(n1), -1).astype(np.int32)
    mp2 = np.where(rng.random(n2) < 0.85, np.arange(n2) + n1, -1).astype(np.int32)
    return sides_of(dict(d1=c["kf_desc"], a1=c["kf_angle"], mp1=mp1, bad1=c["kf_bad"],
                         fv1=c["kf_fv"], d2=c["f_desc"], a2=c["f_angle"], mp2=mp2,
                         bad2=(rng.random(n2) < 0.05).astype(np.uint8), fv2=c["f_fv"]))


def shifted(side, off):
    return dict(side, pidx=np.where(side["pidx"] >= 0, side["pidx"] + off, -1).astype(np.int32))


def join(groups):
    """Scenes (side1, side2, points) laid out in one slot family and one point array."""
    sides, pts, off = [], [], 0
    for s1, s2, p in groups:
        sides += [shifted(s1, off), shifted(s2, off)]
        pts.append(p)
        off += len(p)
    return sides, np.concatenate(pts)


def bow_set(sides, pairs, points, nnratio=0.75, ori=True, min_matches=0, stride=None, edit=None):
    return dict(sides=sides, pairs=pairs, points=points, nnratio=nnratio, ori=ori,
                min_matches=min_matches, stride=stride, edit=edit)


def bow_edge_set(name, nnratio=0.75, ori=True):
    s1, s2, pts = bow_edge(name)
    return bow_set([s1, s2], [(0, 1)], pts, nnratio, ori)


def bow_natural_set(oracle, nnratio, ori):
    s1, s2, pts = bow_natural(oracle)
    return bow_set([s1, s2], [(0, 1), (1, 0)], pts, nnratio, ori)


def bow_empty_set():
    s1, s2, pts = bow_edge("nodes")
    none = B.side(np.zeros((0, 32), np.uint8), np.zeros(0, f32), B.empty_fv(), np.zeros(0, np.int32))
    nofv1, nofv2 = dict(s1, fv=B.empty_fv()), dict(s2, fv=B.empty_fv())
    return bow_set([s1, s2, none, nofv1, nofv2],
                   [(0, 2), (2, 1), (2, 2), (3, 1), (0, 4), (3, 4), (0, 1)], pts)


def bow_bad_null_set(oracle):
    """30 % of the points bad, half of either side's points NULL."""
    s1, s2, pts = bow_natural(oracle)
    rng = np.random.default_rng(3)
    p = pts.copy()
    p["bad"] = rng.random(len(p)) < 0.3
    thin = lambda s: dict(s, pidx=np.where(rng.random(len(s["pidx"])) < 0.5, s["pidx"], -1)
                          .astype(np.int32))
    return bow_set([s1, s2, thin(s1), thin(s2)], [(0, 1), (2, 1), (0, 3), (2, 3)], p)


def bow_no_points_set(oracle):
    s1, s2, _ = bow_natural(oracle)
    return bow_set([s1, s2], [(0, 1)], None)


def bow_mixed_set(oracle, P):
    sides, pts = join([bow_natural(oracle), bow_edge("nodes"), bow_edge("eleven_two_one"),
                       bow_natural(oracle, seed=1)])
    rng = np.random.default_rng(P)
    perm = rng.permutation(len(sides))          # slots permuted
    inv = np.argsort(perm)
    sides = [sides[i] for i in perm]
    cands = [1, 3, 5, 7, 6, 2]
    pairs = [(int(inv[0]), int(inv[cands[int(k)]])) for k in rng.integers(0, len(cands), P)]
    return bow_set(sides, pairs, pts)


@functools.lru_cache(maxsize=None)
def _gate_sides(oracle):
    s1, s2, pts = bow_natural(oracle)
    return [R.thin_kf1_to(oracle, s1, s2, pts, n, 0.75, True) for n in (19, 20)] + [s2], pts


def bow_gate_set(oracle):
    sides, pts = _gate_sides(oracle)
    return bow_set(sides, [(0, 2), (1, 2)], pts, min_matches=20)


MALFORMED = {
    "offset decreases": lambda a, k, S: a["fv_offs"].__setitem__(k * (S + 1) + 2, a["fv_offs"][k * (S + 1) + 1] - 1),
    "first offset negative": lambda a, k, S: a["fv_offs"].__setitem__(k * (S + 1), -1),
    "offset above the count": lambda a, k, S: a["fv_offs"].__setitem__(
        k * (S + 1) + int(a["n_fv_nodes"][k]), int(a["nkeys"][k]) + 1),
    "feature index at the count": lambda a, k, S: a["fv_feats"].__setitem__(k * S, a["nkeys"][k]),
    "feature index huge": lambda a, k, S: a["fv_feats"].__setitem__(k * S + 1, 0xFFFFFFF0),
}


def bow_malformed_set(oracle, kind):
    s1, s2, pts = bow_natural(oracle)
    sides = [s1, s2, dict(s1), dict(s2)]
    stride = max(len(s["desc"]) for s in sides) + 1

    def edit(a):
        MALFORMED[kind](a, 2, stride)
        MALFORMED[kind](a, 3, stride)
        a["nkeys"][1] = stride + 9              # clamped to the stride
        a["n_fv_nodes"][0] = -4                 # clamped to 0
    return bow_set(sides, [(0, 1), (2, 1), (0, 3), (2, 3), (1, 1)], pts, stride=stride, edit=edit)


def bow_stride_sets():
    s1, s2, pts = bow_edge("nodes")
    n = max(len(s1["desc"]), len(s2["desc"]))
    return [bow_set([s1, s2], [(0, 1)], pts, stride=st) for st in (n, n + 1)] + \
           [bow_set([s1, s2], [(0, 0), (1, 1)], pts)]        # the last: identity slots


def all_bow_sets(oracle):
    """(tag, set) of every BoW input the GPU tests run."""
    out = [("nodes", bow_edge_set("nodes", E.bow_case("kf")["nnratio"], False)),
           ("ties", bow_edge_set("ties", 1.25, False))]
    out += [(shape, bow_edge_set(shape)) for shape in E.HIST_SHAPES]
    out += [("natural %s %s" % (r, o), bow_natural_set(oracle, r, o))
            for r in (0.6, 0.9) for o in (False, True)]
    out += [("empty", bow_empty_set()), ("bad and NULL", bow_bad_null_set(oracle)),
            ("no point array", bow_no_points_set(oracle)), ("gate", bow_gate_set(oracle))]
    out += [("mixed %d" % P, bow_mixed_set(oracle, P)) for P in (1, 16, 300)]
    out += [(kind, bow_malformed_set(oracle, kind)) for kind in MALFORMED]
    out += [("stride %d" % i, s) for i, s in enumerate(bow_stride_sets())]
    return out


def bow_pack(c):
    """(packed slot arrays, stride) of a BoW set, its edit applied."""
    stride = c["stride"] or max(1, max(len(s["desc"]) for s in c["sides"]))
    arr = B.pack_slots(c["sides"], stride)
    if c["edit"]:
        c["edit"](arr)
    return arr, stride


def bow_refs(oracle, c, arr, stride, second=None):
    cache = {k: R.bow_kf_expected_slot(oracle, arr, k[0], k[1], stride, c["points"], c["nnratio"],
                                       c["ori"], c["min_matches"], second) for k in set(c["pairs"])}
    return [cache[k] for k in c["pairs"]]


# ============================================================= SearchBySim3
class Problem:
    """One (KF1 slot, KF2 slot) problem: rows over KF1's count, optional inliers,
    the Sim3 record and the active byte."""

    def __init__(self, k1, k2, m12, ix2, sim3, inliers=None, active=1):
        self.k1, self.k2, self.sim3, self.active = k1, k2, sim3, active
        self.m12, self.ix2 = np.asarray(m12, np.int32), np.asarray(ix2, np.int32)
        self.inliers = None if inliers is None else np.asarray(inliers, np.uint8)


def ident():
    return R.sim3_record()


def plain(k1, k2, s1, sim3=None, **kw):
    n = len(s1["desc"])
    return Problem(k1, k2, np.full(n, -1, np.int32), np.full(n, -1, np.int32),
                   ident() if sim3 is None else sim3, **kw)


def search_set(sides, probs, points, mp_desc, host=EDGE_HOST, stride=None, with_inliers=None,
               with_active=None):
    if with_inliers is None:
        with_inliers = any(q.inliers is not None for q in probs)
    if with_active is None:
        with_active = any(q.active != 1 for q in probs)
    return dict(sides=sides, probs=probs, points=np.ascontiguousarray(points, B.MAP_POINT_DTYPE),
                mp_desc=np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32), host=host,
                stride=stride or max(1, max(len(s["desc"]) for s in sides)),
                with_inliers=with_inliers, with_active=with_active)


@functools.lru_cache(maxsize=None)
def crowd(with_masks):
    return R.problem_from_case(E.by_sim3_case(257, with_masks=with_masks))


def _case_set(c):
    s1, s2, points, mp_desc, m12, ix2 = c
    return search_set([s1, s2], [Problem(0, 1, m12, ix2, ident())], points, mp_desc)


def search_crowd_set(with_masks):
    return _case_set(crowd(with_masks))


def search_thresholds_set():
    return _case_set(R.problem_from_case(E.by_sim3_thresholds()))


def search_empty_sets():
    return [_case_set(R.problem_from_case(c)) for c in E.empty_cases() if c["family"] == "by_sim3"]


def sub(side, n):
    """The first n keypoints of a side (no FeatureVector)."""
    s = dict(side)
    for k in ("desc", "angle", "pidx", "keys", "u_right"):
        s[k] = side[k][:n]
    s["fv"] = B.empty_fv()
    return s


def search_counts_set():
    """Keyframes of 0 / 1 / 63 / 64 / 65 / 257 keypoints, paired across sizes."""
    s1, s2, points, mp_desc, _, _ = crowd(False)
    sizes = (0, 1, 63, 64, 65, 257)
    sides = [sub(s1, n) for n in sizes] + [sub(s2, n) for n in sizes]
    probs = [plain(a, len(sizes) + b, sides[a]) for a in range(len(sizes))
             for b in range(len(sizes)) if a == b or (a + b) % 3 == 0]
    return search_set(sides, probs, points, mp_desc)


def grid_scene(xy1, xy2, seed=3, octave=0, noise=0.02):
    """Keyframes over given pixel positions, each keypoint with a MapPoint at its
    own pixel (identity poses, depth E.Z); KF2's descriptors are KF1's with noise
    where the positions pair up in order."""
    rng = np.random.default_rng(seed)
    sides, pts, descs = [], [], []
    base = rng.integers(0, 256, (max(len(xy1), len(xy2)), 32), dtype=np.uint8)
    off = 0
    for xy in (xy1, xy2):
        xy = np.asarray(xy, f32).reshape(-1, 2)
        n = len(xy)
        keys = E.keypoints(xy[:, 0], xy[:, 1], octave)
        desc = E.noisy(rng, base[:n], noise)
        mps = np.array([E.map_point(float(x), float(y), octave) for x, y in xy], E.MAP_POINT_DTYPE)
        kf = dict(keys=keys, desc=desc, Rw=E.EYE, tw=E.ZERO3)
        sides.append(R.side_from_sim3_kf(kf, (np.arange(n) + off).astype(np.int32)))
        pts.append(mps)
        descs.append(E.noisy(rng, desc, 0.01))
        off += n
    return sides, np.concatenate(pts), np.concatenate(descs)


def search_grid_sets():
    """"one_cell": 257 keypoints in one grid cell; "border": keypoints on min_x,
    just below max_x, outside the bounds, and windows clamped at each border."""
    rng = np.random.default_rng(11)
    # quarter-pixel lattice (map_point wants exactly representable positions):
    # 257 of the 17 x 17 positions inside one 10 x 10 pixel cell
    lattice = rng.permutation(289)[:257]
    one_cell = np.stack([100.5 + (lattice % 17) / 4.0, 100.5 + (lattice // 17) / 4.0], 1)
    W, H = float(E.W), float(E.H)
    border = [(0.0, 50.0), (W - 0.25, 60.0), (-3.0, 70.0), (W + 10.0, 80.0), (40.0, 0.0),
              (50.0, H - 0.25), (60.0, -2.0), (70.0, H + 5.0), (1.0, 1.0), (W - 1.5, 1.0),
              (1.0, H - 1.5), (W - 1.5, H - 1.5), (W / 2, 2.0), (W / 2, H - 2.0), (2.0, H / 2),
              (W - 2.0, H / 2)]
    moved = [(x + 0.5, y - 0.5) for x, y in border]
    out = {}
    for name, xy1, xy2 in (("one_cell", one_cell, one_cell + f32(0.25)), ("border", border, moved)):
        sides, points, mp_desc = grid_scene(xy1, xy2)
        out[name] = search_set(sides, [plain(0, 1, sides[0])], points, mp_desc)
    return out


@functools.lru_cache(maxsize=None)
def natural(oracle, s12, rotated, nf=300, seed=5):
    """sim3_chain_ref.loop_scene: a loop candidate and a current keyframe that
    sees its map through the similarity (s12, R12, t12), 80 % of KF2's
    keypoints with a point."""
    return R.loop_scene(oracle, s12, rotated, nf, seed, p2_frac=0.8)


@functools.lru_cache(maxsize=None)
def natural_rows(oracle, s12=1.1, rotated=False):
    """The natural pair with the rows SearchByBoW(KF1, KF2) gives."""
    (s1, s2), points, mp_desc, host, rec = natural(oracle, s12, rotated)
    m12, ix2, info = R.bow_kf_expected(oracle, s1, s2, points, 0.75, True)
    assert info[0] > 20
    return (s1, s2), points, mp_desc, host, rec, m12, ix2


SIMILARITIES = ((0.5, False), (1.0, True), (1.1, False), (2.0, True))


def search_natural_set(oracle, s12, rotated):
    (s1, s2), points, mp_desc, host, rec = natural(oracle, s12, rotated)
    return search_set([s1, s2], [plain(0, 1, s1, rec)], points, mp_desc, host)


def search_filter_set(oracle):
    """The inlier filter absent / all ones / all zeros / mixed, and index2 entries of
    -1, N2 - 1, N2 and kp_stride + 5 (with_inliers: the array is given; the first
    problem has none of its own, so its junk bytes read as inliers)."""
    (s1, s2), points, mp_desc, host, rec, m12, ix2 = natural_rows(oracle)
    n1, n2 = len(s1["desc"]), len(s2["desc"])
    rng = np.random.default_rng(2)
    have = np.nonzero(m12 >= 0)[0]
    odd = ix2.copy()
    stride = n1 + 3
    for i, v in zip(have[:4], (-1, n2 - 1, n2, stride + 5)):
        odd[i] = v
    probs = [Problem(0, 1, m12, ix2, rec),
             Problem(0, 1, m12, ix2, rec, np.ones(n1, np.uint8)),
             Problem(0, 1, m12, ix2, rec, np.zeros(n1, np.uint8)),
             Problem(0, 1, m12, ix2, rec, (rng.random(n1) < 0.5).astype(np.uint8) * 255),
             Problem(0, 1, m12, odd, rec, np.ones(n1, np.uint8))]
    return search_set([s1, s2], probs, points, mp_desc, host, stride, with_inliers=True), len(have)


def search_no_filter_set(oracle):
    c, _ = search_filter_set(oracle)
    return dict(c, probs=c["probs"][:1], with_inliers=False)


def search_mixed_set(oracle, P):
    """Two candidates (slots 1 and 3) against the current keyframe as seen through
    two similarities (slots 0 and 2), the point arrays concatenated; run, no
    Sim3, inactive and filtered problems drawn at random."""
    (s1, s2), points, mp_desc, host, rec, m12, ix2 = natural_rows(oracle)
    (r1, r2), rpts, rdesc, _, rrec = natural(oracle, 1.0, True)
    off = len(points)
    sides = [s1, s2, shifted(r1, off), shifted(r2, off)]
    pts, dsc = np.concatenate([points, rpts]), np.concatenate([mp_desc, rdesc])
    none = R.sim3_record(has=0)
    rng = np.random.default_rng(4)
    kinds = [Problem(0, 1, m12, ix2, rec), Problem(0, 1, m12, ix2, none),
             Problem(0, 1, m12, ix2, rec, active=0),
             Problem(0, 1, m12, ix2, rec, (rng.random(len(m12)) < 0.7).astype(np.uint8)),
             plain(2, 3, r1, rrec), plain(0, 3, s1, rrec)]
    for n in (1, 16, 300):      # one random stream over the three batch sizes
        probs = [kinds[int(k)] for k in rng.integers(0, len(kinds), n)]
        if n == P:
            break
    if P == 1:
        probs = kinds[:1]
    return search_set(sides, probs, pts, dsc, host, with_inliers=True, with_active=True)


def search_stride_sets(oracle):
    (s1, s2), points, mp_desc, host, rec, m12, ix2 = natural_rows(oracle)
    n = max(len(s1["desc"]), len(s2["desc"]))
    return [search_set([s1, s2], [Problem(0, 1, m12, ix2, rec)], points, mp_desc, host, st)
            for st in (n, n + 1)]


def search_identity_set(oracle):
    """Problem p uses slot p for both keyframes."""
    (s1, _), points, mp_desc, host, rec = natural(oracle, 1.1, False)
    return search_set([s1, s1], [plain(0, 0, s1, rec), plain(1, 1, s1, rec)], points, mp_desc, host)


def all_search_sets(oracle):
    """(tag, set) of every SearchBySim3 input the GPU tests run."""
    out = [("crowd masks", search_crowd_set(True)), ("crowd", search_crowd_set(False)),
           ("thresholds", search_thresholds_set()), ("counts", search_counts_set())]
    out += [("empty %d" % i, c) for i, c in enumerate(search_empty_sets())]
    out += list(search_grid_sets().items())
    out += [("natural %s %s" % sr, search_natural_set(oracle, *sr)) for sr in SIMILARITIES]
    out += [("filter", search_filter_set(oracle)[0]), ("no filter", search_no_filter_set(oracle))]
    out += [("mixed %d" % P, search_mixed_set(oracle, P)) for P in (1, 16, 300)]
    out += [("stride %d" % i, c) for i, c in enumerate(search_stride_sets(oracle))]
    out += [("identity slots", search_identity_set(oracle))]
    return out


def search_pack(c):
    return T.pack_slots(c["sides"], c["stride"], with_u_right=False)


def search_refs(oracle, c, arr, second=None):
    """Per problem what the entry must leave (None: skipped), distinct problems once."""
    cache, refs = {}, []
    for q in c["probs"]:
        key = (q.k1, q.k2, q.m12.tobytes(), q.ix2.tobytes(),
               None if q.inliers is None else q.inliers.tobytes(), q.sim3.tobytes(), q.active)
        if key not in cache:
            cache[key] = R.sim3_expected_slot(
                oracle, arr, q.k1, q.k2, c["stride"], c["points"], c["mp_desc"], q.m12, q.ix2,
                q.inliers if c["with_inliers"] else None, q.sim3, c["host"],
                q.active if c["with_active"] else 1, second)
        refs.append(cache[key])
    return refs
