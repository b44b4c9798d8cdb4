"""The device-batched SearchByBoW(KF, F) (orb_match_bow_batch, k_bow_batch) and
the strided-count discard entry against the CPU: the C++ oracle's match_bow per
problem on the slot arrays read as the entry's contract says
(tests/bow_batch_ref.py).  kp_match index-exact over the frame's count, all five
info fields exact, slots past the count and the neighbours' untouched."""
import functools

import numpy as np
import pytest

import bow_batch_ref as B
import matcher_edge_cases as E
import scenarios as S
import track_motion_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
JUNK = 77
INT_MIN = -(1 << 31)


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def matchers(gpu):
    return {(r, o): gpu.ORBmatcher(r, bool(o)) for r in (0.7, 0.75, 0.9, 1.25) for o in (0, 1)}


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


# -------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def natural(oracle, seed, nf):
    return B.from_bow(S.bow_pair(oracle, seed, nf=nf))


@functools.lru_cache(maxsize=None)
def edge(name):
    if name == "nodes":
        return E.bow_case("frame")
    if name == "ties":
        return E.bow_case("frame", ties=True)
    return E.hist_bow(name)


EDGE_NAMES = ("nodes", "ties") + tuple(E.HIST_SHAPES)


def edge_problem(name):
    return B.from_bow(edge(name))


def tiny_problems(oracle):
    """The degenerate shapes: name -> problem."""
    base = natural(oracle, 5, 60)
    kf, f, pts = base["kf"], base["f"], base["points"]
    none = B.side(np.zeros((0, 32), np.uint8), np.zeros(0, f32), B.empty_fv(), np.zeros(0, np.int32))
    nof = B.side(np.zeros((0, 32), np.uint8), np.zeros(0, f32), B.empty_fv())
    d = np.arange(32, dtype=np.uint8).reshape(1, 32)
    one_fv = (np.array([9], np.uint32), np.array([0, 1], np.int32), np.array([0], np.uint32))
    all_bad = pts.copy()
    all_bad["bad"] = 1
    return {
        "no_kf_keypoints": dict(kf=none, f=f, points=pts),
        "no_f_keypoints": dict(kf=kf, f=nof, points=pts),
        "no_nodes": dict(kf=dict(kf, fv=B.empty_fv()), f=dict(f, fv=B.empty_fv()), points=pts),
        "no_common_node": dict(kf=dict(kf, fv=(kf["fv"][0] + 1000,) + kf["fv"][1:]), f=f, points=pts),
        "one_each": dict(kf=B.side(d, [10.0], one_fv, [3]), f=B.side(d, [40.0], one_fv),
                         points=pts[:4]),
        "all_null": dict(kf=dict(kf, pidx=np.full(len(kf["pidx"]), -1, np.int32)), f=f, points=pts),
        "all_bad": dict(kf=kf, f=f, points=all_bad),
    }


# ------------------------------------------------------------------- harness
class Batch:
    """Device copies of packed slots, outputs filled with JUNK."""

    def __init__(self, torch, kf_arrays, f_arrays, stride, n_problems, points=None, mp_stride=0,
                 kf_index=None, f_index=None):
        self.torch, self.P, self.stride, self.mp_stride = torch, n_problems, stride, mp_stride
        self.kf = {k: _dev(torch, v) for k, v in kf_arrays.items()}
        self.f = self.kf if f_arrays is kf_arrays else {k: _dev(torch, v) for k, v in f_arrays.items()}
        self.points = None if points is None else _dev(torch, points)
        self.kf_index = None if kf_index is None else _dev(torch, np.asarray(kf_index, np.int32))
        self.f_index = None if f_index is None else _dev(torch, np.asarray(f_index, np.int32))
        self.km = torch.full((n_problems * stride,), JUNK, dtype=torch.int32, device="cuda")
        self.info = torch.full((n_problems * 5,), JUNK, dtype=torch.int32, device="cuda")

    def args(self, min_matches=0, stream=0):
        p = lambda t: 0 if t is None else t.data_ptr()
        a = dict(n_problems=self.P, d_kf_index=p(self.kf_index), d_f_index=p(self.f_index),
                 d_kf_keys=p(self.kf["keys"]), d_kf_desc=p(self.kf["desc"]),
                 d_kf_nkeys=p(self.kf["nkeys"]), d_kf_point_index=p(self.kf["pidx"]),
                 d_kf_fv_nodes=p(self.kf["fv_nodes"]), d_kf_fv_offs=p(self.kf["fv_offs"]),
                 d_kf_fv_feats=p(self.kf["fv_feats"]), d_kf_n_fv_nodes=p(self.kf["n_fv_nodes"]),
                 d_f_keys=p(self.f["keys"]), d_f_desc=p(self.f["desc"]),
                 d_f_nkeys=p(self.f["nkeys"]), d_f_fv_nodes=p(self.f["fv_nodes"]),
                 d_f_fv_offs=p(self.f["fv_offs"]), d_f_fv_feats=p(self.f["fv_feats"]),
                 d_f_n_fv_nodes=p(self.f["n_fv_nodes"]), kp_stride=self.stride,
                 d_points=p(self.points), mp_stride=self.mp_stride, min_matches=min_matches,
                 d_kp_match=p(self.km), d_info=p(self.info), stream=stream)
        return a

    def launch(self, m, min_matches=0, stream=0, **over):
        m.search_by_bow_batch(**dict(self.args(min_matches, stream), **over))

    def results(self):
        self.torch.cuda.synchronize()
        return (self.km.cpu().numpy().reshape(self.P, self.stride),
                self.info.cpu().numpy().view(B.INFO_DTYPE).reshape(self.P))


def run(torch, oracle, m, probs, min_matches=0, stride=None, pairs=None, kf_sides=None,
        f_sides=None, points="own", edit=None, tag="", launch=True):
    """Problems on distinct slots (or, with kf_sides / f_sides / pairs, problems
    (ks, fs) over the given slots), compared with the reference.  points: "own"
    (each problem's array at p * mp_stride), an array shared by all, or None."""
    if kf_sides is None:
        kf_sides, f_sides = [p["kf"] for p in probs], [p["f"] for p in probs]
        pairs_ = [(i, i) for i in range(len(probs))]
    else:
        pairs_ = pairs
    P = len(pairs_)
    stride = stride or max(1, max(len(s["desc"]) for s in list(kf_sides) + list(f_sides)))
    ka, fa = B.pack_slots(kf_sides, stride), B.pack_slots(f_sides, stride)
    if edit:
        edit(ka, fa)
    if isinstance(points, str):
        plist = [p["points"] for p in probs]
        parr, mp_stride = B.pack_points(plist)
        pref = lambda p: parr[p * mp_stride:(p + 1) * mp_stride]
    elif points is None:
        parr, mp_stride, pref = None, 0, lambda p: None
    else:
        parr, mp_stride, pref = points, 0, lambda p: points
    ident = pairs is None
    d = Batch(torch, ka, fa, stride, P, parr, mp_stride, None if ident else [a for a, _ in pairs_],
              None if ident else [b for _, b in pairs_])
    if not launch:
        return d
    d.launch(m, min_matches)
    km, info = d.results()
    refs = reference(oracle, m, ka, fa, stride, pairs_, pref, min_matches)
    compare(km, info, fa, pairs_, refs, tag)
    return km, info, refs


def reference(oracle, m, ka, fa, stride, pairs, pref, min_matches, cache=None):
    cache = {} if cache is None else cache
    refs = []
    for p, (ks, fs) in enumerate(pairs):
        pts = pref(p)
        key = (ks, fs, None if pts is None else pts.tobytes())
        if key not in cache:
            cache[key] = B.expected_slot(oracle, ka, ks, fa, fs, stride, pts, m.mfNNratio,
                                         m.mbCheckOrientation, min_matches)
        refs.append(cache[key])
    return refs


def compare(km, info, fa, pairs, refs, tag=""):
    stride = km.shape[1]
    for p, ((_, fs), (rkm, rinfo)) in enumerate(zip(pairs, refs)):
        n = int(min(max(int(fa["nkeys"][fs]), 0), stride))
        B.check(km, info, p, n, rkm, rinfo, JUNK, tag)


# --------------------------------------------------------------------- sizes
def test_mixed_sizes_in_one_batch(torch, oracle, matchers):
    """bow_pair at 60 / 200 / 1000 features and the degenerate shapes, one stride."""
    tiny = tiny_problems(oracle)
    probs = [natural(oracle, 5, 60), tiny["no_kf_keypoints"], natural(oracle, 3, 200),
             tiny["no_f_keypoints"], tiny["no_nodes"], natural(oracle, 3, 1000),
             tiny["no_common_node"], tiny["one_each"], tiny["all_null"], tiny["all_bad"]]
    stride = max(len(s["desc"]) for p in probs for s in (p["kf"], p["f"])) + 3
    km, info, _ = run(torch, oracle, matchers[0.7, 1], probs, stride=stride, tag="mixed")
    assert info["n_matches"][[0, 2, 5]].min() >= 30 and info["n_matches"][5] > 250
    assert info["n_matches"][[1, 3, 4, 6, 8, 9]].tolist() == [0] * 6
    assert info["n_common_nodes"][[4, 6]].tolist() == [0, 0] and info["n_common_nodes"][8] > 30
    assert info["n_tried"][[8, 9]].tolist() == [0, 0]
    assert tuple(info[7]) == (1, 1, 1, 1, 1) and km[7, 0] == 3


def test_node_size_edges(torch, oracle, matchers):
    """Frame nodes of 1 / 63 / 64 / 65 / 128 / 129 / 200 features (register path,
    the 64-lane trips and ties across trips) and the histogram shapes in a
    70-feature node, against the oracle and the cases' own expectation."""
    probs = [edge_problem(n) for n in EDGE_NAMES]
    km, info, _ = run(torch, oracle, matchers[0.75, 1], probs, tag="edges 0.75")
    for p, name in enumerate(EDGE_NAMES):
        c = edge(name)
        if c["nnratio"] == 0.75:   # zero angles: the filter keeps every match of "nodes"
            assert np.array_equal(km[p, :len(c["expect"])], c["expect"]), name
            assert info[p]["n_matches"] == c["n_expect"], name
    km, info, _ = run(torch, oracle, matchers[1.25, 0], probs, tag="edges 1.25")
    c = edge("ties")
    p = EDGE_NAMES.index("ties")
    assert np.array_equal(km[p, :len(c["expect"])], c["expect"]) and c["n_expect"] >= 8
    assert info[p]["n_matches"] == c["n_expect"]


def test_node_size_edges_at_stride_8192(gpu, torch, oracle, matchers):
    """The transform's largest stride: dynamic LDS above 64 KiB."""
    assert gpu.match_bow_batch_max_stride() >= 8192
    probs = [edge_problem("nodes"), edge_problem("four_tied"), natural(oracle, 3, 200),
             edge_problem("eleven_two_one")]
    km, info, _ = run(torch, oracle, matchers[0.75, 1], probs, stride=8192, tag="8192")
    assert np.array_equal(km[0, :len(edge("nodes")["expect"])], edge("nodes")["expect"])
    run(torch, oracle, matchers[1.25, 1], [edge_problem("ties")] * 4, stride=8192, tag="8192 ties")


@pytest.mark.parametrize("n_problems", [1, 16, 300])
def test_batch_sizes(torch, oracle, matchers, n_problems):
    tiny = tiny_problems(oracle)
    pool = ([edge_problem(n) for n in EDGE_NAMES] + list(tiny.values())
            + [natural(oracle, 5, 60), natural(oracle, 3, 200), natural(oracle, 40, 200)])
    probs = [pool[(7 * i + 16) % len(pool)] for i in range(n_problems)]
    _, info, _ = run(torch, oracle, matchers[0.75, 1], probs, tag="batch %d" % n_problems)
    assert info["n_matches"].max() >= 30


# --------------------------------------------------------------- indirection
def reloc_set(oracle):
    return [natural(oracle, s, 200) for s in (3, 40, 41, 42)] + [
        B.thin_to(oracle, natural(oracle, 3, 200), n, 0.7, True) for n in (40, 30, 20, 14)]


def test_relocalisation_form(torch, oracle, matchers):
    """K = 8 keyframe slots against frame slot 0: own point arrays, then one shared."""
    probs = reloc_set(oracle)
    kfs, fr = [p["kf"] for p in probs], [probs[0]["f"]]
    pairs = [(k, 0) for k in range(8)]
    _, info, _ = run(torch, oracle, matchers[0.75, 1], probs, 15, pairs=pairs, kf_sides=kfs,
                     f_sides=fr, tag="reloc own")
    assert info["enough"].tolist() == [1, 0, 0, 0, 1, 1, 1, 0]
    shared = probs[0]["points"]
    assert all(len(p["points"]) <= len(shared) for p in probs)
    run(torch, oracle, matchers[0.75, 1], probs, 15, pairs=pairs, kf_sides=kfs, f_sides=fr,
        points=shared, tag="reloc shared")


def test_one_keyframe_against_many_frames_and_permuted_indices(torch, oracle, matchers):
    probs = reloc_set(oracle)
    kfs = [p["kf"] for p in probs]
    frames = [natural(oracle, s, 200)["f"] for s in (3, 40, 41, 42)] + [
        natural(oracle, 5, 60)["f"], edge_problem("nodes")["f"], natural(oracle, 3, 200)["f"],
        natural(oracle, 40, 200)["f"]]
    shared = probs[0]["points"]
    run(torch, oracle, matchers[0.7, 1], None, pairs=[(0, j) for j in range(8)], kf_sides=kfs[:1],
        f_sides=frames, points=shared, tag="one kf")
    pairs = [(5, 0), (0, 0), (5, 6), (3, 3), (0, 6), (7, 2), (5, 0), (1, 1), (0, 0)]
    _, info, _ = run(torch, oracle, matchers[0.7, 1], None, pairs=pairs, kf_sides=kfs,
                     f_sides=frames, points=shared, tag="permuted")
    assert info[1]["n_matches"] >= 30 and tuple(info[0]) == tuple(info[6])


def test_null_index_arrays_are_identity(torch, oracle, matchers):
    probs = reloc_set(oracle)[:5]
    kfs, fs = [p["kf"] for p in probs], [p["f"] for p in probs]
    a = run(torch, oracle, matchers[0.7, 1], probs, tag="null index")
    b = run(torch, oracle, matchers[0.7, 1], probs, pairs=[(i, i) for i in range(5)], kf_sides=kfs,
            f_sides=fs, tag="explicit identity")
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
    # the two sides in one allocation: slots 0-4 keyframes, 5-9 frames
    both = [dict(s, pidx=s.get("pidx", np.full(len(s["desc"]), -1, np.int32))) for s in kfs + fs]
    stride = max(len(s["desc"]) for s in both)
    arr = B.pack_slots(both, stride)
    parr, mps = B.pack_points([p["points"] for p in probs])
    d = Batch(torch, arr, arr, stride, 5, parr, mps, np.arange(5), np.arange(5) + 5)
    d.launch(matchers[0.7, 1])
    km, info = d.results()
    compare(km, info, arr, [(i, i + 5) for i in range(5)], a[2], "one allocation")


# ------------------------------------------------------------ point handling
def test_point_handling(torch, oracle, matchers):
    base = natural(oracle, 3, 200)
    live = np.nonzero(base["kf"]["pidx"] >= 0)[0]
    neg = base["kf"]["pidx"].copy()
    neg[live[0::3]], neg[live[1::3]] = -2, INT_MIN
    neg[live[2::6]] = -1
    dup = base["kf"]["pidx"].copy()
    dup[live[1::2]] = dup[live[0:len(live) // 2 * 2:2]]     # pairs of keypoints on one point
    clean = base["points"].copy()
    clean["bad"] = 0
    probs = [dict(base, kf=dict(base["kf"], pidx=neg)), dict(base, kf=dict(base["kf"], pidx=dup)),
             dict(base, points=clean)]
    km, info, _ = run(torch, oracle, matchers[0.7, 1], probs, tag="points")
    assert 0 < info[0]["n_tried"] < info[2]["n_tried"]
    vals, counts = np.unique(km[1][km[1] >= 0], return_counts=True)
    assert counts.max() == 2                                 # one point on two frame keypoints
    no_pts = run(torch, oracle, matchers[0.7, 1], probs, points=None, tag="d_points NULL")
    assert np.array_equal(no_pts[0][2], km[2]) and tuple(no_pts[1][2]) == tuple(info[2])
    assert no_pts[1][0]["n_tried"] >= info[0]["n_tried"]


# ---------------------------------------------------------------------- gate
@pytest.mark.parametrize("min_matches", [15, 0, 16])
def test_min_matches_gate(torch, oracle, matchers, min_matches):
    probs = [B.thin_to(oracle, natural(oracle, 3, 200), n, 0.7, True) for n in (14, 15)]
    probs.append(natural(oracle, 3, 200))
    km, info, refs = run(torch, oracle, matchers[0.7, 1], probs, min_matches, tag="gate")
    assert info["n_matches"].tolist()[:2] == [14, 15]
    for p, n in enumerate(info["n_matches"].tolist()):
        nf = len(probs[p]["f"]["desc"])
        assert int(info[p]["enough"]) == int(n >= min_matches)
        assert (km[p, :nf] == -1).all() == (n < min_matches)
        assert info[p]["n_accepted"] >= n > 0 and info[p]["n_tried"] > n


# ---------------------------------------------------------------- parameters
@pytest.mark.parametrize("ori", [0, 1])
@pytest.mark.parametrize("nnratio", [0.7, 0.75, 0.9])
def test_parameters(torch, oracle, matchers, nnratio, ori):
    probs = [natural(oracle, 3, 200), natural(oracle, 41, 200), edge_problem("ten_two_one")]
    _, info, _ = run(torch, oracle, matchers[nnratio, ori], probs, tag=(nnratio, ori))
    assert (info["n_accepted"] == info["n_matches"]).all() or ori


# ----------------------------------------------------------------- malformed
def test_malformed_slots_are_reported_not_read(torch, oracle, matchers):
    """In the middle of a batch, so that an unchecked read would stay inside
    the allocation: a feature index equal to the count, a last offset of
    count + 1, a decreasing offset; n_fv_nodes of -3 and stride + 9 are clamped."""
    good = natural(oracle, 3, 200)
    m = matchers[0.7, 1]
    for which, side_name in (("feat", "f"), ("last", "kf"), ("decrease", "f"), ("feat", "kf")):
        def edit(ka, fa, which=which, side_name=side_name):
            a = fa if side_name == "f" else ka
            s = len(a["fv_feats"]) // 5
            n, nn = int(a["nkeys"][2]), int(a["n_fv_nodes"][2])
            if which == "feat":
                a["fv_feats"][2 * s + n // 2] = n
            elif which == "last":
                a["fv_offs"][2 * (s + 1) + nn] = n + 1
            else:
                a["fv_offs"][2 * (s + 1) + nn // 2] = a["fv_offs"][2 * (s + 1) + nn // 2 - 1] - 1
        km, info, refs = run(torch, oracle, m, [good] * 5, edit=edit, tag=(which, side_name))
        assert refs[2][1] == B.MALFORMED and tuple(info[2]) == B.MALFORMED
        assert refs[1][1][0] >= 30 and tuple(info[1]) == tuple(info[3]) == refs[0][1]

    def clamp(ka, fa):
        s = len(fa["fv_feats"]) // 5
        fa["n_fv_nodes"][1] = -3
        # slot 3's node list goes on to its keypoint count with empty nodes of new ids:
        # clamped there it is the same problem, read any further it is malformed
        n, nn, b, ob = int(ka["nkeys"][3]), int(ka["n_fv_nodes"][3]), 3 * s, 3 * (s + 1)
        assert nn < n
        ka["fv_nodes"][b + nn:b + n] = 60000 + np.arange(n - nn)
        ka["fv_offs"][ob + nn + 1:ob + n + 1] = ka["fv_offs"][ob + nn]
        ka["n_fv_nodes"][3] = s + 9
    km, info, refs = run(torch, oracle, m, [good] * 5, edit=clamp, tag="clamped")
    assert tuple(info[1]) == (0, 0, 0, 0, 1)
    assert info[2]["n_matches"] >= 30 and tuple(info[3]) == tuple(info[2])


# -------------------------------------------------------------------- errors
def test_status_codes(gpu, torch, oracle, matchers):
    m = matchers[0.7, 1]
    p = natural(oracle, 5, 60)
    d = run(torch, oracle, m, [p, p], launch=False)
    cap = gpu.match_bow_batch_max_stride()

    def refused(status, matcher=m, **over):
        with pytest.raises(gpu.OrbError) as err:
            d.launch(matcher, **over)
        assert err.value.status == status, over
        km, info = d.results()
        assert (km == JUNK).all() and (info.view(np.int32) == JUNK).all(), over  # nothing ran

    refused(gpu.ORB_ECAPACITY, kp_stride=cap + 1)
    required = [k for k in d.args() if k.startswith("d_") and k not in ("d_kf_index", "d_f_index",
                                                                        "d_points")]
    assert len(required) == 17
    for over in [dict(n_problems=-1), dict(kp_stride=0), dict(kp_stride=-4), dict(mp_stride=-1)] + [
            {k: 0} for k in required]:
        refused(gpu.ORB_EINVAL, **over)
    for bad in (float("nan"), float("inf")):
        refused(gpu.ORB_EINVAL, matcher=gpu.ORBmatcher(bad, True))
    d.launch(m, n_problems=0)                     # fine, and nothing is launched
    km, info = d.results()
    assert (km == JUNK).all() and (info.view(np.int32) == JUNK).all()
    d.launch(m, n_problems=0, d_kp_match=0, d_info=0)
    d.launch(m)                                   # the handle still works
    km, info = d.results()
    assert info["n_matches"].tolist() == [B.expected(oracle, p, 0.7, True)[1][0]] * 2


# ------------------------------------------------------ one-problem equivalence
def test_equals_the_one_problem_entry(gpu, torch, oracle, matchers):
    m = matchers[0.75, 1]
    probs = [natural(oracle, 3, 200), natural(oracle, 5, 60), edge_problem("nodes"),
             edge_problem("four_tied")]
    km, info, _ = run(torch, oracle, m, probs, tag="vs one-problem")
    for p, q in enumerate(probs):
        kf, f = q["kf"], q["f"]
        mp = kf["pidx"]
        bad = np.where(mp >= 0, q["points"]["bad"][np.maximum(mp, 0)], 0).astype(np.uint8)
        n, fm = m.SearchByBoW(kf["desc"], kf["angle"], mp, bad, kf["fv"], f["desc"], f["angle"],
                              f["fv"])
        assert n == info[p]["n_matches"] and np.array_equal(fm, km[p, :len(fm)]), p


# --------------------------------------------------------------- two streams
def test_two_streams_no_synchronisation(gpu, torch, oracle):
    """Two handles on two streams alternate calls of different sizes with no
    host wait in between."""
    ma, mb = gpu.ORBmatcher(0.7, True), gpu.ORBmatcher(0.9, False)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    big = [natural(oracle, (3, 40, 41)[i % 3], 200) for i in range(64)]
    small = [edge_problem("nodes"), natural(oracle, 5, 60), edge_problem("ties")]
    d1, d2 = run(torch, oracle, ma, big, launch=False), run(torch, oracle, mb, small, launch=False)
    d3 = run(torch, oracle, ma, small, launch=False)
    torch.cuda.synchronize()
    d1.launch(ma, 15, stream=s1.cuda_stream)
    d2.launch(mb, 0, stream=s2.cuda_stream)
    d3.launch(ma, 0, stream=s1.cuda_stream)
    d2.launch(mb, 0, stream=s2.cuda_stream)
    d1.launch(ma, 0, stream=s1.cuda_stream)
    for d, m, probs, tag in ((d1, ma, big, "stream 1"), (d2, mb, small, "stream 2"),
                             (d3, ma, small, "stream 1 small")):
        km, info = d.results()
        cache = {}
        for p, q in enumerate(probs):
            if id(q) not in cache:
                cache[id(q)] = B.expected(oracle, q, m.mfNNratio, m.mbCheckOrientation)
            B.check(km, info, p, len(q["f"]["desc"]), *cache[id(q)], JUNK, tag)


# ------------------------------------------------------- discard entry points
def test_discard_entry_points_agree(gpu, torch, matchers):
    """track_discard_outliers_batch_n pointed at a FRAME_MATCH_INFO_DTYPE array's
    first field equals track_discard_outliers_batch; pointed at a plain int32
    array (stride 1) it reads that."""
    rng = np.random.default_rng(9)
    P, stride, mps = 6, 300, 200
    m = matchers[0.7, 1]
    km = np.where(rng.random((P, stride)) < 0.6, rng.integers(0, mps, (P, stride)), -1).astype(np.int32)
    ol = (rng.random((P, stride)) < 0.3).astype(np.uint8)
    pts = np.zeros((P, mps), R.MAP_POINT_DTYPE)
    pts["has_obs"], pts["bad"] = rng.random((P, mps)) < 0.7, rng.random((P, mps)) < 0.1
    nk = np.array([300, 0, 1, 64, 65, 257], np.int32)
    info = np.zeros(P, R.INFO_DTYPE)
    info["n_matches"] = 400 + np.arange(P)
    info["retried"] = 12345                      # the other fields are not the count
    outs = []
    for entry in ("struct", "strided", "plain"):
        d_km, d_ol, d_pts = _dev(torch, km).view(torch.int32), _dev(torch, ol), _dev(torch, pts)
        d_nk, d_info = _dev(torch, nk), _dev(torch, info)
        d_plain = _dev(torch, info["n_matches"].astype(np.int32))
        d_out = torch.full((P * 3,), JUNK, dtype=torch.int32, device="cuda")
        common = (P, d_nk.data_ptr(), stride, d_km.data_ptr(), d_ol.data_ptr(), d_pts.data_ptr(),
                  mps, 1)
        if entry == "struct":
            m.track_discard_outliers_batch(*common, d_info.data_ptr(), d_out.data_ptr())
        elif entry == "strided":
            m.track_discard_outliers_batch_n(*common, d_info.data_ptr(), 5, d_out.data_ptr())
        else:
            m.track_discard_outliers_batch_n(*common, d_plain.data_ptr(), 1, d_out.data_ptr())
        torch.cuda.synchronize()
        outs.append((d_km.cpu().numpy().tobytes(), d_ol.cpu().numpy().tobytes(),
                     d_pts.cpu().numpy().tobytes(), d_out.cpu().numpy().tobytes()))
    assert outs[0] == outs[1] == outs[2]
    g_out = np.frombuffer(outs[1][3], np.int32).view(R.DISCARD_DTYPE)
    for p in range(P):
        n = int(nk[p])
        rout = R.discard_outliers(km[p, :n], ol[p, :n], pts[p], 400 + p, True)[3]
        assert g_out[p].tolist() == rout.tolist(), p
    with pytest.raises(gpu.OrbError) as err:
        m.track_discard_outliers_batch_n(*common, d_info.data_ptr(), 0, d_out.data_ptr())
    assert err.value.status == gpu.ORB_EINVAL


# --------------------------------------------------------------------- chain
def test_reference_keyframe_chain_device_resident(gpu, torch, oracle):
    """TrackReferenceKeyFrame for four problems, every intermediate in device
    memory: ComputeBoW of four keyframes and four frames (transform_batch) ->
    SearchByBoW batch on its outputs -> PoseOptimization on the kp_match ->
    discard and mark (the strided count) -> isInFrustum at the optimised pose;
    each stage against its CPU reference on the previous reference's output."""
    import poseopt_cases as pc
    F, stride, NE, NK, W, H = 4, 2048, 60, 80, 1241, 376
    v = S.vocabulary(rng_seed=21, k=10, L=5)
    cam, levels, LS = pc.CAM, pc.INV_LEVEL_SIGMA2, f32(E.LS)
    desc = np.zeros((2 * F, stride, 32), np.uint8)
    keys = np.zeros((2 * F, stride), B.KEYPOINT_DTYPE)
    counts = np.zeros(2 * F, np.int32)
    pidx = np.full((F, stride), -1, np.int32)
    M = NE + 7
    Pall = np.zeros((F, M), gpu.MAP_POINT_DTYPE)
    pin = np.zeros(F, gpu.POSE_DTYPE)
    q = []
    for f in range(F):
        rng = np.random.default_rng(300 + f)
        c = pc.make_case(300 + f, NK, NE, "mono", noise=1.0, outlier_frac=0.2)
        kd = S.vocab_features(v, NE, rng_seed=40 + f)
        bits = np.unpackbits(kd, axis=1)
        noisy = np.packbits(bits ^ (rng.random(bits.shape) < 0.02).astype(np.uint8), axis=1)
        fd = S.vocab_features(v, NK, rng_seed=80 + f)
        order = rng.permutation(NE)              # keyframe keypoint of the j-th edge
        fd[c["slots"]] = noisy[order]
        fk = np.zeros(NK, B.KEYPOINT_DTYPE)
        for name in ("x", "y", "size", "octave", "class_id"):
            fk[name] = c["keys"][name]
        fk["angle"] = rng.uniform(0, 360, NK).astype(f32)
        ka = np.zeros(NE, f32)
        ka[order] = (fk["angle"][c["slots"]] + f32(10.0)) % f32(360.0)
        kp = np.full(NE, -1, np.int32)
        kp[order] = c["point_index"][c["slots"]]
        kp[rng.random(NE) < 0.05] = -1
        pts = np.zeros(M, gpu.MAP_POINT_DTYPE)
        pts["pos"] = c["points"]
        ow = c["pose"]["ow"][0]
        nrm = ow[None, :] - pts["pos"]
        pts["normal"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
        pts["min_distance"], pts["max_distance"] = 0.1, 1000.0
        pts["has_obs"] = rng.random(M) < 0.8
        pts["bad"] = rng.random(M) < 0.04
        desc[f, :NE], desc[F + f, :NK] = kd, fd
        keys[f]["angle"][:NE], keys[F + f][:NK] = ka, fk
        counts[f], counts[F + f] = NE, NK
        pidx[f, :NE], Pall[f], pin[f] = kp, pts, c["pose"][0]
        # references, stage by stage
        kfv, ffv = oracle.vocab_transform(v, kd, 4)[2:5], oracle.vocab_transform(v, fd, 4)[2:5]
        prob = dict(kf=B.side(kd, ka, kfv, kp), f=B.side(fd, fk["angle"], ffv), points=pts)
        km3, info3 = B.expected(oracle, prob, 0.75, True, 15)
        r4 = pc.ref.pose_optimization(np.stack([fk["x"], fk["y"]], 1), fk["octave"],
                                      np.full(NK, -1, f32), km3, pts["pos"], levels, cam,
                                      c["pose"]["rcw"][0], c["pose"]["tcw"][0], c["pose"]["ow"][0],
                                      np.full(NK, pc.SENTINEL, np.uint8))
        km5, ol5, P5, out5 = R.discard_outliers(km3, r4["outlier"], pts, info3[0], True)
        pose2 = np.zeros(1, gpu.POSE_DTYPE)
        pose2["rcw"], pose2["tcw"], pose2["ow"] = r4["rcw"], r4["tcw"], r4["ow"]
        n6, tr6 = oracle.frustum(P5, pose2, cam, W, H, 0.5, LS, 8)
        assert info3[0] >= 15 and info3[4] == 1 and r4["n_inliers"] >= 10
        q.append(dict(km3=km3, info3=info3, r4=r4, km5=km5, ol5=ol5, P5=P5, out5=out5, n6=n6,
                      tr6=tr6))
    assert sum(c["out5"]["n_discarded"] for c in q) > 0
    voc = gpu.ORBVocabulary(v["k"], v["L"], v["parent"], v["leaf"], v["desc"], v["weight"])
    z = lambda n, dt: torch.full((n,), -7, dtype=dt, device="cuda")
    n8 = 2 * F * stride
    d_desc, d_keys, d_counts = _dev(torch, desc), _dev(torch, keys), _dev(torch, counts)
    d_pidx, d_P, d_pin = _dev(torch, pidx), _dev(torch, Pall), _dev(torch, pin)
    fw, fwt, fn = z(n8, torch.int32), z(n8, torch.float64), z(n8, torch.int32)
    bw, bv, nw = z(n8, torch.int32), z(n8, torch.float64), z(2 * F, torch.int32)
    fvn, fvo, fvf, nfv = (z(n8, torch.int32), z(2 * F * (stride + 1), torch.int32),
                          z(n8, torch.int32), z(2 * F, torch.int32))
    d_km = torch.full((F, stride), JUNK, dtype=torch.int32, device="cuda")
    d_info3 = torch.zeros(F * 5, dtype=torch.int32, device="cuda")
    d_ur = torch.full((F * stride,), -1.0, dtype=torch.float32, device="cuda")
    d_pout = torch.zeros(F * gpu.POSE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_outl = torch.full((F * stride,), pc.SENTINEL, dtype=torch.uint8, device="cuda")
    d_info4 = torch.zeros(F * 4, dtype=torch.int32, device="cuda")
    d_out5 = torch.zeros(F * 3, dtype=torch.int32, device="cuda")
    d_nm = torch.full((F,), M, dtype=torch.int32, device="cuda")
    d_tr = torch.zeros(F * M * gpu.MP_TRACK_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_cnt6 = torch.zeros(F, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m = gpu.ORBmatcher(0.75, True)
    st = torch.cuda.Stream()
    s = st.cuda_stream
    fo = F * stride          # the frames are slots F..2F-1 of the transform's batch
    with torch.cuda.stream(st):
        voc.transform_batch(2 * F, d_counts.data_ptr(), d_desc.data_ptr(), stride, 4, fw.data_ptr(),
                            fwt.data_ptr(), fn.data_ptr(), bw.data_ptr(), bv.data_ptr(),
                            nw.data_ptr(), fvn.data_ptr(), fvo.data_ptr(), fvf.data_ptr(),
                            nfv.data_ptr(), stream=s)
        k_cur, n_cur = d_keys.data_ptr() + fo * 28, d_counts.data_ptr() + F * 4
        m.search_by_bow_batch(
            F, 0, 0, d_keys.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), d_pidx.data_ptr(),
            fvn.data_ptr(), fvo.data_ptr(), fvf.data_ptr(), nfv.data_ptr(),
            k_cur, d_desc.data_ptr() + fo * 32, n_cur, fvn.data_ptr() + fo * 4,
            fvo.data_ptr() + F * (stride + 1) * 4, fvf.data_ptr() + fo * 4, nfv.data_ptr() + F * 4,
            stride, d_P.data_ptr(), M, 15, d_km.data_ptr(), d_info3.data_ptr(), stream=s)
        km3 = d_km.clone()
        m.pose_optimization_batch(F, n_cur, k_cur, d_ur.data_ptr(), stride, d_km.data_ptr(),
                                  d_P.data_ptr(), gpu.MAP_POINT_DTYPE.itemsize, M, levels, cam,
                                  d_pin.data_ptr(), d_pout.data_ptr(), d_outl.data_ptr(),
                                  d_info4.data_ptr(), stream=s)
        m.track_discard_outliers_batch_n(F, n_cur, stride, d_km.data_ptr(), d_outl.data_ptr(),
                                         d_P.data_ptr(), M, True, d_info3.data_ptr(), 5,
                                         d_out5.data_ptr(), stream=s)
        m.frustum_batch(F, d_P.data_ptr(), d_nm.data_ptr(), M, d_pout.data_ptr(), cam, 0.0, float(W),
                        0.0, float(H), 0.5, LS, 8, d_tr.data_ptr(), d_cnt6.data_ptr(), stream=s)
    torch.cuda.synchronize()    # the one host wait
    g_km3, g_km5 = km3.cpu().numpy(), d_km.cpu().numpy()
    g_info3 = d_info3.cpu().numpy().view(B.INFO_DTYPE)
    g_pout = d_pout.cpu().numpy().view(gpu.POSE_DTYPE)
    g_outl = d_outl.cpu().numpy().reshape(F, stride)
    g_info4 = d_info4.cpu().numpy().view(gpu.POSE_OPT_INFO_DTYPE)
    g_out5 = d_out5.cpu().numpy().view(R.DISCARD_DTYPE)
    g_P = d_P.cpu().numpy().view(gpu.MAP_POINT_DTYPE).reshape(F, M)
    g_tr = d_tr.cpu().numpy().view(gpu.MP_TRACK_DTYPE).reshape(F, M)
    g_cnt6 = d_cnt6.cpu().numpy()
    for f, c in enumerate(q):
        B.check(g_km3, g_info3, f, NK, c["km3"], c["info3"], JUNK, ("bow", f))
        r4 = c["r4"]
        assert g_info4[f]["n_inliers"] == r4["n_inliers"], f
        assert g_pout[f]["rcw"].tobytes() == np.asarray(r4["rcw"], f32).tobytes(), f
        assert g_pout[f]["tcw"].tobytes() == np.asarray(r4["tcw"], f32).tobytes(), f
        assert np.array_equal(g_km5[f, :NK], c["km5"]) and (g_km5[f, NK:] == JUNK).all(), f
        assert np.array_equal(g_outl[f, :NK], c["ol5"]), f
        assert g_out5[f].tolist() == c["out5"].tolist(), f
        assert g_P[f].tobytes() == c["P5"].tobytes(), f
        assert g_cnt6[f] == c["n6"] and g_tr[f].tobytes() == c["tr6"].tobytes(), f
