"""The device-batched SearchByBoW(pKF1, pKF2, vpMatches12) (orb_match_bow_kf_batch,
k_bow_kf_batch) against the CPU: the C++ oracle's search_by_bow_kf per problem
on the slot arrays read as the entry's contract says (tests/sim3_chain_ref.py),
pyref's restatement as the second statement.  Both rows index-exact over KF1's
count, all five info fields exact, slots past the count untouched (0x5A
sentinel)."""
import numpy as np
import pytest

import bow_batch_ref as B
import matcher_edge_cases as E
import pyref
import sim3_chain_cases as C
import sim3_chain_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
SENT = 0x5A5A5A5A


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def matchers(gpu):
    return {(r, o): gpu.ORBmatcher(r, bool(o)) for r in (0.6, 0.75, 0.9, 1.25) for o in (0, 1)}


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


# ------------------------------------------------------------------- harness
class Batch:
    def __init__(self, torch, arr, stride, pairs, points, identity_slots=False):
        self.torch, self.arr, self.stride, self.pairs, self.points = torch, arr, stride, pairs, points
        P = self.P = len(pairs)
        self.d = {k: _dev(torch, v) for k, v in arr.items()}
        self.s1 = None if identity_slots else _dev(torch, np.array([a for a, _ in pairs] or [0], np.int32))
        self.s2 = None if identity_slots else _dev(torch, np.array([b for _, b in pairs] or [0], np.int32))
        self.dpoints = None if points is None else _dev(torch, points)
        self.m12 = torch.full((max(P, 1) * stride,), SENT, dtype=torch.int32, device="cuda")
        self.ix2 = torch.full((max(P, 1) * stride,), SENT, dtype=torch.int32, device="cuda")
        self.info = torch.full((max(P, 1) * 20,), 0x5A, dtype=torch.uint8, device="cuda")

    def args(self, min_matches=0, stream=0):
        p = lambda t: 0 if t is None else t.data_ptr()
        d = self.d
        return dict(n_problems=self.P, d_kf1_slot=p(self.s1), d_kf2_slot=p(self.s2),
                    d_kf_keys=p(d["keys"]), d_kf_desc=p(d["desc"]), d_kf_nkeys=p(d["nkeys"]),
                    d_kf_point_index=p(d["pidx"]), d_kf_fv_nodes=p(d["fv_nodes"]),
                    d_kf_fv_offs=p(d["fv_offs"]), d_kf_fv_feats=p(d["fv_feats"]),
                    d_kf_n_fv_nodes=p(d["n_fv_nodes"]), kp_stride=self.stride,
                    d_points=p(self.dpoints), min_matches=min_matches, d_match12=p(self.m12),
                    d_index2=p(self.ix2), d_info=p(self.info), stream=stream)

    def launch(self, m, min_matches=0, stream=0, **over):
        m.search_by_bow_kf_batch(**dict(self.args(min_matches, stream), **over))

    def results(self):
        self.torch.cuda.synchronize()
        sh = (-1, self.stride)
        return (self.m12.cpu().numpy().reshape(sh), self.ix2.cpu().numpy().reshape(sh),
                self.info.cpu().numpy().view(B.INFO_DTYPE).reshape(-1))

    def reference(self, oracle, nnratio, ori, min_matches=0, second=None):
        c = dict(pairs=self.pairs, points=self.points, nnratio=nnratio, ori=ori,
                 min_matches=min_matches)
        return C.bow_refs(oracle, c, self.arr, self.stride, second)

    def compare(self, refs, tag=""):
        m12, ix2, info = self.results()
        for p, ((k1, _), want) in enumerate(zip(self.pairs, refs)):
            n = int(min(max(int(self.arr["nkeys"][k1]), 0), self.stride))
            R.check_bow(m12, ix2, info, p, n, want, SENT, tag)
        return m12, ix2, info


def run(torch, oracle, matchers, c, second=None, tag="", **kw):
    """A sim3_chain_cases BoW set through the entry, compared with the reference."""
    arr, stride = C.bow_pack(c)
    b = Batch(torch, arr, stride, c["pairs"], c["points"], **kw)
    b.launch(matchers[(c["nnratio"], int(c["ori"]))], c["min_matches"])
    refs = b.reference(oracle, c["nnratio"], c["ori"], c["min_matches"], second)
    return (b, refs) + b.compare(refs, tag)


# --------------------------------------------------------------------- tests
def test_node_sizes_claims_and_thresholds(torch, oracle, matchers):
    """Nodes of 1 / 63 / 64 / 65 / 128 / 129 / 200 features, claims inside a node
    (later probes see earlier vbMatched2) and the distances 49 / 50 / 51: the
    directed case's own expectation, the oracle and pyref."""
    case = E.bow_case("kf")
    c = C.bow_edge_set("nodes", case["nnratio"], False)
    _, refs, m12, ix2, info = run(torch, oracle, matchers, c, tag="nodes")
    assert np.array_equal(m12[0, :len(case["expect"])], case["expect"])
    assert info["n_matches"][0] == case["n_expect"]
    run(torch, oracle, matchers, c, pyref.search_by_bow_kf, "nodes/pyref")


def test_ties_take_the_first_minimum(torch, oracle, matchers):
    case = E.bow_case("kf", ties=True)
    _, _, m12, _, info = run(torch, oracle, matchers, C.bow_edge_set("ties", 1.25, False), tag="ties")
    assert np.array_equal(m12[0, :len(case["expect"])], case["expect"])


@pytest.mark.parametrize("shape", tuple(E.HIST_SHAPES))
def test_rotation_histogram_shapes(torch, oracle, matchers, shape):
    _, refs, _, _, info = run(torch, oracle, matchers, C.bow_edge_set(shape), tag=shape)
    assert info["n_accepted"][0] >= info["n_matches"][0] > 0


@pytest.mark.parametrize("nnratio", (0.6, 0.9))
@pytest.mark.parametrize("ori", (False, True))
def test_natural_keyframes_nnratio_and_orientation(torch, oracle, matchers, nnratio, ori):
    c = C.bow_natural_set(oracle, nnratio, ori)
    _, refs, _, _, info = run(torch, oracle, matchers, c, tag="natural")
    assert info["n_matches"][0] > 20
    run(torch, oracle, matchers, c, pyref.search_by_bow_kf, "natural/pyref")


def test_empty_keyframes_and_feature_vectors(torch, oracle, matchers):
    _, _, _, _, info = run(torch, oracle, matchers, C.bow_empty_set(), tag="empty")
    assert (info["n_matches"][:6] == 0).all() and info["n_matches"][6] > 0


def test_bad_and_null_points_on_either_side_and_no_point_array(torch, oracle, matchers):
    _, refs, _, _, info = run(torch, oracle, matchers, C.bow_bad_null_set(oracle), tag="bad")
    assert info["n_tried"][1] < info["n_tried"][0]
    # d_points NULL: no point is bad
    _, refs0, _, _, info0 = run(torch, oracle, matchers, C.bow_no_points_set(oracle),
                                tag="no points")
    assert info0["n_matches"][0] > info["n_matches"][0]


@pytest.mark.parametrize("P", (1, 16, 300))
def test_mixed_batches_share_the_current_keyframe(torch, oracle, matchers, P):
    run(torch, oracle, matchers, C.bow_mixed_set(oracle, P), tag="mixed%d" % P)


def test_gate_at_19_and_20(torch, oracle, matchers):
    c = C.bow_gate_set(oracle)
    _, refs, m12, ix2, info = run(torch, oracle, matchers, c, tag="gate")
    assert [tuple(info[p])[0] for p in (0, 1)] == [19, 20]
    assert [int(info["enough"][p]) for p in (0, 1)] == [0, 1]
    n1 = len(c["sides"][0]["desc"])
    assert (m12[0, :n1] == -1).all() and (ix2[0, :n1] == -1).all() and (m12[1, :n1] >= 0).sum() == 20


@pytest.mark.parametrize("kind", tuple(C.MALFORMED))
def test_malformed_slots_in_the_middle_of_a_batch(torch, oracle, matchers, kind):
    # the clamped slots make different problems of (0, 1): keep them apart
    _, refs, _, _, info = run(torch, oracle, matchers, C.bow_malformed_set(oracle, kind), tag=kind)
    assert [int(v) for v in info["n_matches"][1:4]] == [-1, -1, -1]
    assert info["n_matches"][0] == 0 and info["n_matches"][4] > 0


def test_smallest_stride_and_one_more(torch, oracle, matchers):
    a, b, ident = C.bow_stride_sets()
    run(torch, oracle, matchers, a, tag="stride")
    run(torch, oracle, matchers, b, tag="stride + 1")
    run(torch, oracle, matchers, ident, tag="identity slots", identity_slots=True)


def test_equals_the_one_problem_entry(torch, oracle, matchers):
    s1, s2, pts = C.bow_natural(oracle)
    m = matchers[(0.75, 1)]
    _, refs, m12, _, info = run(torch, oracle, matchers, C.bow_set([s1, s2], [(0, 1)], pts), tag="one")
    bad = lambda s: R._bad_of(s["pidx"], pts)
    nm, row = m.SearchByBoWKF(s1["desc"], s1["angle"], s1["pidx"], bad(s1), s1["fv"], s2["desc"],
                              s2["angle"], s2["pidx"], bad(s2), s2["fv"])
    assert nm == info["n_matches"][0] and np.array_equal(row, m12[0, :len(row)])


def test_two_streams_on_one_handle(torch, oracle, matchers):
    s1, s2, pts = C.bow_natural(oracle)
    arr = B.pack_slots([s1, s2], max(len(s1["desc"]), len(s2["desc"])))
    a = Batch(torch, arr, len(arr["pidx"]) // 2, [(0, 1)] * 8, pts)
    b = Batch(torch, arr, len(arr["pidx"]) // 2, [(1, 0)] * 8, pts)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    m = matchers[(0.75, 1)]
    a.launch(m, stream=sa.cuda_stream)
    b.launch(m, stream=sb.cuda_stream)
    a.compare(a.reference(oracle, 0.75, True), "stream a")
    b.compare(b.reference(oracle, 0.75, True), "stream b")


def test_status_codes_and_capacity(torch, gpu, oracle, matchers):
    s1, s2, pts = C.bow_edge("nodes")
    stride = max(len(s1["desc"]), len(s2["desc"]))
    b = Batch(torch, B.pack_slots([s1, s2], stride), stride, [(0, 1)], pts)
    m = matchers[(0.75, 1)]
    cap = gpu.match_bow_kf_batch_max_stride()
    for over, status in ((dict(kp_stride=0), gpu.ORB_EINVAL), (dict(n_problems=-1), gpu.ORB_EINVAL),
                         (dict(d_kf_desc=0), gpu.ORB_EINVAL), (dict(d_index2=0), gpu.ORB_EINVAL),
                         (dict(d_info=0), gpu.ORB_EINVAL),
                         (dict(kp_stride=cap + 1), gpu.ORB_ECAPACITY)):
        with pytest.raises(gpu.OrbError) as e:
            b.launch(m, **over)
        assert e.value.status == status, over
    odd = gpu.ORBmatcher(0.75, True)
    for v in (float("nan"), float("inf"), float("-inf")):     # nnratio not finite
        odd.mfNNratio = v
        with pytest.raises(gpu.OrbError) as e:
            b.launch(odd)
        assert e.value.status == gpu.ORB_EINVAL, v
    b.launch(m, n_problems=0)
    m12, ix2, info = b.results()
    assert (m12 == SENT).all() and (ix2 == SENT).all() and (info.view(np.uint8) == 0x5A).all()
