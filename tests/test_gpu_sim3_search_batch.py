"""The device-batched SearchBySim3 (orb_search_by_sim3_batch, k_sim3_search_batch)
against the CPU: the C++ oracle's search_by_sim3 per problem on the slot arrays
read as the entry's contract says (tests/sim3_chain_ref.py), pyref's restatement
as the second statement.  The rows and d_new12 index-exact over KF1's count, all
five info fields exact, slots past the count and skipped problems byte-for-byte
untouched (0x5A sentinel)."""
import numpy as np
import pytest

import bow_batch_ref as B
import matcher_edge_cases as E
import pyref
import sim3_chain_cases as C
import sim3_chain_ref as R
import tri_batch_ref as T
from sim3_chain_cases import EDGE_HOST, Problem, ident, natural_rows, plain

pytestmark = pytest.mark.gpu
f32 = np.float32
SENT = 0x5A5A5A5A


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def matcher(gpu):
    return gpu.ORBmatcher(0.75, True)


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


# ------------------------------------------------------------------- harness
class Batch:
    def __init__(self, torch, sides, probs, points, mp_desc, stride=None, host=EDGE_HOST,
                 with_inliers=None, with_active=None, with_new=True, identity_slots=False):
        self.torch, self.probs, self.host = torch, probs, host
        self.points = np.ascontiguousarray(points, B.MAP_POINT_DTYPE)
        self.mp_desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        self.stride = stride = stride or max(1, max(len(s["desc"]) for s in sides))
        self.arr = T.pack_slots(sides, stride, with_u_right=False)
        P = self.P = len(probs)
        rows = {k: np.full((max(P, 1), stride), SENT, np.int32) for k in ("match12", "index2", "new12")}
        inl = np.full((max(P, 1), stride), 0x5A, np.uint8)
        for p, q in enumerate(probs):
            n = len(q.m12)
            rows["match12"][p, :n], rows["index2"][p, :n] = q.m12, q.ix2
            if q.inliers is not None:
                inl[p, :n] = q.inliers
        if with_inliers is None:
            with_inliers = any(q.inliers is not None for q in probs)
        if with_active is None:
            with_active = any(q.active != 1 for q in probs)
        if not with_new:
            del rows["new12"]
        self.before = {k: v.copy() for k, v in rows.items()}
        self.d = {k: _dev(torch, v) for k, v in self.arr.items() if v is not None}
        self.rows = {k: _dev(torch, v) for k, v in rows.items()}
        self.inl = _dev(torch, inl) if with_inliers else None
        self.s1 = None if identity_slots else _dev(torch, np.array([q.k1 for q in probs] or [0], np.int32))
        self.s2 = None if identity_slots else _dev(torch, np.array([q.k2 for q in probs] or [0], np.int32))
        self.sim3 = _dev(torch, np.array([q.sim3 for q in probs] or [R.sim3_record()],
                                         R.SIM3_RESULT_DTYPE))
        self.active = _dev(torch, np.array([q.active for q in probs] or [1], np.uint8)) \
            if with_active else None
        self.dpoints, self.dmp_desc = _dev(torch, self.points), _dev(torch, self.mp_desc)
        self.info = torch.full((max(P, 1) * 20,), 0x5A, dtype=torch.uint8, device="cuda")

    def args(self, stream=0):
        p = lambda t: 0 if t is None else t.data_ptr()
        d, h = self.d, self.host
        return dict(n_problems=self.P, d_kf1_slot=p(self.s1), d_kf2_slot=p(self.s2),
                    d_kf_keys=p(d["keys"]), d_kf_desc=p(d["desc"]), d_kf_nkeys=p(d["nkeys"]),
                    d_kf_point_index=p(d["pidx"]), d_kf_pose=p(d["pose"]), kp_stride=self.stride,
                    d_points=p(self.dpoints), d_mp_desc=p(self.dmp_desc),
                    d_match12=p(self.rows["match12"]), d_index2=p(self.rows["index2"]),
                    d_inliers12=p(self.inl), d_sim3=p(self.sim3), cam=h["cam"],
                    bounds=(0.0, float(h["width"]), 0.0, float(h["height"])),
                    scale_factors=h["scale"], log_scale_factor=float(h["log_scale"]),
                    d_info=p(self.info), th=h["th"], d_active=p(self.active),
                    d_new12=p(self.rows.get("new12")), stream=stream)

    def launch(self, m, stream=0, **over):
        m.search_by_sim3_batch(**dict(self.args(stream), **over))

    def results(self):
        self.torch.cuda.synchronize()
        rows = {k: v.cpu().numpy().view(np.int32).reshape(-1, self.stride)
                for k, v in self.rows.items()}
        return rows, self.info.cpu().numpy().view(R.SEARCH_INFO_DTYPE).reshape(-1)

    def reference(self, oracle, second=None):
        c = dict(probs=self.probs, stride=self.stride, points=self.points, mp_desc=self.mp_desc,
                 host=self.host, with_inliers=self.inl is not None,
                 with_active=self.active is not None)
        return C.search_refs(oracle, c, self.arr, second)

    def compare(self, refs, tag=""):
        rows, info = self.results()
        for p, (q, want) in enumerate(zip(self.probs, refs)):
            n = int(min(max(int(self.arr["nkeys"][q.k1]), 0), self.stride))
            R.check_sim3(rows, info, p, n, self.before, want, 0x5A, tag)
        return rows, info


def run(torch, oracle, m, sides, probs, points, mp_desc, second=None, tag="", **kw):
    b = Batch(torch, sides, probs, points, mp_desc, **kw)
    b.launch(m)
    refs = b.reference(oracle, second)
    rows, info = b.compare(refs, tag)
    return b, refs, rows, info


def run_set(torch, oracle, m, c, second=None, tag=""):
    """A sim3_chain_cases search set through the entry, compared with the reference."""
    return run(torch, oracle, m, c["sides"], c["probs"], c["points"], c["mp_desc"], second, tag,
               stride=c["stride"], host=c["host"], with_inliers=c["with_inliers"],
               with_active=c["with_active"])


# --------------------------------------------------------------------- tests
@pytest.mark.parametrize("with_masks", (True, False))
def test_crowded_keyframes_with_and_without_masks(torch, oracle, matcher, with_masks):
    c = C.search_crowd_set(with_masks)
    _, refs, _, info = run_set(torch, oracle, matcher, c, tag="crowd")
    assert refs[0][3][0] >= 20 and info["n_best12"][0] > info["n_found"][0]
    run_set(torch, oracle, matcher, c, pyref.search_by_sim3, "crowd/pyref")


def test_thresholds_bounds_and_first_minimum(torch, oracle, matcher):
    expect = E.by_sim3_thresholds()["expect"]
    _, refs, rows, _ = run_set(torch, oracle, matcher, C.search_thresholds_set(), tag="thresholds")
    assert np.array_equal(rows["new12"][0, :len(expect)], expect)


def test_empty_keyframes(torch, oracle, matcher):
    sets = C.search_empty_sets()
    assert len(sets) == 2
    for c in sets:
        _, refs, _, info = run_set(torch, oracle, matcher, c, tag="empty")
        assert tuple(info[0]) == (0, 0, 0, 0, 0)


def test_keypoint_counts_in_one_batch(torch, oracle, matcher):
    _, refs, _, _ = run_set(torch, oracle, matcher, C.search_counts_set(), tag="counts")
    assert sum(r[3][0] for r in refs) > 50


def test_one_cell_borders_and_clamped_windows(torch, oracle, matcher):
    for name, c in C.search_grid_sets().items():
        _, refs, _, _ = run_set(torch, oracle, matcher, c, tag=name)
        assert refs[0][3][3] > 0 and refs[0][3][0] > 0, name


@pytest.mark.parametrize("s12,rotated", C.SIMILARITIES)
def test_natural_keyframes_under_similarities(torch, oracle, matcher, s12, rotated):
    _, refs, _, _ = run_set(torch, oracle, matcher, C.search_natural_set(oracle, s12, rotated),
                            tag="natural")
    assert refs[0][3][0] > 5 and refs[0][3][3] > refs[0][3][0]


def test_inlier_filter_and_index2_range(torch, oracle, matcher):
    c, n_have = C.search_filter_set(oracle)
    _, refs, _, info = run_set(torch, oracle, matcher, c, tag="filter")
    assert info["n_kept"][2] == 0 and 0 < info["n_kept"][3] < info["n_kept"][1] == n_have
    # without the inlier array nothing is filtered
    run_set(torch, oracle, matcher, C.search_no_filter_set(oracle), tag="no filter")


@pytest.mark.parametrize("P", (1, 16, 300))
def test_skipped_problems_stay_untouched_in_mixed_batches(torch, oracle, matcher, P):
    _, refs, _, _ = run_set(torch, oracle, matcher, C.search_mixed_set(oracle, P), tag="batch%d" % P)
    assert P == 1 or (any(r is None for r in refs) and any(r is not None for r in refs))


def test_stride_new12_and_the_one_problem_entry(torch, gpu, oracle, matcher):
    (s1, s2), points, mp_desc, host, rec, m12, ix2 = natural_rows(oracle)
    for c in C.search_stride_sets(oracle):
        run_set(torch, oracle, matcher, c, tag="stride%d" % c["stride"])
    b, refs, rows, _ = run(torch, oracle, matcher, [s1, s2], [Problem(0, 1, m12, ix2, rec)],
                           points, mp_desc, host=host, with_new=False, tag="no new12")
    c = C.search_identity_set(oracle)
    run(torch, oracle, matcher, c["sides"], c["probs"], c["points"], c["mp_desc"], host=c["host"],
        identity_slots=True, tag="identity slots")
    # d_new12 is orb_search_by_sim3's match12 on the same inputs
    a1, a2 = R.already_masks(m12, ix2, len(s2["desc"]))
    k1, k2 = R.kf_dict(s1, points, mp_desc, a1, host), R.kf_dict(s2, points, mp_desc, a2, host)
    fr = lambda k: gpu.Frame(k["keys"], k["desc"], k["scale"], k["width"], k["height"])
    nf, f12 = matcher.SearchBySim3(fr(k1), fr(k2), float(host["log_scale"]), host["cam"], k1["Rw"],
                                   k1["tw"], k2["Rw"], k2["tw"], k1["mps"], k1["valid"],
                                   k1["already"], k1["mp_desc"], k2["mps"], k2["valid"],
                                   k2["already"], k2["mp_desc"], float(rec["scale"]),
                                   rec["R"].reshape(3, 3), rec["t"], 7.5)
    assert nf == refs[0][3][0] and np.array_equal(f12, refs[0][2])


def test_two_streams_on_one_handle(torch, oracle, matcher):
    (s1, s2), points, mp_desc, host, rec, m12, ix2 = natural_rows(oracle)
    probs = [Problem(0, 1, m12, ix2, rec)] * 8
    a = Batch(torch, [s1, s2], probs, points, mp_desc, host=host)
    b = Batch(torch, [s1, s2], probs, points, mp_desc, host=host)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a.launch(matcher, stream=sa.cuda_stream)
    b.launch(matcher, stream=sb.cuda_stream)
    refs = a.reference(oracle)
    a.compare(refs, "stream a")
    b.compare(refs, "stream b")


def test_status_codes_and_capacity(torch, gpu, oracle, matcher):
    s1, s2, points, mp_desc, m12, ix2 = C.crowd(True)
    b = Batch(torch, [s1, s2], [Problem(0, 1, m12, ix2, ident())], points, mp_desc)
    cap = gpu.search_by_sim3_batch_max_stride()
    assert cap >= gpu.optimize_sim3_max_stride()
    for over, status in ((dict(kp_stride=0), gpu.ORB_EINVAL), (dict(n_problems=-1), gpu.ORB_EINVAL),
                         (dict(d_kf_keys=0), gpu.ORB_EINVAL), (dict(d_mp_desc=0), gpu.ORB_EINVAL),
                         (dict(d_info=0), gpu.ORB_EINVAL), (dict(scale_factors=[]), gpu.ORB_EINVAL),
                         (dict(scale_factors=np.ones(17, f32)), gpu.ORB_EINVAL),
                         (dict(bounds=(0.0, 0.0, 0.0, 480.0)), gpu.ORB_EINVAL),
                         (dict(bounds=(0.0, 640.0, 480.0, 480.0)), gpu.ORB_EINVAL),
                         (dict(bounds=(0.0, 640.0, 10.0, 5.0)), gpu.ORB_EINVAL),
                         (dict(kp_stride=cap + 1), gpu.ORB_ECAPACITY)):
        with pytest.raises(gpu.OrbError) as e:
            b.launch(matcher, **over)
        assert e.value.status == status, over
    b.launch(matcher, n_problems=0)
    rows, info = b.results()
    assert all((rows[k] == b.before[k]).all() for k in rows)
    assert (info.view(np.uint8) == 0x5A).all()
