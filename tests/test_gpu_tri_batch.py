"""The device-batched SearchForTriangulation (orb_search_for_triangulation_batch,
k_tri_batch) against the CPU: the C++ oracle's search_for_triangulation per
problem on the slot arrays read as the entry's contract says
(tests/tri_batch_ref.py), pyref's restatement as the second statement.  The
match12 row index-exact over KF1's count, all six info fields exact, slots past
the count and the neighbours' untouched; and the chain matcher -> new points on
one stream with no host copy between the two, KF2's point_index row included
where several accepted matches name one KF2 keypoint."""
import functools

import numpy as np
import pytest

import bow_batch_ref as B
import matcher_edge_cases as E
import newpoints_cases as C
import newpoints_ref as R
import pyref
import scenarios as S
import tri_batch_ref as T
from test_gpu_newpoints import run_group, same_f, same_rec

pytestmark = pytest.mark.gpu
f32 = np.float32
JUNK = 77
EDGE_HOST = (E.CAM, E.SCALE, E.SIGMA2)     # the host values the directed cases are built for
FLAGS = ((False, True), (True, False), (False, False))   # (only_stereo, check_orientation)


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def matchers(gpu):
    return {o: gpu.ORBmatcher(0.6, bool(o)) for o in (False, True)}


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


# -------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def edge(name):
    """Directed cases: node sizes 1 .. 200, ties across the 64-lane trips, the
    thresholds and gates (matcher_edge_cases.tri_case), the histogram shapes."""
    if name == "geometry":
        return E.tri_case()
    if name == "ties":
        return E.tri_case(ties=True)
    if name == "plain":
        return E.tri_case(geometry=False)
    return E.hist_bow(name, form="kf")


EDGE_NAMES = ("geometry", "ties", "plain") + tuple(E.HIST_SHAPES)


@functools.lru_cache(maxsize=None)
def edge_problem(name):
    return T.from_tri_case(edge(name))


@functools.lru_cache(maxsize=None)
def natural(oracle, seed, rng_seed, frac, nf=1000):
    """scenarios.keyframe_pair with the baseline of test_gpu_matchers_f, has_mp
    from point_index at `frac`."""
    k0, k1 = S.keyframe_pair(oracle, seed, rng_seed=rng_seed, baseline=(0.5, 0.0, 0.1), nf=nf)
    rng = np.random.default_rng(16)
    pidx = [np.where(rng.random(len(k["keys"])) < frac, np.arange(len(k["keys"])), -1)
            .astype(np.int32) for k in (k0, k1)]
    return T.from_keyframes(oracle, k0, k1, *pidx), (S.camera(), k1["scale"], k1["sigma2"])


# ------------------------------------------------------------------- harness
class Batch:
    """Device copies of packed slots and the per-problem arrays; outputs JUNK."""

    def __init__(self, torch, arr, stride, pairs, f12, host=EDGE_HOST):
        self.torch, self.P, self.stride, self.host = torch, len(pairs), stride, host
        self.d = {k: None if v is None else _dev(torch, v) for k, v in arr.items()}
        self.s1 = _dev(torch, np.array([a for a, _ in pairs], np.int32))
        self.s2 = _dev(torch, np.array([b for _, b in pairs], np.int32))
        self.f12 = _dev(torch, np.asarray(f12, f32).reshape(-1, 9))
        self.m12 = torch.full((max(self.P, 1) * stride,), JUNK, dtype=torch.int32, device="cuda")
        self.info = torch.full((max(self.P, 1) * 6,), JUNK, dtype=torch.int32, device="cuda")

    def args(self, only_stereo=False, stream=0):
        p = lambda t: 0 if t is None else t.data_ptr()
        d = self.d
        return dict(n_problems=self.P, d_kf1_slot=p(self.s1), d_kf2_slot=p(self.s2),
                    d_kf_keys=p(d["keys"]), d_kf_desc=p(d["desc"]), d_kf_nkeys=p(d["nkeys"]),
                    d_kf_point_index=p(d["pidx"]), d_kf_fv_nodes=p(d["fv_nodes"]),
                    d_kf_fv_offs=p(d["fv_offs"]), d_kf_fv_feats=p(d["fv_feats"]),
                    d_kf_n_fv_nodes=p(d["n_fv_nodes"]), d_kf_u_right=p(d["u_right"]),
                    d_kf_pose=p(d["pose"]), kp_stride=self.stride, d_f12=p(self.f12),
                    cam2=self.host[0], scale_factors=self.host[1], level_sigma2=self.host[2],
                    only_stereo=only_stereo, d_match12=p(self.m12), d_info=p(self.info),
                    stream=stream)

    def launch(self, m, only_stereo=False, stream=0, **over):
        m.search_for_triangulation_batch(**dict(self.args(only_stereo, stream), **over))

    def results(self):
        self.torch.cuda.synchronize()
        return (self.m12.cpu().numpy().reshape(-1, self.stride)[:max(self.P, 1)],
                self.info.cpu().numpy().view(T.INFO_DTYPE).reshape(-1))


def reference(oracle, arr, stride, pairs, f12, host, only_stereo, ori, second=None):
    cache, refs = {}, []
    for p, (k1, k2) in enumerate(pairs):
        key = (k1, k2, np.asarray(f12[p], f32).tobytes())
        if key not in cache:
            cache[key] = T.expected_slot(oracle, arr, k1, k2, f12[p], stride, *host, only_stereo,
                                         ori, second)
        refs.append(cache[key])
    return refs


def compare(m12, info, arr, stride, pairs, refs, tag=""):
    for p, ((k1, _), (row, want)) in enumerate(zip(pairs, refs)):
        n = int(min(max(int(arr["nkeys"][k1]), 0), stride))
        T.check(m12, info, p, n, row, want, JUNK, tag)


def run(torch, oracle, m, sides, pairs, f12, only_stereo=False, stride=None, host=EDGE_HOST,
        edit=None, with_u_right=True, second=None, tag="", launch=True):
    """Problems (KF1 slot, KF2 slot) over `sides`, compared with the reference."""
    stride = stride or max(1, max(len(s["desc"]) for s in sides))
    arr = T.pack_slots(sides, stride, with_u_right)
    if edit:
        edit(arr)
    d = Batch(torch, arr, stride, pairs, f12, host)
    if not launch:
        return d
    d.launch(m, only_stereo)
    m12, info = d.results()
    refs = reference(oracle, arr, stride, pairs, f12, host, only_stereo, m.mbCheckOrientation,
                     second)
    compare(m12, info, arr, stride, pairs, refs, tag)
    return m12, info, refs


def separate(problems):
    """Each (side1, side2, F12) on two slots of its own."""
    sides, pairs, f12 = [], [], []
    for s1, s2, f in problems:
        pairs.append((len(sides), len(sides) + 1))
        sides += [s1, s2]
        f12.append(f)
    return sides, pairs, np.stack(f12) if f12 else np.zeros((0, 9), f32)


# ------------------------------------------------------------ directed cases
@pytest.mark.parametrize("extra", [0, 1])
def test_directed_cases(torch, oracle, matchers, extra):
    """Every directed case in one batch at the smallest stride that holds the
    largest one, and at that stride + 1, under the three flag pairs."""
    sides, pairs, f12 = separate([edge_problem(n) for n in EDGE_NAMES])
    stride = max(len(s["desc"]) for s in sides) + extra
    for only_stereo, ori in FLAGS:
        m12, info, _ = run(torch, oracle, matchers[ori], sides, pairs, f12, only_stereo, stride,
                           tag=("directed", only_stereo, ori))
        for p, name in enumerate(EDGE_NAMES):
            want = edge(name)["expect"]
            if not only_stereo and (ori or name in ("geometry", "ties", "plain")):
                assert np.array_equal(m12[p, :len(want)], want), (name, only_stereo, ori)
        if not only_stereo:
            assert info["n_matches"][:3].min() >= 12 and info["n_shared2"][0] > 0
    # the restatement in Python says the same of the geometry and the tie cases
    run(torch, oracle, matchers[True], sides[:4], pairs[:2], f12[:2], stride=stride,
        second=pyref.search_for_triangulation, tag="directed, pyref")


# ------------------------------------------------------------- natural pairs
@pytest.mark.parametrize("only_stereo,ori", FLAGS)
def test_natural_pairs(torch, oracle, matchers, only_stereo, ori):
    """keyframe_pair (3, 1) and (7, 2), has_mp at 0 % and 50 %: ~1,000 keypoints,
    ~125 natural nodes, 31 to 462 matches.  One KF2 keypoint is the match of
    several KF1 keypoints in every run but one."""
    probs, host = [], None
    for seed, rs in ((3, 1), (7, 2)):
        for frac in (0.0, 0.5):
            q, host = natural(oracle, seed, rs, frac)
            probs.append(q)
    sides, pairs, f12 = separate(probs)
    m12, info, refs = run(torch, oracle, matchers[ori], sides, pairs, f12, only_stereo, host=host,
                          tag=("natural", only_stereo, ori))
    clean = 0
    for p, (row, want) in enumerate(refs):
        shared = T.shared_count(row)                 # from the oracle's row
        assert info[p]["n_shared2"] == shared == want[4], p
        if shared > 0:
            assert info[p]["n_shared2"] > 0, p
        clean += shared == 0
        assert info[p]["n_matches"] >= 31 and info[p]["n_undefined"] == 0
    # only (3, 1), only_stereo, 50 % has no shared KF2 keypoint (31 matches)
    assert clean == (1 if only_stereo else 0)
    if only_stereo:
        assert refs[1][1][0] == 31 and refs[1][1][4] == 0


# --------------------------------------------------------------- batch sizes
def mixed_pool(oracle):
    """Slots and (KF1, KF2, F12) problems of mixed sizes: the directed cases, a
    natural pair of 200 features, an empty KF1, an empty KF2, no common node,
    and slots that serve many problems on either side."""
    g1, g2, fe = edge_problem("geometry")
    t1, t2, _ = edge_problem("ties")
    (n1, n2, fn), _ = natural(oracle, 3, 1, 0.5, 200)
    none = T.empty_side()
    apart = dict(g1, fv=(g1["fv"][0] + 100000,) + g1["fv"][1:])
    sides = [g1, g2, t1, t2, n1, n2, none, apart]
    problems = [(0, 1, fe), (2, 3, fe), (4, 5, fn), (6, 1, fe), (0, 6, fe), (7, 1, fe), (2, 1, fe),
                (0, 3, fe), (5, 4, fn), (4, 1, fn), (0, 5, fe), (1, 3, fe), (6, 6, fe)]
    return sides, problems


@pytest.mark.parametrize("n_problems", [1, 16, 300])
def test_batch_sizes(torch, oracle, matchers, n_problems):
    sides, pool = mixed_pool(oracle)
    idx = [(7 * i) % len(pool) for i in range(n_problems)]
    probs = [pool[k] for k in idx]
    pairs, f12 = [(a, b) for a, b, _ in probs], np.stack([f for _, _, f in probs])
    m12, info, _ = run(torch, oracle, matchers[True], sides, pairs, f12,
                       tag="batch %d" % n_problems)
    assert info["n_matches"][0] >= 40
    if n_problems >= 16:
        by = {k: idx.index(k) for k in range(len(pool))}
        assert [tuple(info[by[k]]) for k in (3, 4, 5, 12)] == [(0,) * 6] * 4   # empty / apart
        assert info[by[2]]["n_matches"] > 10 and info[by[8]]["n_matches"] > 10


# ------------------------------------------------------ degenerate epipoles
def test_degenerate_epipoles_null_u_right_and_level_counts(torch, oracle, matchers):
    g1, g2, fe = edge_problem("geometry")
    t1, t2, _ = edge_problem("ties")
    on_plane = dict(g1, pose=T.pose_rec(ow=(1.0, 0.5, 0.0)))     # C2z = 0: invz = inf
    on_axis = dict(g1, pose=T.pose_rec(ow=(0.0, 0.5, 0.0)))      # 0 * inf: ex is NaN
    same = dict(g1, pose=T.pose_rec(ow=(0.0, 0.0, 0.0)))         # C2 = 0: both NaN
    sides = [g1, g2, on_plane, on_axis, same, t1, t2]
    pairs = [(0, 1), (2, 1), (3, 1), (4, 1), (5, 6)]
    f12 = np.stack([fe] * 5)
    m12, info, refs = run(torch, oracle, matchers[False], sides, pairs, f12, tag="epipoles")
    # nothing is skipped by the gate: the mono-mono pair it rejects ("epi_in") comes back
    assert info["n_matches"][1] == info["n_matches"][0] + 1
    assert info["n_matches"][2:4].tolist() == [info["n_matches"][1]] * 2
    for ur in (True, False):
        for L in (1, 16):
            scale = np.cumprod(np.concatenate([[1.0], np.full(L - 1, 1.2)])).astype(f32)
            host = (E.CAM, scale, (scale * scale).astype(f32))
            a = run(torch, oracle, matchers[True], sides, pairs, f12, host=host, with_u_right=ur,
                    tag=("levels", L, ur))
            assert a[1]["n_matches"][0] > 20 and (a[1]["n_undefined"] == 0).all()
    # without mvuRight every keypoint is monocular: only_stereo finds nothing to try
    m12, info, _ = run(torch, oracle, matchers[True], sides, pairs, f12, only_stereo=True,
                       with_u_right=False, tag="only_stereo, no u_right")
    assert (info["n_tried"] == 0).all() and (info["n_matches"] == 0).all()


# ----------------------------------------------------------------- malformed
MALFORMED_EDITS = ("decrease", "above", "feat", "negative_first", "counts")


@pytest.mark.parametrize("which", MALFORMED_EDITS)
@pytest.mark.parametrize("side", [0, 1])
def test_malformed_slots_are_reported_not_read(torch, oracle, matchers, which, side):
    """In the middle of a batch, so that an unchecked read would stay inside the
    allocation.  Problem 2's KF1 (side 0) or KF2 (side 1) slot is damaged."""
    g1, g2, fe = edge_problem("geometry")
    sides, pairs, f12 = separate([(g1, g2, fe)] * 5)
    stride = max(len(s["desc"]) for s in sides) + 2

    def edit(a):
        k = 4 + side
        n, nn = int(a["nkeys"][k]), int(a["n_fv_nodes"][k])
        ob = k * (stride + 1)
        if which == "decrease":
            a["fv_offs"][ob + nn // 2] = a["fv_offs"][ob + nn // 2 - 1] - 1
        elif which == "above":
            a["fv_offs"][ob + nn] = n + 1
        elif which == "feat":
            a["fv_feats"][k * stride + n // 2] = n
        elif which == "negative_first":
            a["fv_offs"][ob] = -1
        else:   # counts above the stride: clamped, and the node list runs into the junk
            a["nkeys"][k] = stride + 9
            a["n_fv_nodes"][k] = stride + 9
    m12, info, refs = run(torch, oracle, matchers[True], sides, pairs, f12, stride=stride,
                          edit=edit, tag=(which, side))
    assert refs[2][1] == T.MALFORMED and tuple(info[2]) == T.MALFORMED
    n1 = stride if (which == "counts" and side == 0) else len(g1["desc"])
    assert (m12[2, :n1] == -1).all() and (m12[2, n1:] == JUNK).all()
    assert tuple(info[1]) == tuple(info[3]) == refs[0][1] and refs[0][1][0] >= 40
    assert np.array_equal(m12[1], m12[3]) and np.array_equal(m12[1], m12[0])


def test_clamped_counts_are_the_same_problem(torch, oracle, matchers):
    """n_fv_nodes of -3 is an empty FeatureVector; a node list that goes on to
    the keypoint count with empty nodes of new ids, clamped there, changes
    nothing."""
    (n1, n2, fn), host = natural(oracle, 3, 1, 0.5, 200)
    sides, pairs, f12 = separate([(n1, n2, fn)] * 3)
    stride = max(len(s["desc"]) for s in sides) + 1

    def edit(a):
        a["n_fv_nodes"][2] = -3
        k = 4
        n, nn, b, ob = int(a["nkeys"][k]), int(a["n_fv_nodes"][k]), k * stride, k * (stride + 1)
        assert nn < n
        a["fv_nodes"][b + nn:b + n] = 600000 + np.arange(n - nn)
        a["fv_offs"][ob + nn + 1:ob + n + 1] = a["fv_offs"][ob + nn]
        a["n_fv_nodes"][k] = stride + 9
    m12, info, refs = run(torch, oracle, matchers[True], sides, pairs, f12, stride=stride,
                          host=host, edit=edit, tag="clamped")
    assert tuple(info[1]) == (0,) * 6
    assert info[0]["n_matches"] > 10 and tuple(info[2]) == tuple(info[0])


def test_octave_outside_the_tables_is_counted_and_never_wins(torch, oracle, matchers):
    c = edge("geometry")
    g1, g2, fe = edge_problem("geometry")
    want = c["expect"]
    hit = np.nonzero(want >= 0)[0]
    keys2 = g2["keys"].copy()
    losers = [int(want[hit[3]]), int(want[hit[11]]), int(want[hit[20]])]
    keys2["octave"][losers] = [8, -1, 1 << 30]
    sides, pairs, f12 = [g1, dict(g2, keys=keys2), g2], [(0, 2), (0, 1), (0, 2)], np.stack([fe] * 3)
    m12, info, refs = run(torch, oracle, matchers[False], sides, pairs, f12, tag="octave")
    assert info[1]["n_undefined"] >= 3 and info[0]["n_undefined"] == info[2]["n_undefined"] == 0
    assert not np.isin(m12[1, :len(want)], losers).any()
    assert np.array_equal(m12[0, :len(want)], want) and np.array_equal(m12[0], m12[2])
    # with one level every octave above 0 is outside
    keys2 = g2["keys"].copy()
    keys2["octave"][losers] = 1
    host = (E.CAM, E.SCALE[:1], E.SIGMA2[:1])
    m12, info, _ = run(torch, oracle, matchers[False], [g1, dict(g2, keys=keys2)], [(0, 1)],
                       fe[None], host=host, tag="octave, one level")
    assert info[0]["n_undefined"] >= 3 and not np.isin(m12[0, :len(want)], losers).any()


# -------------------------------------------------------------------- errors
def test_status_codes(gpu, torch, oracle, matchers):
    m = matchers[True]
    g1, g2, fe = edge_problem("geometry")
    d = run(torch, oracle, m, [g1, g2], [(0, 1), (0, 1)], np.stack([fe, fe]), launch=False)
    cap = gpu.search_for_triangulation_batch_max_stride()

    def refused(status, **over):
        with pytest.raises(gpu.OrbError) as err:
            d.launch(m, **over)
        assert err.value.status == status, over
        m12, info = d.results()
        assert (m12 == JUNK).all() and (info.view(np.int32) == JUNK).all(), over  # nothing ran

    refused(gpu.ORB_ECAPACITY, kp_stride=cap + 1)
    required = [k for k in d.args() if k.startswith("d_") and k != "d_kf_u_right"]
    assert len(required) == 14
    bad_levels = [dict(scale_factors=np.ones(n, f32), level_sigma2=np.ones(n, f32)) for n in (0, 17)]
    for v in (0.0, -1.0, float("nan"), float("inf")):
        s = E.SCALE.copy()
        s[3] = v
        bad_levels += [dict(scale_factors=s), dict(level_sigma2=s)]
    for over in [dict(n_problems=-1), dict(kp_stride=0), dict(kp_stride=-4)] + bad_levels + [
            {k: 0} for k in required]:
        refused(gpu.ORB_EINVAL, **over)
    d.launch(m, n_problems=0)                     # fine, and nothing is launched
    m12, info = d.results()
    assert (m12 == JUNK).all() and (info.view(np.int32) == JUNK).all()
    d.launch(m, n_problems=0, d_match12=0, d_info=0)
    d.launch(m)                                   # the handle still works
    m12, info = d.results()
    want = T.expected(oracle, g1, g2, fe, *EDGE_HOST, False, True)
    T.check(m12, info, 0, len(want[0]), *want, JUNK, "after the refusals")
    T.check(m12, info, 1, len(want[0]), *want, JUNK, "after the refusals")


def test_stride_of_the_new_points_capacity_is_accepted(gpu, torch, oracle, matchers):
    """kp_stride = 10,176, the largest create_new_map_points_batch takes: dynamic
    LDS above 64 KiB, one small problem."""
    stride = gpu.ORBmatcher.create_new_map_points_max_stride()
    assert stride == 10176 <= gpu.search_for_triangulation_batch_max_stride()
    t1, t2, fe = edge_problem("ties")
    m12, info, _ = run(torch, oracle, matchers[True], [t1, t2], [(0, 1)], fe[None], stride=stride,
                       tag="stride 10176")
    want = edge("ties")["expect"]
    assert np.array_equal(m12[0, :len(want)], want) and info[0]["n_matches"] == 12


# ------------------------------------------------------ one-problem equivalence
def test_equals_the_one_problem_entry(gpu, torch, oracle, matchers):
    for ori, only_stereo in ((True, False), (False, True)):
        m = matchers[ori]
        (n1, n2, fn), host = natural(oracle, 7, 2, 0.5)
        for probs, hv in (([edge_problem("geometry"), edge_problem("ties")], EDGE_HOST),
                          ([(n1, n2, fn)], host)):
            sides, pairs, f12 = separate(probs)
            m12, info, _ = run(torch, oracle, m, sides, pairs, f12, only_stereo, host=hv,
                               tag="vs one-problem")
            for p, (s1, s2, f) in enumerate(probs):
                fr = lambda s: gpu.Frame(s["keys"], s["desc"], hv[1], E.W, E.H, u_right=s["u_right"])
                n, row = m.SearchForTriangulation(
                    fr(s1), (s1["pidx"] >= 0).astype(np.uint8), fr(s2),
                    (s2["pidx"] >= 0).astype(np.uint8), hv[2], f, hv[0], s1["pose"]["ow"],
                    s2["pose"]["rcw"], s2["pose"]["tcw"], s1["fv"], s2["fv"], only_stereo)
                assert n == info[p]["n_matches"] and np.array_equal(row, m12[p, :len(row)]), p


# --------------------------------------------------------------- two streams
def test_two_streams_on_one_handle_no_synchronisation(gpu, torch, oracle, matchers):
    """One handle, two streams, calls of different sizes alternating with no
    host wait in between: the kernel keeps no state in the handle."""
    m = matchers[True]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    (n1, n2, fn), host = natural(oracle, 3, 1, 0.0)
    big = separate([(n1, n2, fn)] * 24)
    small = separate([edge_problem("geometry"), edge_problem("ties"), edge_problem("four_tied")])
    d1 = run(torch, oracle, m, *big, host=host, launch=False)
    d2 = run(torch, oracle, m, *small, launch=False)
    d3 = run(torch, oracle, m, *small, launch=False)
    torch.cuda.synchronize()
    d1.launch(m, stream=s1.cuda_stream)
    d2.launch(m, stream=s2.cuda_stream)
    d3.launch(m, True, stream=s1.cuda_stream)
    d2.launch(m, stream=s2.cuda_stream)
    d1.launch(m, stream=s1.cuda_stream)
    for d, (sides, pairs, f12), hv, st, tag in ((d1, big, host, False, "stream 1"),
                                                (d2, small, EDGE_HOST, False, "stream 2"),
                                                (d3, small, EDGE_HOST, True, "stream 1 small")):
        m12, info = d.results()
        arr = T.pack_slots(sides, d.stride)
        compare(m12, info, arr, d.stride, pairs,
                reference(oracle, arr, d.stride, pairs, f12, hv, st, True), tag)


# --------------------------------------------------------------------- chain
def chain_scene(monocular):
    """One keyframe and three neighbours with descriptors: newpoints_cases'
    natural geometry (the same KF1 against three baselines), a random
    descriptor per KF1 keypoint and its matched KF2 keypoint six bits away.
    Twelve KF1 keypoints are moved onto another one (0.2 px apart, two bits
    apart): both take that one's KF2 keypoint and both triangulate."""
    baselines = ((0.9, 0.05, 0.1), (-0.7, 0.1, 0.2), (0.2, -0.6, 0.3))
    cs = [C.natural_case(f"tri_chain{k}", 31, 150, monocular, baseline=bl)
          for k, bl in enumerate(baselines)]
    rng = np.random.default_rng(77)
    kf1 = cs[0].kf1
    n1 = len(kf1["keys"])
    flip = lambda d, k: E.flip_bits(d, k, start=int(rng.integers(16, 240)))
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    free = np.nonzero((cs[0].match12 >= 0) & (kf1["point_index"] < 0))[0]
    keys1 = kf1["keys"].copy()
    ur1 = None if kf1["u_right"] is None else kf1["u_right"].copy()
    dp1 = None if kf1["depth"] is None else kf1["depth"].copy()
    moved = free[1:48:4]
    for a, b in zip(free[0:48:4], moved):
        keys1[b] = keys1[a]
        keys1[b]["x"] += f32(0.2)
        if ur1 is not None:
            ur1[b], dp1[b] = ur1[a], dp1[a]
        d1[b] = flip(d1[a], 2)
    kf1 = dict(kf1, keys=keys1, u_right=ur1, depth=dp1)
    kf2s, d2s, f12 = [], [], []
    for k, c in enumerate(cs):
        n2 = len(c.kf2["keys"])
        d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
        # neighbour k can match the KF1 keypoints with i1 % 3 <= k: a third is new to
        # each neighbour, the rest already have their points unless they were rejected
        for i in np.setdiff1d(np.nonzero(c.match12 >= 0)[0], moved):
            if i % 3 <= k:
                d2[c.match12[i]] = flip(d1[i], 6)
        kf2s.append(c.kf2)
        d2s.append(d2)
        pose = lambda kf: dict(Rw=kf["pose"]["rcw"].reshape(3, 3), tw=kf["pose"]["tcw"])
        f12.append(S.fundamental(pose(kf1), pose(c.kf2)).reshape(9))
    return cs, kf1, d1, kf2s, d2s, np.stack(f12)


def chain_side(oracle, kf, desc):
    n = len(kf["keys"])
    ur = np.full(n, -1.0, f32) if kf["u_right"] is None else kf["u_right"]
    s = B.side(desc, kf["keys"]["angle"], oracle.feature_vector(S.vocab_nodes(desc)),
               kf["point_index"])
    s.update(keys=kf["keys"], u_right=ur, pose=kf["pose"])
    return s


@pytest.mark.parametrize("monocular", [False, True])
def test_chain_matcher_to_new_points_device_resident(gpu, torch, oracle, matchers, monocular):
    """LocalMapping::CreateNewMapPoints for one keyframe and three neighbours:
    slot tensors uploaded once, F12 per pair uploaded ahead, then per neighbour
    matcher -> (median) -> new points on one stream with no host copy between
    them; afterwards everything against the host loop oracle matcher ->
    newpoints_ref, each neighbour seeing the previous one's AddMapPoints."""
    m = matchers[True]
    cs, kf1, d1, kf2s, d2s, f12 = chain_scene(monocular)
    n1, SS = len(kf1["keys"]), 384
    n_exist, cap = cs[0].cursor, cs[0].cursor + 3 * n1
    cam, sf, sig = C.CAM_N, C.SCALE_FACTORS, C.LEVEL_SIGMA2
    # ---- the host loop
    points = C.junk_points(cap)
    points[:n_exist] = cs[0].points
    r_kf1 = dict(kf1, point_index=kf1["point_index"].copy())
    r_kf2 = [dict(k, point_index=k["point_index"].copy()) for k in kf2s]
    r_status = np.full((3, n1), 0xEE, np.uint8)
    r_x3d = np.full((3, n1, 3), -7.25, f32)
    r_pairs = np.full((3, n1, 2), -77, np.int32)
    cursor, r_info, r_tri, r_m12, r_med, shared_accepted = n_exist, [], [], [], [], 0
    for k in range(3):
        row, tinfo = T.expected(oracle, chain_side(oracle, r_kf1, d1),
                                chain_side(oracle, r_kf2[k], d2s[k]), f12[k], cam, sf, sig, False,
                                True)
        med = R.scene_median_depth(r_kf2[k]["point_index"], r_kf2[k]["pose"], points["pos"], 2)[0]
        info, cursor = R.create_new_map_points(r_kf1, r_kf2[k], row, med, cam, cam, sf, sig,
                                               monocular, points, cursor, r_status[k], r_x3d[k],
                                               r_pairs[k])
        acc = row[r_status[k] == R.ACCEPTED]
        shared_accepted += T.shared_count(acc)
        if T.shared_count(acc):   # KF2's row holds the id of the largest such i1
            j = np.bincount(acc).argmax()
            i_last = np.nonzero((row == j) & (r_status[k] == R.ACCEPTED))[0].max()
            assert r_kf2[k]["point_index"][j] == r_kf1["point_index"][i_last]
        r_tri.append(tinfo), r_m12.append(row), r_info.append(info), r_med.append(med)
    # the reference alone shows what item 3 is about, and the later neighbours find work
    assert shared_accepted >= 8 and sum(t[4] for t in r_tri) >= shared_accepted
    assert all(int(i["n_new"]) > 3 for i in r_info) and all(t[0] > 3 for t in r_tri)
    assert r_tri[1][3] < r_tri[0][3]        # fewer KF1 keypoints are tried once points exist
    # ---- the device: slot 0 = the current keyframe, slots 1..3 = the neighbours
    sides = [chain_side(oracle, kf1, d1)] + [chain_side(oracle, k, d) for k, d in zip(kf2s, d2s)]
    arr = T.pack_slots(sides, SS, with_u_right=not monocular)
    arr["pidx"][:] = -9
    depth = np.full(4 * SS, np.nan, f32)
    for s, kf in enumerate([kf1] + kf2s):
        n = len(kf["keys"])
        arr["pidx"][s * SS:s * SS + n] = kf["point_index"]
        if not monocular:
            depth[s * SS:s * SS + n] = kf["depth"]
    pts = C.junk_points(cap)
    pts[:n_exist] = cs[0].points
    d = {k: _dev(torch, v) for k, v in arr.items() if v is not None}
    d.update({k: _dev(torch, v) for k, v in dict(
        depth=depth, points=pts, slots=np.arange(4, dtype=np.int32), f12=f12.astype(f32),
        cursor=np.array([n_exist], np.int32), cidx=np.zeros(1, np.int32)).items()})
    med = torch.full((4,), -1.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    m12 = torch.full((3 * SS,), JUNK, dtype=torch.int32, device="cuda")
    tinfo = torch.full((3 * 6,), JUNK, dtype=torch.int32, device="cuda")
    status = torch.full((3 * SS,), 0xEE, dtype=torch.uint8, device="cuda")
    x3d = torch.full((3 * SS * 3,), -7.25, dtype=torch.float32, device="cuda")
    pairs = torch.full((3 * SS * 2,), -77, dtype=torch.int32, device="cuda")
    info = torch.zeros(3 * 64, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    sp, P = stream.cuda_stream, lambda name: d[name].data_ptr()
    ur, dp = (0, 0) if monocular else (P("u_right"), P("depth"))
    for k in range(3):
        m.search_for_triangulation_batch(
            1, P("slots"), P("slots") + 4 * (k + 1), P("keys"), P("desc"), P("nkeys"), P("pidx"),
            P("fv_nodes"), P("fv_offs"), P("fv_feats"), P("n_fv_nodes"), ur, P("pose"), SS,
            P("f12") + 36 * k, cam, sf, sig, False, m12.data_ptr() + 4 * SS * k,
            tinfo.data_ptr() + 24 * k, sp)
        m.scene_median_depth_batch(1, P("slots") + 4 * (k + 1), P("nkeys"), P("pidx"), P("pose"), SS,
                                   P("points"), med.data_ptr() + 4 * (k + 1),
                                   cnt.data_ptr() + 4 * (k + 1), 2, sp)
        m.create_new_map_points_batch(
            1, P("slots"), P("slots") + 4 * (k + 1), P("keys"), P("nkeys"), P("pidx"), P("pose"),
            ur, dp, SS, m12.data_ptr() + 4 * SS * k, med.data_ptr() + 4 * (k + 1), cam, cam, sf, sig,
            monocular, P("points"), cap, P("cursor"), P("cidx"), status.data_ptr() + SS * k,
            x3d.data_ptr() + 12 * SS * k, pairs.data_ptr() + 8 * SS * k, info.data_ptr() + 64 * k, sp)
    stream.synchronize()    # the one host wait
    g_m12 = m12.cpu().numpy().reshape(3, SS)
    g_tinfo = tinfo.cpu().numpy().view(T.INFO_DTYPE)
    for k in range(3):
        T.check(g_m12, g_tinfo, k, n1, r_m12[k], r_tri[k], JUNK, ("chain matcher", k))
    same_f(med.cpu().numpy()[1:], np.array(r_med, f32), "chain medians")
    st = status.cpu().numpy().reshape(3, SS)
    assert (st[:, :n1] == r_status).all() and (st[:, n1:] == 0xEE).all()
    same_f(x3d.cpu().numpy().reshape(3, SS, 3)[:, :n1], r_x3d, "chain x3d")
    assert (pairs.cpu().numpy().reshape(3, SS, 2)[:, :n1] == r_pairs).all()
    same_rec(d["points"].cpu().numpy().view(R.MAP_POINT_DTYPE), points, "chain points")
    got = d["pidx"].cpu().numpy().view(np.int32).reshape(4, SS)
    assert (got[0, :n1] == r_kf1["point_index"]).all() and (got[0, n1:] == -9).all()
    for k in range(3):
        n2 = len(r_kf2[k]["point_index"])
        assert (got[k + 1, :n2] == r_kf2[k]["point_index"]).all(), k
        assert (got[k + 1, n2:] == -9).all()
    same_rec(info.cpu().numpy().view(R.NEW_POINT_INFO_DTYPE), np.array(r_info), "chain info")
    assert int(d["cursor"].cpu().numpy().view(np.int32)[0]) == cursor


# ------------------------------------------- new points: one idx2, several i1
def shared_idx2_case():
    """A hand-made match12: KF1 keypoints 0, 1, 2 (copies of keypoint 0, the
    middle one 60 px off) all name keypoint 0's KF2 match.  The first and the
    third are accepted, the middle one fails a reprojection check."""
    c = C.natural_case("shared_idx2", 41, 40, True, accept=[True] * 40)
    keys1 = c.kf1["keys"].copy()
    keys1[1], keys1[2] = keys1[0], keys1[0]
    keys1[1]["y"] += f32(60.0)
    keys1[2]["x"] += f32(0.25)
    m12 = c.match12.copy()
    m12[1] = m12[2] = m12[0]
    return C.Case("shared_idx2", dict(c.kf1, keys=keys1), c.kf2, m12, True, c.median, C.CAM_N,
                  C.CAM_N, cursor=c.cursor, capacity=c.capacity, points=c.points)


def test_new_points_kf2_row_holds_the_largest_i1(torch, matchers):
    c = shared_idx2_case()
    ref = c.ref()
    assert ref["status"][[0, 2]].tolist() == [R.ACCEPTED] * 2
    assert ref["status"][1] in (R.REPROJ1, R.REPROJ2)
    j = int(c.match12[0])
    assert ref["pidx2"][j] == ref["pidx1"][2] == ref["pidx1"][0] + 1   # the third's id
    for _ in range(3):      # a plain store would leave either id, run to run
        run_group(torch, matchers[False], [c] * 6, stride=384)
