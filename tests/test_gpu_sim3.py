"""Sim3Solver as a device batch (orb_sim3_solver_setup_batch / _iterate_batch,
k_sim3_setup / k_sim3_iterate) against tests/sim3_ref.py: every byte of the
state, the correspondences, the result and the inlier flags, slots past each
count untouched.  Float fields are compared by bit pattern, except that any NaN
equals any NaN (the degenerate samples produce them; which NaN an operation
returns is the one thing IEEE leaves to the machine)."""
import math

import numpy as np
import pytest

import scenarios as S
import sim3_cases as C
from sim3_ref import CORR_DTYPE, RESULT_DTYPE, STATE_DTYPE

pytestmark = pytest.mark.gpu
JUNK = 0x5A
LS = np.float32(math.log(np.float32(1.2)))


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def matcher(gpu):
    return gpu.ORBmatcher(0.75, True)


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def same(a, b, what=""):
    """Structured records equal byte for byte, any NaN equal to any NaN."""
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.shape, b.shape)
    for name in a.dtype.names:
        x, y = a[name], b[name]
        if x.dtype.kind == "f":
            ok = (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))
        else:
            ok = x == y
        assert ok.all(), (what, name, x[~ok][:4], y[~ok][:4], np.argwhere(~ok)[:4])


class Dev:
    """A sim3_cases.Batch on the device, outputs filled with JUNK bytes."""

    def __init__(self, torch, matcher, problems, stride=C.STRIDE, max_iterations=C.MAX_ITERATIONS,
                 rand_max=C.RAND_MAX, force_index1=False):
        assert all(p.rand_max == rand_max for p in problems)
        self.torch, self.m, self.rand_max = torch, matcher, rand_max
        self.b = b = C.Batch(problems, stride, max_iterations, force_index1)
        self.P, self.S = len(problems), stride
        self.d = {k: _dev(torch, getattr(b, k)) for k in
                  ("kf1_slot", "kf2_slot", "keys", "nkeys", "point_index", "pose", "points",
                   "match12", "index2", "draws")}
        self.d["index1"] = None if b.index1 is None else _dev(torch, b.index1)
        junk = lambda n: torch.full((max(n, 1),), JUNK, dtype=torch.uint8, device="cuda")
        self.state = junk(self.P * STATE_DTYPE.itemsize)
        self.corr = junk(self.P * stride * CORR_DTYPE.itemsize)
        self.inl = junk(self.P * stride)
        self.res = junk(self.P * RESULT_DTYPE.itemsize)
        self.ref = b.solvers()
        self.last = [None] * self.P  # the reference's last iterate() per problem

    def setup(self, stream=0, **kw):
        d = self.d
        a = dict(probability=C.PROBABILITY, min_inliers=C.MIN_INLIERS,
                 max_iterations=self.b.max_iterations, level_sigma2=C.LEVEL_SIGMA2, cam1=C.CAM1,
                 cam2=C.CAM2, fix_scale=self.b.problems[0].fix_scale if self.P else False)
        a.update(kw)
        self.m.sim3_solver_setup_batch(
            self.P, d["kf1_slot"].data_ptr(), d["kf2_slot"].data_ptr(), d["keys"].data_ptr(),
            d["nkeys"].data_ptr(), d["point_index"].data_ptr(), d["pose"].data_ptr(), self.S,
            d["points"].data_ptr(), d["match12"].data_ptr(),
            0 if d["index1"] is None else d["index1"].data_ptr(), d["index2"].data_ptr(),
            d_state=self.state.data_ptr(), d_corr=self.corr.data_ptr(), stream=stream, **a)

    def iterate(self, n, active=None, stream=0, ref=True):
        act = None if active is None else _dev(self.torch, np.asarray(active, np.uint8))
        self.m.sim3_solver_iterate_batch(
            self.P, self.S, self.state.data_ptr(), self.corr.data_ptr(), self.d["draws"].data_ptr(),
            self.b.draws.shape[1], n, self.inl.data_ptr(), self.res.data_ptr(),
            0 if act is None else act.data_ptr(), self.rand_max, self.b.max_iterations, stream)
        if ref:
            for i, s in enumerate(self.ref):
                if active is None or active[i]:
                    self.last[i] = s.iterate(n)
        self._keep = act

    # ---- readback and comparison
    def states(self):
        self.torch.cuda.synchronize()
        return self.state.cpu().numpy()[:self.P * STATE_DTYPE.itemsize].view(STATE_DTYPE)

    def results(self):
        self.torch.cuda.synchronize()
        return self.res.cpu().numpy()[:self.P * RESULT_DTYPE.itemsize].view(RESULT_DTYPE)

    def check(self, results=True, only=None):
        st = self.states()
        corr = self.corr.cpu().numpy().view(CORR_DTYPE).reshape(self.P, self.S)
        raw = self.corr.cpu().numpy().reshape(self.P, self.S, CORR_DTYPE.itemsize)
        inl = self.inl.cpu().numpy().reshape(self.P, self.S)
        res = self.results()
        for i, s in enumerate(self.ref):
            if only is not None and i not in only:
                continue
            name = self.b.problems[i].name
            same(st[i], s.state_record(), f"{name} state")
            same(corr[i, :s.N], s.corr_records(), f"{name} corr")
            assert (raw[i, s.N:] == JUNK).all(), f"{name}: corr past N written"
            if self.last[i] is None:
                if results:
                    assert (inl[i] == JUNK).all(), f"{name}: inliers written before any iterate"
                continue
            T, no_more, vb, n_in = self.last[i]
            if results:
                same(res[i], s.result_record(T, no_more, n_in), f"{name} result")
                assert np.array_equal(inl[i, :s.mN1], vb.astype(np.uint8)), f"{name} inliers12"
            assert (inl[i, s.mN1:] == JUNK).all(), f"{name}: inliers12 past mN1 written"


def homogeneous(problems):
    """Problems whose fix_scale differs cannot share a setup call."""
    return [[p for p in problems if bool(p.fix_scale) == f] for f in (False, True)]


def directed_default():
    return [p for p in C.directed().values() if p.rand_max == C.RAND_MAX]


# ------------------------------------------------------------ directed inputs
@pytest.mark.parametrize("fix", [False, True])
def test_directed_one_batch_rounds(torch, matcher, fix):
    """Every directed input in one batch: setup, then ComputeSim3's rounds of
    iterate(5) with the finished problems discarded, compared after every round."""
    probs = homogeneous(directed_default())[int(fix)]
    d = Dev(torch, matcher, probs)
    d.setup()
    d.check()
    active = np.ones(len(probs), np.uint8)
    rounds = 0
    while active.any():
        d.iterate(5, active)
        d.check()
        res = d.results()
        for i in np.nonzero(active)[0]:
            if res["no_more"][i] or res["has_sim3"][i]:
                active[i] = 0  # vbDiscarded
        rounds += 1
        assert rounds <= 61
    assert rounds > 2


@pytest.mark.parametrize("name", sorted(C.directed()))
def test_directed_alone_find(torch, matcher, name):
    p = C.directed()[name]
    d = Dev(torch, matcher, [p], rand_max=p.rand_max)
    d.setup()
    d.check()
    d.iterate(C.MAX_ITERATIONS)  # find()
    d.check()
    d.iterate(C.MAX_ITERATIONS)  # and what a caller that goes on would get
    d.check()


def test_counts_present():
    need = {f"N={n}" for n in (19, 20, 21, 63, 64, 65, 80, 81, 200)} | {"N=stride"}
    have = set().union(*(p.tags for p in C.directed().values()))
    assert need <= have
    assert C.directed()["full_stride"].solver().N == C.STRIDE


# ------------------------------------------------------- batch sizes and slots
@pytest.mark.parametrize("n", [1, 16, 300])
def test_batch_sizes_with_holes(torch, matcher, n):
    for probs in homogeneous(C.mixed(n)):
        if not probs:
            continue
        d = Dev(torch, matcher, probs)
        d.setup()
        d.check()
        rng = np.random.default_rng(n)
        active = (rng.random(len(probs)) < 0.7).astype(np.uint8)
        if len(probs) == 1:
            active[:] = 1
        d.iterate(2, active)
        d.check()
        d.iterate(C.MAX_ITERATIONS)
        d.check()


def test_shared_and_repeated_slots(torch, matcher):
    """Problems built on the same two keyframes and point array (one slot pair),
    the keyframes swapped between the two sides, and one problem twice."""
    base = C.make_problem("shared0", 700, n_corr=60, n_outliers=15, plan=("b", "g"))
    probs = [base]
    rng = np.random.default_rng(3)
    for k in range(1, 4):
        m12 = base.match12.copy()
        drop = rng.choice(np.nonzero(m12 >= 0)[0], 5 * k, replace=False)
        m12[drop] = -1
        draws = rng.integers(0, C.RAND_MAX + 1, len(base.draws)).astype(np.uint32)
        probs.append(C.Problem(f"shared{k}", base.kf1, base.kf2, base.points, m12, None,
                               base.index2, False, draws))
    probs.append(base)
    other = C.make_problem("other", 701, n_corr=30, n_outliers=5, plan=("g",))
    probs.append(other)
    d = Dev(torch, matcher, probs)
    assert len(set(d.b.kf1_slot[:5])) == 1 and d.b.kf1_slot[5] != d.b.kf1_slot[0]
    d.setup()
    d.check()
    d.iterate(C.MAX_ITERATIONS)
    d.check()
    st = d.states()
    assert st[0].tobytes() == st[4].tobytes()


# --------------------------------------------------------------------- rounds
NEVER = ("exhaust", "borderline", "fix_scale_wrong", "zero_rotation", "n20", "n19")


def test_rounds_to_exhaustion_equal_find(torch, matcher):
    """iterate(5) until bNoMore leaves the state one find() leaves."""
    D = C.directed()
    for probs in homogeneous([D[n] for n in NEVER]):
        a, b = Dev(torch, matcher, probs), Dev(torch, matcher, probs)
        a.setup()
        b.setup()
        b.iterate(C.MAX_ITERATIONS)
        active = np.ones(len(probs), np.uint8)
        for _ in range(61):
            a.iterate(5, active)
            active &= (a.results()["no_more"] == 0).astype(np.uint8)
            if not active.any():
                break
        assert not active.any()
        a.check(results=False)
        b.check()
        assert a.state.cpu().numpy().tobytes() == b.state.cpu().numpy().tobytes()
        assert a.corr.cpu().numpy().tobytes() == b.corr.cpu().numpy().tobytes()


@pytest.mark.parametrize("name", ["first_of_chunk", "last_of_chunk", "last_of_window",
                                  "at_max_its", "tie", "exhaust", "n81"])
def test_rounds_equal_one_call_of_the_same_total(torch, matcher, name):
    p = C.directed()[name]
    a = Dev(torch, matcher, [p])
    a.setup()
    total = 0
    for _ in range(61):
        a.iterate(5)
        r = a.results()[0]
        total += int(r["iterations_run"])
        if r["no_more"] or r["has_sim3"]:
            break
    a.check()
    b = Dev(torch, matcher, [p])
    b.setup()
    b.iterate(total)
    b.check()
    assert a.state.cpu().numpy().tobytes() == b.state.cpu().numpy().tobytes()
    assert a.corr.cpu().numpy().tobytes() == b.corr.cpu().numpy().tobytes()
    assert a.inl.cpu().numpy().tobytes() == b.inl.cpu().numpy().tobytes()
    ra, rb = a.results()[0].copy(), b.results()[0].copy()
    ra["iterations_run"] = rb["iterations_run"] = 0
    same(ra, rb, "result")


# ------------------------------------------------------ where the success falls
@pytest.mark.parametrize("name,at", [("first_of_chunk", C.CHUNK + 1), ("last_of_chunk", C.CHUNK),
                                     ("last_of_window", 5)])
@pytest.mark.parametrize("window", [5, C.MAX_ITERATIONS])
def test_success_position(torch, matcher, name, at, window):
    p = C.directed()[name]
    d = Dev(torch, matcher, [p])
    d.setup()
    for _ in range(61):
        d.iterate(window)
        d.check()
        if d.results()[0]["has_sim3"]:
            break
    st = d.states()[0]
    assert st["iterations"] == at and st["best_iteration"] == at
    assert d.results()[0]["no_more"] == 0


def test_success_exactly_at_max_its_then_no_more(torch, matcher):
    p = C.directed()["at_max_its"]
    d = Dev(torch, matcher, [p])
    d.setup()
    d.iterate(C.MAX_ITERATIONS)
    d.check()
    st, r = d.states()[0], d.results()[0]
    assert r["has_sim3"] == 1 and r["no_more"] == 0 and st["iterations"] == st["max_its"]
    d.iterate(5)
    d.check()
    r = d.results()[0]
    assert r["has_sim3"] == 0 and r["no_more"] == 1 and r["iterations_run"] == 0
    torch.cuda.synchronize()
    assert not d.inl.cpu().numpy()[:d.ref[0].mN1].any()


def test_tie_takes_the_later(torch, matcher):
    p = C.directed()["tie"]
    d = Dev(torch, matcher, [p])
    d.setup()
    d.iterate(1)
    first = int(d.states()[0]["best_inliers"])
    assert 0 < first <= C.MIN_INLIERS
    d.iterate(1)
    d.check()
    st = d.states()[0]
    assert st["best_inliers"] == first and st["best_iteration"] == 2


@pytest.mark.parametrize("window", [0, 1, 3, C.CHUNK - 1, C.CHUNK, C.CHUNK + 1, 20])
def test_window_and_chunk_shapes(torch, matcher, window):
    """Windows shorter than, equal to and longer than a chunk, on a problem that
    never succeeds and on one whose success falls inside the second chunk."""
    D = C.directed()
    d = Dev(torch, matcher, [D["exhaust"], D["first_of_chunk"]])
    d.setup()
    for _ in range(3):
        d.iterate(window)
        d.check()


# ------------------------------------------------------------------- malformed
@pytest.mark.parametrize("kind", ["index1_big", "index2_big", "octave1_neg", "octave2_big"])
def test_malformed_slots(torch, matcher, kind):
    bad = C.malformed()[kind]
    good = C.make_problem("good", 800, plan=("g",), with_index1=True)
    d = Dev(torch, matcher, [good, bad, good])
    d.setup()
    d.check()
    st = d.states()
    assert st["status"].tolist() == [0, -1, 0] and st["n"][1] == 0
    for _ in range(2):
        d.iterate(5)
        d.check()
        r = d.results()[1]
        assert r["no_more"] == 1 and r["has_sim3"] == 0 and r["iterations_run"] == 0


def test_draw_above_rand_max(torch, matcher):
    bad = C.malformed()["draw_big"]
    good = C.make_problem("good", 801, plan=("b", "b", "g"), with_index1=True, rand_max=32767)
    d = Dev(torch, matcher, [bad, good], rand_max=32767)
    d.setup()
    d.iterate(5)
    d.check()
    st, r = d.states(), d.results()
    assert st["status"].tolist() == [-1, 0] and st["iterations"][0] == 1
    assert r["no_more"][0] == 1 and r["iterations_run"][0] == 1 and r["has_sim3"][1] == 1
    d.iterate(5)
    d.check()
    assert d.results()["iterations_run"][0] == 0


# -------------------------------------------------- status codes and capacity
def test_status_codes_and_capacity(torch, gpu, matcher):
    p = C.make_problem("p", 900, plan=("g",))
    d = Dev(torch, matcher, [p])
    before = [t.clone() for t in (d.state, d.corr, d.inl, d.res)]

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(a, b) for a, b in zip(before, (d.state, d.corr, d.inl, d.res)))

    def status(fn, *a, **k):
        with pytest.raises(gpu.OrbError) as e:
            fn(*a, **k)
        return e.value.status

    big = gpu.sim3_solver_max_stride() + 1
    S0 = d.S
    d.S = big
    assert status(d.setup) == gpu.ORB_ECAPACITY
    assert status(d.iterate, 5, ref=False) == gpu.ORB_ECAPACITY
    d.S = S0
    assert untouched()
    for kw in (dict(min_inliers=2), dict(max_iterations=0), dict(probability=1.0),
               dict(probability=0.0), dict(level_sigma2=np.zeros(0, np.float32)),
               dict(level_sigma2=np.ones(17, np.float32)),
               dict(level_sigma2=np.array([1, np.nan], np.float32)),
               dict(level_sigma2=np.array([1, -1], np.float32))):
        assert status(d.setup, **kw) == gpu.ORB_EINVAL, kw
    d.S = 0
    assert status(d.setup) == gpu.ORB_EINVAL
    d.S = S0
    m = matcher
    ok = (1, d.S, d.state.data_ptr(), d.corr.data_ptr(), d.d["draws"].data_ptr(), 900, 5,
          d.inl.data_ptr(), d.res.data_ptr())
    assert status(m.sim3_solver_iterate_batch, *ok[:5], 899, *ok[6:]) == gpu.ORB_EINVAL  # draw_stride
    assert status(m.sim3_solver_iterate_batch, *ok[:6], -1, *ok[7:]) == gpu.ORB_EINVAL
    assert status(m.sim3_solver_iterate_batch, *ok[:2], 0, *ok[3:]) == gpu.ORB_EINVAL
    assert status(m.sim3_solver_iterate_batch, *ok[:8], 0) == gpu.ORB_EINVAL
    assert status(m.sim3_solver_iterate_batch, -1, *ok[1:]) == gpu.ORB_EINVAL
    assert untouched()
    m.sim3_solver_iterate_batch(0, *ok[1:])  # no problems: ORB_OK, no launch
    assert untouched()


# ----------------------------------------------------------------- two streams
def test_two_streams(torch, matcher):
    """Two batches on two streams, each ordered by its stream alone."""
    pa = C.mixed(12, seed=21)
    pb = C.mixed(12, seed=22)
    fa, fb = homogeneous(pa)[0], homogeneous(pb)[1]
    a, b = Dev(torch, matcher, fa), Dev(torch, matcher, fb)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a.setup(stream=sa.cuda_stream)
    b.setup(stream=sb.cuda_stream)
    for _ in range(3):
        a.iterate(5, stream=sa.cuda_stream)
        b.iterate(5, stream=sb.cuda_stream)
    sa.synchronize()
    sb.synchronize()
    a.check()
    b.check()


# ------------------------------------------------------------------- the chain
def test_chain_bow_solver_search_by_sim3(torch, gpu, oracle, matcher):
    """orb_match_bow_kf -> setup -> iterate -> orb_search_by_sim3 with the
    returned s, R, t: a loop candidate whose map drifted by a scale of 1.1."""
    rng = np.random.default_rng(5)
    R2, t2, _ = S.pose(rng)
    kf2 = S.keyframe(oracle, 3, 0, R2, t2, rng, nf=500)
    n = len(kf2["keys"])
    # the current keyframe sees the same image; its map is the candidate's, scaled
    R1, t1, ow1 = S.pose(rng)
    kf1 = dict(kf2)
    bits = np.unpackbits(kf2["desc"], axis=1) ^ (rng.random((n, 256)) < 0.03)
    kf1["desc"] = np.packbits(bits.astype(np.uint8), axis=1)
    X2 = (kf2["mps"]["pos"].astype(np.float64) @ R2.astype(np.float64).T) + t2
    mps1 = kf2["mps"].copy()
    mps1["pos"] = ((1.1 * X2 - t1.astype(np.float64)) @ R1.astype(np.float64)).astype(np.float32)
    mps1["max_distance"] *= np.float32(1.1)
    mps1["min_distance"] *= np.float32(1.1)
    kf1.update(mps=mps1, Rw=R1, tw=t1, ow=ow1)
    # SearchByBoW(pKF1, pKF2): map point ids are the keypoint index (+ n for KF2)
    fv1 = oracle.feature_vector(S.vocab_nodes(kf1["desc"]))
    fv2 = oracle.feature_vector(S.vocab_nodes(kf2["desc"]))
    mp1 = np.where(kf1["valid"] > 0, np.arange(n), -1).astype(np.int32)
    mp2 = np.where(kf2["valid"] > 0, np.arange(n) + n, -1).astype(np.int32)
    nm, m12 = matcher.SearchByBoWKF(kf1["desc"], kf1["keys"]["angle"], mp1, kf1["mps"]["bad"],
                                    fv1, kf2["desc"], kf2["keys"]["angle"], mp2,
                                    kf2["mps"]["bad"], fv2)
    assert nm > 40
    # the solver, through the one-problem class and against the restatement
    points = np.concatenate([kf1["mps"], kf2["mps"]])
    index2 = np.where(m12 >= 0, m12 - n, -1).astype(np.int32)
    draws = rng.integers(0, C.RAND_MAX + 1, 900).astype(np.uint32)
    cam = S.camera()
    sigma2 = np.asarray(kf1["sigma2"], np.float32)
    pose1, pose2 = S.pose_record(oracle, R1, t1)[0], S.pose_record(oracle, R2, t2)[0]
    solver = gpu.Sim3Solver(matcher, kf1["keys"], mp1, pose1, kf2["keys"], pose2, points, m12,
                            index2, sigma2, cam, cam, False, draws)
    from sim3_ref import KeyFrame, Sim3Solver
    ref = Sim3Solver(KeyFrame(kf1["keys"]["octave"], mp1, R1.reshape(9), t1),
                     KeyFrame(kf2["keys"]["octave"], mp2, R2.reshape(9), t2), m12, False,
                     points_pos=points["pos"], points_bad=points["bad"], index2=index2,
                     level_sigma2=sigma2, K1=cam[:4], K2=cam[:4], draws=draws)
    same(solver.state(), ref.state_record(), "chain setup")
    T, no_more, inl, n_in = solver.iterate(5)
    Tr, nmr, inlr, n_inr = ref.iterate(5)
    while T is None and not no_more:
        T, no_more, inl, n_in = solver.iterate(5)
        Tr, nmr, inlr, n_inr = ref.iterate(5)
    same(solver.state(), ref.state_record(), "chain state")
    assert T is not None and Tr is not None and n_in == n_inr and np.array_equal(inl, inlr)
    assert T.tobytes() == Tr.tobytes()
    s12, R12, t12 = solver.GetEstimatedScale(), solver.GetEstimatedRotation(), solver.GetEstimatedTranslation()
    assert abs(s12 - 1.1) < 1e-2
    # SearchBySim3 with the estimate finds more than BoW did
    k1, k2 = dict(kf1), dict(kf2)
    k1["already"] = (m12 >= 0).astype(np.uint8)
    k2["already"] = np.zeros(n, np.uint8)
    k2["already"][index2[index2 >= 0]] = 1
    rn, rm = oracle.search_by_sim3(k1, k2, cam, s12, R12, t12, 7.5, LS)
    fr = lambda k: gpu.Frame(k["keys"], k["desc"], k["scale"], k["width"], k["height"])
    nf, f12 = matcher.SearchBySim3(fr(k1), fr(k2), float(LS), cam, k1["Rw"], k1["tw"], k2["Rw"],
                                   k2["tw"], k1["mps"], k1["valid"], k1["already"], k1["mp_desc"],
                                   k2["mps"], k2["valid"], k2["already"], k2["mp_desc"], s12, R12,
                                   t12, 7.5)
    assert nf == rn and np.array_equal(f12, rm)
    assert nf > 10
