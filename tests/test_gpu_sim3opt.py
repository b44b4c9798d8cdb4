"""Optimizer::OptimizeSim3 as a device batch (orb_optimize_sim3_batch,
k_optimize_sim3) against tests/sim3opt_ref.py, bit for bit: q, t, s, the float
fields, the counts and the updated d_match12; rows of skipped, malformed and
inactive problems untouched.  Floating fields are compared by bit pattern,
except that any NaN equals any NaN (which NaN an operation returns is the one
thing IEEE leaves to the machine)."""
import numpy as np
import pytest

import sim3opt_cases as C
import sim3opt_ref as R

pytestmark = pytest.mark.gpu
JUNK = 0x5A
OUT = R.OPT_RESULT_DTYPE

_cases, _refs = None, {}


def cases():
    global _cases
    if _cases is None:
        _cases = C.all_cases()
    return _cases


def ref_of(name):
    """The reference's answer for a case, computed once and left unchanged."""
    if name not in _refs:
        _refs[name] = C.run_ref(cases()[name])
    return _refs[name]


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
    """Structured records equal bit for bit, any NaN equal to any NaN."""
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.shape, b.shape)
    for name in a.dtype.names:
        x, y = a[name], b[name]
        if x.dtype.kind == "f":
            u = np.uint64 if x.dtype.itemsize == 8 else np.uint32
            ok = (x.view(u) == y.view(u)) | (np.isnan(x) & np.isnan(y))
        else:
            ok = x == y
        assert ok.all(), (what, name, x[~ok][:4], y[~ok][:4], np.argwhere(~ok)[:4])


def min_stride(case):
    return max(case["n1"], case["n2"], 1)


class Pack:
    """A list of case names as the device arrays of one call.  A case that
    appears more than once shares its two keyframe slots and its points among
    its problems; every problem has its own match12 / index2 rows.  Whatever
    lies past a count is junk.  has_sim3 / active: per-problem flags."""

    def __init__(self, torch, gpu, names, stride=None, has_sim3=None, active=None, seed=0):
        self.torch, self.names = torch, list(names)
        cs = [cases()[n] for n in self.names]
        assert len({c["host"] for c in cs}) <= 1
        self.host = C.HOSTS[cs[0]["host"]] if cs else C.HOSTS["std"]
        self.S = S = max([min_stride(c) for c in cs] + [1]) if stride is None else stride
        self.P = P = len(cs)
        rng = np.random.default_rng(seed)
        uniq = list(dict.fromkeys(self.names))
        order = list(rng.permutation(2 * len(uniq)))  # slots in no particular order
        slot_of, base_of, npts = {}, {}, 3
        for k, n in enumerate(uniq):
            slot_of[n] = (int(order[2 * k]), int(order[2 * k + 1]))
            base_of[n] = npts
            npts += len(cases()[n]["pos"])
        ns = max(2 * len(uniq), 1)
        keys = np.zeros((ns, S), gpu.KEYPOINT_DTYPE)
        keys["octave"] = rng.integers(-50, 50, (ns, S))  # junk past every count
        keys["x"], keys["y"] = rng.uniform(0, 700, (ns, S)), rng.uniform(0, 700, (ns, S))
        pidx = rng.integers(-3, 2 ** 31 - 1, (ns, S)).astype(np.int32)
        nkeys = np.zeros(ns, np.int32)
        pose = np.zeros(ns, gpu.POSE_DTYPE)
        points = np.zeros(npts, gpu.MAP_POINT_DTYPE)
        points["pos"] = rng.uniform(-3, 3, (npts, 3))
        for n in uniq:
            c, (s1, s2), b = cases()[n], slot_of[n], base_of[n]
            a1, a2 = min(len(c["keys1"]), S), min(len(c["keys2"]), S)
            keys["x"][s1, :a1], keys["y"][s1, :a1] = c["keys1"][:a1, 0], c["keys1"][:a1, 1]
            keys["x"][s2, :a2], keys["y"][s2, :a2] = c["keys2"][:a2, 0], c["keys2"][:a2, 1]
            keys["octave"][s1, :a1], keys["octave"][s2, :a2] = c["octave1"][:a1], c["octave2"][:a2]
            pi = np.asarray(c["point_index1"], np.int64)[:a1]
            pidx[s1, :a1] = np.where((pi >= 0) & (np.arange(a1) < c["n1"]), pi + b, pi).astype(np.int32)
            # a count above the stride is clamped on the device
            nkeys[s1], nkeys[s2] = c["n1"], c["n2"]
            pose["rcw"][s1], pose["tcw"][s1] = c["pose1"]
            pose["rcw"][s2], pose["tcw"][s2] = c["pose2"]
            points["pos"][b:b + len(c["pos"])] = c["pos"]
            points["bad"][b:b + len(c["pos"])] = c["bad"]
        match = rng.integers(-3, 2 ** 31 - 1, (max(P, 1), S)).astype(np.int32)
        index2 = rng.integers(-3, 2 ** 31 - 1, (max(P, 1), S)).astype(np.int32)
        start = np.zeros(max(P, 1), gpu.SIM3_RESULT_DTYPE)
        start["has_sim3"] = 1 if has_sim3 is None else np.asarray(has_sim3)
        start["n_inliers"], start["T12"] = 77, 3.0  # fields the call does not read
        for i, (n, c) in enumerate(zip(self.names, cs)):
            a1 = min(len(c["match12"]), S)
            m = np.asarray(c["match12"], np.int64)[:a1]
            match[i, :a1] = np.where((m >= 0) & (np.arange(a1) < c["n1"]), m + base_of[n], m).astype(np.int32)
            index2[i, :a1] = c["index2"][:a1]
            start["R"][i], start["t"][i], start["scale"][i] = c["start"]
        self.match0, self.start = match, start
        self.kf1 = np.array([slot_of[n][0] for n in self.names] + [0], np.int32)
        self.kf2 = np.array([slot_of[n][1] for n in self.names] + [0], np.int32)
        self.active = None if active is None else np.asarray(active, np.uint8)
        self.d = {k: _dev(torch, v) for k, v in dict(
            kf1=self.kf1, kf2=self.kf2, keys=keys, nkeys=nkeys, pidx=pidx, pose=pose, points=points,
            match=match, index2=index2, start=start).items()}
        self.d_active = None if active is None else _dev(torch, self.active)
        self.out = torch.full((max(P, 1) * OUT.itemsize,), JUNK, dtype=torch.uint8, device="cuda")

    def args(self):
        d = self.d
        return [self.P, d["kf1"].data_ptr(), d["kf2"].data_ptr(), d["keys"].data_ptr(),
                d["nkeys"].data_ptr(), d["pidx"].data_ptr(), d["pose"].data_ptr(), self.S,
                d["points"].data_ptr(), d["match"].data_ptr(), d["index2"].data_ptr(),
                d["start"].data_ptr(), self.host["levels"], self.host["K1"], self.host["K2"],
                self.out.data_ptr()]

    def run(self, matcher, stream=0):
        matcher.optimize_sim3_batch(
            *self.args(), th2=float(self.host["th2"]), fix_scale=self.host["fix_scale"],
            d_active=0 if self.d_active is None else self.d_active.data_ptr(), stream=stream)

    def check(self):
        self.torch.cuda.synchronize()
        out = self.out.cpu().numpy()
        raw = out.reshape(-1, OUT.itemsize)
        rec = out.view(OUT)
        match = self.d["match"].cpu().numpy().view(np.int32).reshape(-1, self.S)
        for i, n in enumerate(self.names):
            c = cases()[n]
            live = bool(self.start["has_sim3"][i]) and (self.active is None or bool(self.active[i]))
            if not live:
                assert (raw[i] == JUNK).all(), f"{n}[{i}]: the row of a skipped problem written"
                assert np.array_equal(match[i], self.match0[i]), f"{n}[{i}]: match12 of a skipped problem"
                continue
            r = ref_of(n)
            same(rec[i], R.result_record(r)[0], f"{n}[{i}]")
            exp = self.match0[i].copy()
            n1 = min(c["n1"], self.S)
            gone = (np.asarray(r["match12"])[:n1] < 0) & (np.asarray(c["match12"])[:n1] >= 0)
            exp[:n1][gone] = -1
            assert np.array_equal(match[i], exp), (f"{n}[{i}] match12", np.argwhere(match[i] != exp)[:6].ravel())


STD = [n for n, c in C.all_cases().items() if c["host"] == "std"]
OTHER = sorted({c["host"] for c in C.all_cases().values()} - {"std"})


# ------------------------------------------------------------- one at a time
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("name", sorted(C.all_cases()))
def test_case_alone(torch, gpu, matcher, name, extra):
    """Every case alone, at the smallest stride that holds it and one more."""
    p = Pack(torch, gpu, [name], stride=min_stride(cases()[name]) + extra, seed=extra)
    p.run(matcher)
    p.check()


# ------------------------------------------------------------------- batches
@pytest.mark.parametrize("n", [1, 16, 300])
def test_batches_mixed_with_holes(torch, gpu, matcher, n):
    """Batches of mixed problems: repeated cases share slots, malformed ones
    stand in the middle, some problems are inactive or have no Sim3."""
    rng = np.random.default_rng(n)
    names = [STD[k] for k in rng.integers(0, len(STD), n)]
    if n >= 16:
        names[n // 2], names[n // 2 + 1], names[3] = "bad_i2", "bad_oct2", "bad_oct1_neg"
    has = np.ones(n, np.int32)
    act = np.ones(n, np.uint8)
    if n > 1:
        has[rng.integers(0, n, max(n // 8, 1))] = 0
        act[rng.integers(0, n, max(n // 8, 1))] = 0
    stride = max(min_stride(cases()[m]) for m in set(names)) + 3
    p = Pack(torch, gpu, names, stride=stride, has_sim3=has, active=act if n > 1 else None, seed=n)
    p.run(matcher)
    p.check()


@pytest.mark.parametrize("host", OTHER)
def test_other_host_values(torch, gpu, matcher, host):
    names = [n for n, c in cases().items() if c["host"] == host]
    p = Pack(torch, gpu, names + names[::-1], seed=5)
    p.run(matcher)
    p.check()


@pytest.mark.parametrize("stride", ["below_64k", "above_64k", "max"])
def test_lds_sizes(torch, gpu, matcher, stride):
    """The records stay in LDS at every stride (no scratch tier): the edge of the
    default 64 KiB dynamic allocation and the largest stride."""
    s = {"below_64k": 462, "above_64k": 463, "max": gpu.optimize_sim3_max_stride()}[stride]
    p = Pack(torch, gpu, ["nat200", "pairs129", "gate9_bad"], stride=s, seed=3)
    p.run(matcher)
    p.check()


# --------------------------------------------------------- one-problem entry
@pytest.mark.parametrize("name", ["nat75", "skips", "bad_oct2", "gate9_clean", "threshold", "fix50",
                                  "gate0_clean", "junk"])
def test_one_problem_entry(gpu, matcher, name):
    c, r = cases()[name], ref_of(name)
    H = C.HOSTS[c["host"]]
    n1, n2 = c["n1"], c["n2"]
    k1, k2 = np.zeros(n1, gpu.KEYPOINT_DTYPE), np.zeros(n2, gpu.KEYPOINT_DTYPE)
    k1["x"], k1["y"], k1["octave"] = c["keys1"][:n1, 0], c["keys1"][:n1, 1], c["octave1"][:n1]
    k2["x"], k2["y"], k2["octave"] = c["keys2"][:n2, 0], c["keys2"][:n2, 1], c["octave2"][:n2]
    pts = np.zeros(len(c["pos"]), gpu.MAP_POINT_DTYPE)
    pts["pos"], pts["bad"] = c["pos"], c["bad"]
    p1, p2 = np.zeros(1, gpu.POSE_DTYPE), np.zeros(1, gpu.POSE_DTYPE)
    p1["rcw"][0], p1["tcw"][0] = c["pose1"]
    p2["rcw"][0], p2["tcw"][0] = c["pose2"]
    n_in, m12, rec = matcher.OptimizeSim3(
        k1, c["point_index1"][:n1], p1[0], k2, p2[0], pts, c["match12"][:n1], c["index2"][:n1],
        *c["start"], H["levels"], H["K1"], H["K2"], float(H["th2"]), H["fix_scale"])
    same(np.frombuffer(rec.tobytes(), OUT), R.result_record(r), name)
    assert n_in == r["n_inliers"]
    assert np.array_equal(m12, np.asarray(r["match12"])[:n1])


# --------------------------------------------------------------- two streams
def test_two_streams(torch, gpu, matcher):
    a = Pack(torch, gpu, ["nat150", "pairs65", "skips", "bad_i2", "nat30"] * 3, seed=1)
    b = Pack(torch, gpu, ["fix50", "nat120_fix", "clean60_fix"] * 4, seed=2)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a.run(matcher, sa.cuda_stream)
    b.run(matcher, sb.cuda_stream)
    sa.synchronize()
    sb.synchronize()
    a.check()
    b.check()


# ------------------------------------------------- status codes and capacity
def test_status_codes_and_capacity(torch, gpu, matcher):
    p = Pack(torch, gpu, ["nat30", "gate10_bad"], seed=4)
    before = p.d["match"].cpu().numpy().copy()

    def untouched():
        torch.cuda.synchronize()
        return (p.out.cpu().numpy() == JUNK).all() and np.array_equal(p.d["match"].cpu().numpy(), before)

    def call(a, **kw):
        k = dict(th2=10.0, fix_scale=False)
        k.update(kw)
        matcher.optimize_sim3_batch(*a, **k)

    ok = p.args()
    for i in (3, 4, 5, 6, 8, 9, 10, 11, 15):  # every required device pointer
        a = list(ok)
        a[i] = 0
        with pytest.raises(gpu.OrbError) as e:
            call(a)
        assert e.value.status == gpu.ORB_EINVAL, i
    for i, v in ((0, -1), (7, 0), (7, -4), (12, np.zeros(0, np.float32)), (12, np.ones(17, np.float32))):
        a = list(ok)
        a[i] = v
        with pytest.raises(gpu.OrbError) as e:
            call(a)
        assert e.value.status == gpu.ORB_EINVAL, (i, v)
    a = list(ok)
    a[7] = gpu.optimize_sim3_max_stride() + 1
    with pytest.raises(gpu.OrbError) as e:
        call(a)
    assert e.value.status == gpu.ORB_ECAPACITY
    a[0] = 0  # the capacity is judged before the empty batch
    with pytest.raises(gpu.OrbError) as e:
        call(a)
    assert e.value.status == gpu.ORB_ECAPACITY
    assert untouched()
    call([0] + [0] * 6 + [ok[7]] + [0] * 4 + ok[12:15] + [0])  # no problems: ORB_OK, no launch
    assert untouched()
    assert gpu.optimize_sim3_max_stride() == matcher.optimize_sim3_max_stride() == \
        (160 * 1024 - 2 * 18720 - 2208) // 56


# ----------------------------------------------------------------- pinned_exp
def test_pinned_exp_device(torch, matcher):
    """pinned_exp on the device against the Python pin: the arguments the cases
    reach, and overflow, underflow, +-0, NaN and +-inf."""
    reached = set()
    for n in cases():
        reached |= ref_of(n)["trace"]["exp_args"]
    xs = [R._from_bits(b) for b in sorted(reached)]
    xs += [0.0, -0.0, np.nan, np.inf, -np.inf, 709.782712893384, 709.7827128933841, 710.0, 1e308,
           -745.1332191019411, -745.1332191019412, -745.2, -1e308, -708.4, -740.0, -744.9, 1e-9,
           -1e-9, 2.0 ** -28, 2.0 ** -28 * (1 - 2.0 ** -53), 0.34657359027997264, 0.3465735902799727,
           1.0397207708399179, 1.039720770839918, -0.35, -1.04, 1.0, -1.0, 5e-324, 88.7, -88.7]
    rng = np.random.default_rng(8)
    xs += list(rng.uniform(-750, 715, 2000)) + list(rng.uniform(-2, 2, 2000)) + \
        list(rng.standard_normal(500) * 1e-5)
    x = np.array(xs, np.float64)
    dx = _dev(torch, x)
    dy = torch.zeros(len(x) * 8, dtype=torch.uint8, device="cuda")
    matcher.pinned_exp_batch(len(x), dx.data_ptr(), dy.data_ptr())
    torch.cuda.synchronize()
    y = dy.cpu().numpy().view(np.float64)
    exp = np.array([R.pinned_exp(float(v)) for v in x], np.float64)
    ok = (y.view(np.uint64) == exp.view(np.uint64)) | (np.isnan(y) & np.isnan(exp))
    assert ok.all(), (x[~ok][:5], y[~ok][:5], exp[~ok][:5])


# ------------------------------------------------------------------ the chain
def test_chain_solver_to_optimize(torch, gpu, matcher):
    """orb_sim3_solver_iterate_batch -> orb_optimize_sim3_batch on the device:
    d_result is passed as d_start without a host copy, and the slot and match
    arrays are the ones the solver was given."""
    import sim3_cases as SC
    from test_gpu_sim3 import Dev, homogeneous

    probs = homogeneous(SC.mixed(16, seed=32))[0]  # the solver finds a Sim3 for 6 of these 8
    dev = Dev(torch, matcher, probs)
    # observations the optimiser can use: the solver's own projections
    b = dev.b
    rng = np.random.default_rng(6)
    b.keys["x"], b.keys["y"] = rng.uniform(0, 640, b.keys.shape), rng.uniform(0, 480, b.keys.shape)
    for i, s in enumerate(dev.ref):
        s1, s2 = b.kf1_slot[i], b.kf2_slot[i]
        for k, i1 in enumerate(s.mvnIndices1):
            b.keys["x"][s1, i1], b.keys["y"][s1, i1] = s.mvP1im1[k]
            i2 = b.index2[i, i1]
            b.keys["x"][s2, i2], b.keys["y"][s2, i2] = s.mvP2im2[k]
    dev.d["keys"] = _dev(torch, b.keys)
    inv = (1.0 / SC.LEVEL_SIGMA2.astype(np.float64)).astype(np.float32)
    out = torch.full((dev.P * OUT.itemsize,), JUNK, dtype=torch.uint8, device="cuda")
    d = dev.d
    dev.setup()
    dev.iterate(SC.MAX_ITERATIONS, ref=False)
    matcher.optimize_sim3_batch(
        dev.P, d["kf1_slot"].data_ptr(), d["kf2_slot"].data_ptr(), d["keys"].data_ptr(),
        d["nkeys"].data_ptr(), d["point_index"].data_ptr(), d["pose"].data_ptr(), dev.S,
        d["points"].data_ptr(), d["match12"].data_ptr(), d["index2"].data_ptr(), dev.res.data_ptr(),
        inv, SC.CAM1, SC.CAM2, out.data_ptr(), th2=10.0, fix_scale=False)
    torch.cuda.synchronize()
    res = dev.results()
    rec = out.cpu().numpy().view(OUT)
    raw = out.cpu().numpy().reshape(-1, OUT.itemsize)
    match = d["match12"].cpu().numpy().view(np.int32).reshape(dev.P, dev.S)
    ran = 0
    for i in range(dev.P):
        if not res["has_sim3"][i]:
            assert (raw[i] == JUNK).all() and np.array_equal(match[i], b.match12[i])
            continue
        ran += 1
        s1, s2 = b.kf1_slot[i], b.kf2_slot[i]
        xy = lambda s: np.stack([b.keys["x"][s], b.keys["y"][s]], 1)
        r = R.optimize_sim3(
            xy(s1), b.keys["octave"][s1], b.point_index[s1], (b.pose["rcw"][s1], b.pose["tcw"][s1]),
            xy(s2), b.keys["octave"][s2], (b.pose["rcw"][s2], b.pose["tcw"][s2]), b.points["pos"],
            b.points["bad"], b.match12[i], b.index2[i], (res["R"][i], res["t"][i], res["scale"][i]),
            inv, SC.CAM1, SC.CAM2, 10.0, False, n1=min(max(b.nkeys[s1], 0), dev.S),
            n2=min(max(b.nkeys[s2], 0), dev.S))
        same(rec[i], R.result_record(r)[0], f"chain {i}")
        n1 = min(max(b.nkeys[s1], 0), dev.S)
        exp = b.match12[i].copy()
        exp[:n1] = r["match12"][:n1] if r["status"] == 0 else exp[:n1]
        assert np.array_equal(match[i], exp), f"chain {i} match12"
    found = sum(s.iterate(SC.MAX_ITERATIONS)[0] is not None for s in dev.ref)
    assert ran == found >= 3
