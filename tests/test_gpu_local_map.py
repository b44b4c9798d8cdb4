"""orb_update_local_map_batch (k_local_map) and TrackLocalMap's two tails on the
GPU against the Python restatement of the reference (tests/local_map_ref.py):
every output array and every info field index-exact, slots past each count
untouched (pinned with a junk fill)."""
import functools

import numpy as np
import pytest

import local_map_cases as C
import local_map_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
JUNK = 77
PSZ = R.MAP_POINT_DTYPE.itemsize


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def matcher(gpu):
    return gpu.ORBmatcher(0.8, True)


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


@functools.lru_cache(maxsize=None)
def combined(names, seed=0):
    return C.combine([C.get(n) for n in names], seed)


def solo(name):
    i = C.get(name)
    return i["map"], [dict(name=name, kp_match=i["kp_match"], local_kf=i["local_kf"],
                           mp_stride=i["mp_stride"])]


class Batch:
    """Device copies of a map and of P problems' arrays, outputs junk-filled."""

    def __init__(self, torch, gpu, m, probs, kp_stride=None, kf_stride=None, mp_stride=None,
                 view=None):
        self.torch, self.gpu, self.m, self.probs = torch, gpu, m, probs
        self.P = P = len(probs)
        self.S = S = kp_stride or max(1, max(len(q["kp_match"]) for q in probs)) + 2
        self.KS = KS = kf_stride or max(1, len(m["rank"]))
        self.MS = MS = mp_stride or max(q["mp_stride"] for q in probs)
        self.view = view or gpu.MapView(**C.view_arrays(m))
        self.nk = np.array([len(q["kp_match"]) for q in probs], np.int32)
        self.km = np.full((P, S), JUNK, np.int32)
        self.lkf = np.full((P, KS), JUNK, np.int32)
        self.nlkf = np.zeros(P, np.int32)
        for p, q in enumerate(probs):
            self.km[p, :self.nk[p]] = q["kp_match"]
            self.lkf[p, :len(q["local_kf"])] = q["local_kf"]
            self.nlkf[p] = len(q["local_kf"])
        t = torch
        self.d = dict(nk=_dev(t, self.nk), km=_dev(t, self.km), lkf=_dev(t, self.lkf),
                      nlkf=_dev(t, self.nlkf),
                      li=t.full((P * MS,), JUNK, dtype=t.int32, device="cuda"),
                      mps=t.full((P * MS * PSZ,), JUNK, dtype=t.uint8, device="cuda"),
                      desc=t.full((P * MS * 32,), JUNK, dtype=t.uint8, device="cuda"),
                      nmps=t.full((P,), JUNK, dtype=t.int32, device="cuda"),
                      locked=t.full((P * S,), JUNK, dtype=t.uint8, device="cuda"),
                      info=t.full((P * 8,), JUNK, dtype=t.int32, device="cuda"))

    def args(self, stream=0, **over):
        d = self.d
        a = dict(n_problems=self.P, view=self.view, d_nkeys=d["nk"].data_ptr(),
                 d_kp_match=d["km"].data_ptr(), kp_stride=self.S, d_local_kf=d["lkf"].data_ptr(),
                 d_n_local_kf=d["nlkf"].data_ptr(), kf_stride=self.KS,
                 d_local_index=d["li"].data_ptr(), d_mps=d["mps"].data_ptr(),
                 d_mp_desc=d["desc"].data_ptr(), d_nmps=d["nmps"].data_ptr(), mp_stride=self.MS,
                 d_locked=d["locked"].data_ptr(), d_info=d["info"].data_ptr(), stream=stream)
        a.update(over)
        return a

    def launch(self, matcher, stream=0, **over):
        matcher.update_local_map_batch(**self.args(stream, **over))

    def host(self):
        self.torch.cuda.synchronize()
        d, P = self.d, self.P
        h = lambda k, dt: d[k].cpu().numpy().view(dt)
        return dict(km=h("km", np.int32).reshape(P, self.S),
                    lkf=h("lkf", np.int32).reshape(P, self.KS), nlkf=h("nlkf", np.int32),
                    li=h("li", np.int32).reshape(P, self.MS),
                    mps=h("mps", np.uint8).reshape(P, self.MS, PSZ),
                    desc=h("desc", np.uint8).reshape(P, self.MS, 32), nmps=h("nmps", np.int32),
                    locked=h("locked", np.uint8).reshape(P, self.S),
                    info=h("info", R.INFO_DTYPE).reshape(P))

    def untouched(self, g):
        """Every output as it was before any call."""
        return (np.array_equal(g["km"], self.km) and np.array_equal(g["lkf"], self.lkf)
                and np.array_equal(g["nlkf"], self.nlkf) and (g["li"] == JUNK).all()
                and (g["mps"] == JUNK).all() and (g["desc"] == JUNK).all()
                and (g["nmps"] == JUNK).all() and (g["locked"] == JUNK).all()
                and (g["info"].view(np.int32) == JUNK).all())

    def check(self, g=None, before=None, tag=""):
        """Against the reference; `before`: (km, lkf, nlkf) on entry when the
        call was not the first on these arrays."""
        g = g or self.host()
        km0, lkf0, nlkf0 = before or (self.km, self.lkf, self.nlkf)
        for p, q in enumerate(self.probs):
            n, t = int(self.nk[p]), (tag, p, q["name"])
            nl0 = min(max(int(nlkf0[p]), 0), self.KS)
            e = R.update_local_map(self.m, km0[p, :n], lkf0[p, :nl0], self.MS)
            assert g["info"][p].tolist() == e["info"].tolist(), (t, g["info"][p], e["info"])
            assert np.array_equal(g["km"][p, :n], e["kp_match"]), t
            assert np.array_equal(g["km"][p, n:], km0[p, n:]), t
            L = len(e["local_kf"])
            assert int(g["nlkf"][p]) == (int(nlkf0[p]) if e["info"]["kept"] else L), t
            assert np.array_equal(g["lkf"][p, :L], e["local_kf"]), (t, g["lkf"][p, :L], e["local_kf"])
            assert np.array_equal(g["lkf"][p, L:], lkf0[p, L:]), t
            k = len(e["local_index"])
            assert int(g["nmps"][p]) == k == min(e["n_local_points"], self.MS), t
            assert np.array_equal(g["li"][p, :k], e["local_index"]), t
            assert (g["li"][p, k:] == JUNK).all(), t
            assert g["mps"][p, :k].tobytes() == e["mps"].tobytes(), t
            assert (g["mps"][p, k:] == JUNK).all(), t
            assert g["desc"][p, :k].tobytes() == e["desc"].tobytes(), t
            assert (g["desc"][p, k:] == JUNK).all(), t
            assert np.array_equal(g["locked"][p, :n], e["locked"]), t
            assert (g["locked"][p, n:] == JUNK).all(), t
        return g


SMALL = tuple(C.SMALL)
LARGE = tuple(C.LARGE)


# ------------------------------------------------------------------ directed
def test_every_directed_input_in_one_mixed_batch(gpu, torch, matcher):
    m, probs = combined(SMALL + LARGE)
    assert len(m["rank"]) <= gpu.update_local_map_max_keyframes()
    b = Batch(torch, gpu, m, probs)
    b.launch(matcher)
    g = b.check()
    info = {q["name"]: g["info"][p] for p, q in enumerate(probs)}
    assert info["tiny"].tolist() == (5, 2, 3, info["tiny"]["ref_kf"], 3, 4, 1, 0)
    assert info["voted79"]["n_local_kf"] == 82 and info["voted80"]["n_local_kf"] == 83
    assert info["voted81"]["n_added"] == 0 and info["voted100"]["n_local_kf"] == 100
    assert info["empty_stale"]["kept"] == 1 and info["all_voted_bad"]["n_local_kf"] == 0
    assert info["over_mp_stride"]["n_local_points"] == 26
    assert info["tier%d" % (C.HASH_CAP + 1)]["n_local_points"] == C.HASH_CAP + 1


@pytest.mark.parametrize("name", SMALL + LARGE)
def test_each_directed_input_alone(gpu, torch, matcher, name):
    m, probs = solo(name)
    b = Batch(torch, gpu, m, probs)
    b.launch(matcher)
    b.check(tag=name)


def test_local_map_smaller_than_the_count(gpu, torch, matcher):
    """mp_stride below n_local_points: the first mp_stride points are written,
    the count is reported in full; also at the scratch tier."""
    for name, ms in (("over_mp_stride", 5), ("points_mix", 1), ("count65", 64), ("tier_mix", 1000)):
        m, probs = solo(name)
        b = Batch(torch, gpu, m, probs, mp_stride=ms)
        b.launch(matcher)
        g = b.check(tag=name)
        assert g["info"][0]["n_local_points"] > ms == g["nmps"][0]


@pytest.mark.parametrize("P", [1, 16, 300])
def test_batch_sizes(gpu, torch, matcher, P):
    m, probs = combined(SMALL)
    order = np.random.default_rng(P).permutation(len(probs))
    sel = [probs[order[i % len(probs)]] for i in range(P)]
    b = Batch(torch, gpu, m, sel)
    b.launch(matcher)
    b.check(tag="P%d" % P)


def test_kept_list_across_two_calls(gpu, torch, matcher):
    """Call 1 builds the lists; the frame then loses every match (and the map
    changes nothing): call 2 keeps call 1's lists and gathers from them."""
    names = ("tiny", "neighbours", "children5", "points_mix", "voted80", "all_voted_bad")
    m, probs = combined(names, 5)
    b = Batch(torch, gpu, m, probs)
    b.launch(matcher)
    g1 = b.check(tag="call1")
    S = b.S
    lost = np.full((b.P, S), JUNK, np.int32)
    for p in range(b.P):
        lost[p, :b.nk[p]] = np.where(np.arange(b.nk[p]) % 2 == 0, -1, -2)
    b.d["km"].copy_(_dev(torch, lost))
    b.launch(matcher)
    g2 = b.check(before=(lost, g1["lkf"], g1["nlkf"]), tag="call2")
    for p, q in enumerate(probs):
        assert g2["info"][p]["kept"] == 1 and g2["info"][p]["n_voted"] == 0
        assert np.array_equal(g2["lkf"][p], g1["lkf"][p]) and g2["nlkf"][p] == g1["nlkf"][p]
        # the same keyframes give the same points; nothing is held any more
        k = int(g1["nmps"][p])
        assert np.array_equal(g2["li"][p, :k], g1["li"][p, :k]) and g2["nmps"][p] == k
        assert (g2["mps"][p, :k, 33] == 0).all() and (g2["locked"][p, :b.nk[p]] == 0).all()
    assert g1["info"][0]["n_local_kf"] == 5 and g2["info"][0]["n_local_kf"] == 5


def test_kf_stride_above_n_kf_and_entry_count_clamped(gpu, torch, matcher):
    m, probs = combined(("tiny", "empty_stale", "tie_max", "voted82"), 2)
    nkf = len(m["rank"])
    b = Batch(torch, gpu, m, probs, kf_stride=nkf + 37, kp_stride=200)
    b.launch(matcher)
    b.check(tag="wide")
    # an entry count outside [0, kf_stride] is clamped: below zero the kept list is empty
    m1, p1 = solo("tiny_empty")
    b = Batch(torch, gpu, m1, p1, kf_stride=7)
    b.d["nlkf"].copy_(_dev(torch, np.array([-3], np.int32)))
    b.launch(matcher)
    g = b.host()
    assert g["info"][0].tolist() == (0, 0, 0, -1, 0, 0, 0, 1) and g["nmps"][0] == 0
    assert g["nlkf"][0] == -3 and (g["li"] == JUNK).all()


def test_status_codes_write_nothing(gpu, torch, matcher):
    m, probs = combined(("tiny", "points_mix"), 1)
    b = Batch(torch, gpu, m, probs)
    E = gpu.OrbError
    bad = [dict(view=None), dict(d_nkeys=0), dict(d_kp_match=0), dict(d_local_kf=0),
           dict(d_n_local_kf=0), dict(d_local_index=0), dict(d_mps=0), dict(d_mp_desc=0),
           dict(d_nmps=0), dict(d_locked=0), dict(d_info=0), dict(n_problems=-1),
           dict(kp_stride=0), dict(mp_stride=0), dict(mp_stride=-4),
           dict(kf_stride=len(m["rank"]) - 1)]
    for over in bad:
        with pytest.raises(E) as err:
            b.launch(matcher, **over)
        assert err.value.status == gpu.ORB_EINVAL, over
    # a null pointer inside the view
    saved = b.view.c.kf_mp
    b.view.c.kf_mp = None
    with pytest.raises(E) as err:
        b.launch(matcher)
    assert err.value.status == gpu.ORB_EINVAL
    b.view.c.kf_mp = saved
    # capacity: before anything is launched
    cap = gpu.update_local_map_max_keyframes()
    with pytest.raises(E) as err:
        b.launch(matcher, kf_stride=cap + 1)
    assert err.value.status == gpu.ORB_ECAPACITY
    n_kf = b.view.c.n_kf
    b.view.c.n_kf = cap + 1
    with pytest.raises(E) as err:
        b.launch(matcher, kf_stride=cap + 1)
    assert err.value.status == gpu.ORB_ECAPACITY
    b.view.c.n_kf = n_kf
    b.launch(matcher, n_problems=0)            # ORB_OK, no launch
    assert b.untouched(b.host())
    b.launch(matcher)                          # and the same arrays still work
    b.check()


def test_capacity_boundary_runs(gpu, torch, matcher):
    """kf_stride at the capacity itself: the largest LDS layout launches."""
    m, probs = solo("points_mix")
    b = Batch(torch, gpu, m, probs, kf_stride=gpu.update_local_map_max_keyframes())
    b.launch(matcher)
    b.check(tag="cap")


def test_two_streams(gpu, torch, matcher):
    """Two batches on two streams through one handle (the scratch tier in both:
    the handle's call-order rule serialises them on the device)."""
    names = ("tier_mix", "points_mix", "tier%d" % (C.HASH_CAP + 1), "voted79")
    m, probs = combined(names, 9)
    view = gpu.MapView(**C.view_arrays(m))
    a = Batch(torch, gpu, m, probs, view=view)
    b = Batch(torch, gpu, m, probs[::-1], view=view)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a.launch(matcher, stream=s1.cuda_stream)
    b.launch(matcher, stream=s2.cuda_stream)
    a.launch(matcher, stream=s2.cuda_stream, d_kp_match=a.d["km"].data_ptr())
    torch.cuda.synchronize()
    b.check(tag="s2")
    # a ran twice on its own outputs: the second run sees the first's nulling and list
    g = a.host()
    for p, q in enumerate(a.probs):
        n = int(a.nk[p])
        e1 = R.update_local_map(m, a.km[p, :n], a.lkf[p, :a.nlkf[p]], a.MS)
        e2 = R.update_local_map(m, e1["kp_match"], e1["local_kf"], a.MS)
        assert g["info"][p].tolist() == e2["info"].tolist(), (p, q["name"])
        assert np.array_equal(g["li"][p, :len(e2["local_index"])], e2["local_index"])


# --------------------------------------------------------------------- tails
def test_merge_every_branch(gpu, torch, matcher):
    rng = np.random.default_rng(3)
    P, S, MS = 5, 300, 90
    nk = np.array([0, 1, 64, 257, 300], np.int32)
    km = rng.integers(-2, 5000, (P, S)).astype(np.int32)
    kl = rng.integers(-1, MS, (P, S)).astype(np.int32)
    kl[rng.random((P, S)) < 0.5] = -1
    kl[1, 0] = 7
    li = rng.integers(0, 5000, (P, MS)).astype(np.int32)
    d_km, d_kl, d_li, d_nk = (_dev(torch, a) for a in (km, kl, li, nk))
    matcher.track_local_merge_batch(P, d_nk.data_ptr(), S, d_kl.data_ptr(), d_li.data_ptr(), MS,
                                    d_km.data_ptr())
    torch.cuda.synchronize()
    g = d_km.cpu().numpy().view(np.int32).reshape(P, S)
    for p in range(P):
        n = nk[p]
        assert np.array_equal(g[p, :n], R.merge(km[p, :n], kl[p, :n], li[p])), p
        assert np.array_equal(g[p, n:], km[p, n:]), p
    assert g[1, 0] == li[1, 7]
    for over in (dict(kp_stride=0), dict(mp_stride=0), dict(n=-1), dict(kl=0), dict(km=0)):
        with pytest.raises(gpu.OrbError) as err:
            matcher.track_local_merge_batch(
                over.get("n", P), d_nk.data_ptr(), over.get("kp_stride", S),
                over.get("kl", d_kl.data_ptr()), d_li.data_ptr(), over.get("mp_stride", MS),
                over.get("km", d_km.data_ptr()))
        assert err.value.status == gpu.ORB_EINVAL, over
    matcher.track_local_merge_batch(0, d_nk.data_ptr(), S, d_kl.data_ptr(), d_li.data_ptr(), MS,
                                    d_km.data_ptr())


@pytest.mark.parametrize("only_tracking", [0, 1])
@pytest.mark.parametrize("null_outliers", [0, 1])
@pytest.mark.parametrize("pt_stride", [0, 400])
def test_finish_every_branch(gpu, torch, matcher, only_tracking, null_outliers, pt_stride):
    rng = np.random.default_rng(4)
    P, S, M = 6, 300, 400
    nk = np.array([0, 1, 63, 65, 256, 300], np.int32)
    km = rng.integers(-2, M, (P, S)).astype(np.int32)
    km[rng.random((P, S)) < 0.3] = -1
    km[1, 0] = 9
    ol = (rng.random((P, S)) < 0.4).astype(np.uint8)
    pts = np.zeros((P if pt_stride else 1, M), R.MAP_POINT_DTYPE)
    pts["has_obs"] = rng.random(pts.shape) < 0.6
    d_km, d_ol, d_pts, d_nk = (_dev(torch, a) for a in (km, ol, pts, nk))
    d_n = torch.full((P,), JUNK, dtype=torch.int32, device="cuda")
    matcher.track_local_map_finish_batch(P, d_nk.data_ptr(), S, d_km.data_ptr(), d_ol.data_ptr(),
                                         d_pts.data_ptr(), pt_stride, only_tracking,
                                         null_outliers, d_n.data_ptr())
    torch.cuda.synchronize()
    g = d_km.cpu().numpy().view(np.int32).reshape(P, S)
    gn = d_n.cpu().numpy()
    for p in range(P):
        n = nk[p]
        e_n, e_km = R.finish(km[p, :n], ol[p, :n], pts[p if pt_stride else 0], only_tracking,
                             null_outliers)
        assert gn[p] == e_n and np.array_equal(g[p, :n], e_km), p
        assert np.array_equal(g[p, n:], km[p, n:]), p
    assert np.array_equal(d_ol.cpu().numpy().reshape(P, S), ol)      # read only
    with pytest.raises(gpu.OrbError) as err:
        matcher.track_local_map_finish_batch(P, d_nk.data_ptr(), 0, d_km.data_ptr(),
                                             d_ol.data_ptr(), d_pts.data_ptr(), pt_stride, 0, 0,
                                             d_n.data_ptr())
    assert err.value.status == gpu.ORB_EINVAL


# --------------------------------------------------------------------- chain
def _chain_map(F, M, K, points, rng):
    """F problems' points (M each, problem f's at f * M) under K keyframes per
    problem: every point is observed by two of its problem's keyframes and
    listed by them (shuffled, some slots NULL); the last four keyframes of a
    problem observe nothing and are reached as neighbours only; covisibles,
    children and parents stay inside the problem."""
    n_kf = F * K
    kf_mp = [[] for _ in range(n_kf)]
    obs = []
    for f in range(F):
        for i in range(M):
            ks = rng.choice(K - 4, 2, replace=False) + f * K
            obs.append([int(k) for k in ks])
            for k in ks:
                kf_mp[k].append(f * M + i)
            if rng.random() < 0.2:       # the last four keyframes get no vote; they list points
                kf_mp[f * K + K - 4 + int(rng.integers(0, 4))].append(f * M + i)
    for k in range(n_kf):
        rng.shuffle(kf_mp[k])
        kf_mp[k] = [x for j, x in enumerate(kf_mp[k]) for x in ((x, -1) if j % 9 == 0 else (x,))]
    grp = lambda k: (k // K) * K
    cov = [[int(grp(k) + (k - grp(k) + d) % K) for d in rng.permutation(np.arange(1, K))[:12]]
           for k in range(n_kf)]
    child = [[k + 1] if (k + 1) % K else [] for k in range(n_kf)]
    parent = np.array([k - 1 if k % K else -1 for k in range(n_kf)], np.int32)
    bad = np.zeros(n_kf, np.uint8)
    bad[rng.integers(0, n_kf, F)] = 1
    return dict(rank=rng.permutation(n_kf).astype(np.int32), bad=bad, parent=parent, cov=cov,
                child=child, kf_mp=kf_mp, obs=obs, points=points, desc=None)


def test_track_local_map_chain(gpu, torch, oracle):
    """Four problems, every intermediate in device memory over ONE shared map:
    motion-model match -> PoseOptimization -> discard -> UpdateLocalMap ->
    isInFrustum -> SearchByProjection(F, localMap) -> merge -> PoseOptimization
    over the view's points -> finish; each stage against its CPU reference on
    the same inputs."""
    import matcher_edge_cases as E
    import poseopt_cases as pc
    import scenarios as S
    import track_motion_ref as TR
    W, H, F, M, NF, K = 1241, 376, 4, 2000, 1000, 24
    cam = S.camera()
    scale = oracle.params(NF)["scale"]
    levels = (f32(1.0) / (scale * scale)).astype(f32)
    LS = f32(E.LS)
    rng0 = np.random.default_rng(11)
    pre = []
    for f in range(F):
        rng = np.random.default_rng(90 + f)
        ka, da, _ = oracle.extract(oracle.synth_image(90 + f, 0, W, H), NF)
        kb, db, _ = oracle.extract(oracle.synth_image(90 + f, 1, W, H), NF)
        pose, P, mpd = S.local_map_3d(oracle, kb, db, M, W, H, rng_seed=90 + f)
        P["seen"] = rng.random(M) < 0.3          # the map's own byte is not this frame's
        P["bad"] = rng.random(M) < 0.03
        P0 = P.copy()
        P0["seen"], P0["bad"] = 0, 0
        _, tr0 = oracle.frustum(P0, pose, cam, W, H, 0.5, LS, 8)
        px = np.where(tr0["in_view"] != 0, tr0["proj_x"], 1e9)
        d2 = ((ka["x"][:, None] + S._ego_shift(90 + f) - px[None, :]) ** 2
              + (ka["y"][:, None] - tr0["proj_y"][None, :]) ** 2)
        near = d2.argmin(1)
        lidx = np.where((d2[np.arange(len(ka)), near] < 16.0) & (rng.random(len(ka)) < 0.9),
                        near, -1).astype(np.int32)
        last_pose = TR.pose(pose["rcw"][0].reshape(3, 3), pose["tcw"][0] + np.array([0, 0, 0.3], f32))
        pre.append(dict(ka=ka, kb=kb, db=db, pose=pose, last_pose=last_pose, P=P, mpd=mpd, lidx=lidx))
    Pall = np.concatenate([c["P"] for c in pre])
    mdall = np.concatenate([c["mpd"] for c in pre])
    m = _chain_map(F, M, K, Pall, rng0)
    m["desc"] = mdall
    MS = M + 8
    glob = lambda a, f: np.where(a >= 0, a + f * M, a).astype(np.int32)
    q = []
    for f, c in enumerate(pre):
        kb, db, P, pose = c["kb"], c["db"], c["P"], c["pose"]
        n = len(kb)
        prob = dict(keys=kb, desc=db, u_right=None, locked=None, pose_cur=pose,
                    pose_last=c["last_pose"], last_keys=c["ka"], last_point_index=c["lidx"],
                    last_outlier=None, points=P, mp_desc=c["mpd"])
        km3, info3 = TR.search(oracle, prob, cam, scale, W, H, 15.0, True, True, 20)
        ur = np.full(n, -1, f32)
        xy = np.stack([kb["x"], kb["y"]], 1)
        r4 = pc.ref.pose_optimization(xy, kb["octave"], ur, km3, P["pos"], levels, cam,
                                      pose["rcw"][0], pose["tcw"][0], pose["ow"][0],
                                      np.full(n, pc.SENTINEL, np.uint8))
        km5, ol5, _, out5 = TR.discard_outliers(km3, r4["outlier"], P, info3["n_matches"], False)
        e8 = R.update_local_map(m, glob(km5, f), [], MS)
        pose2 = np.zeros(1, gpu.POSE_DTYPE)
        pose2["rcw"], pose2["tcw"], pose2["ow"] = r4["rcw"], r4["tcw"], r4["ow"]
        n6, tr6 = oracle.frustum(e8["mps"], pose2, cam, W, H, 0.5, LS, 8)
        nm7, km7 = oracle.match_projection_local(kb, db, scale, W, H, tr6, e8["desc"], 3.0, 0.8,
                                                 e8["locked"])
        km9 = R.merge(e8["kp_match"], km7, e8["local_index"])
        r10 = pc.ref.pose_optimization(xy, kb["octave"], ur, km9, Pall["pos"], levels, cam,
                                       r4["rcw"], r4["tcw"], r4["ow"],
                                       np.full(n, pc.SENTINEL, np.uint8))
        n11, km11 = R.finish(km9, r10["outlier"], Pall, False, True)
        assert info3["n_matches"] > 100 and out5["n_discarded"] > 0 and nm7 > 30
        assert e8["info"]["n_nulled"] > 0 and e8["info"]["n_added"] > 0
        assert 500 < e8["n_local_points"] <= M and (e8["mps"]["seen"] != 0).sum() > 50
        assert n11 > 50 and (km11 != km9).any()
        q.append(dict(c, n=n, km3=km3, info3=info3, r4=r4, km5=km5, ol5=ol5, out5=out5, e8=e8,
                      n6=n6, tr6=tr6, nm7=nm7, km7=km7, km9=km9, r10=r10, n11=n11, km11=km11))
    cap = max(max(len(c["ka"]), len(c["kb"])) for c in pre) + 5
    keys = np.zeros((2 * F, cap), gpu.KEYPOINT_DTYPE)
    desc = np.zeros((F, cap, 32), np.uint8)
    cnt = np.zeros(2 * F, np.int32)
    lidx = np.full((F, cap), -1, np.int32)
    pcur, plast = np.zeros(F, gpu.POSE_DTYPE), np.zeros(F, gpu.POSE_DTYPE)
    for f, c in enumerate(pre):
        keys[f, :len(c["ka"])], keys[F + f, :len(c["kb"])] = c["ka"], c["kb"]
        desc[f, :len(c["kb"])] = c["db"]
        cnt[f], cnt[F + f] = len(c["ka"]), len(c["kb"])
        lidx[f, :len(c["lidx"])] = glob(c["lidx"], f)
        pcur[f], plast[f] = c["pose"][0], c["last_pose"][0]
    view = gpu.MapView(**C.view_arrays(m))
    d_keys, d_desc, d_cnt, d_lidx, d_pcur, d_plast = (_dev(torch, a) for a in
                                                      (keys, desc, cnt, lidx, pcur, plast))
    t = torch
    i32 = lambda n, v=JUNK: t.full((n,), v, dtype=t.int32, device="cuda")
    u8 = lambda n, v=JUNK: t.full((n,), v, dtype=t.uint8, device="cuda")
    d_ur = t.full((F * cap,), -1.0, dtype=t.float32, device="cuda")
    d_km, d_info3, d_info4, d_out5 = i32(F * cap).view(F, cap), i32(F * 5), i32(F * 4), i32(F * 3)
    d_pout, d_pout2 = u8(F * gpu.POSE_DTYPE.itemsize, 0), u8(F * gpu.POSE_DTYPE.itemsize, 0)
    d_outl, d_outl2 = u8(F * cap, pc.SENTINEL), u8(F * cap, pc.SENTINEL)
    d_lkf, d_nlkf, d_li = i32(F * F * K), i32(F, 0), i32(F * MS)
    d_mps, d_md8, d_nmps = u8(F * MS * PSZ), u8(F * MS * 32), i32(F)
    d_locked, d_info8 = u8(F * cap), i32(F * 8)
    d_tr, d_cnt6 = u8(F * MS * gpu.MP_TRACK_DTYPE.itemsize, 0), i32(F)
    d_km7, d_nm7, d_info10, d_inl = i32(F * cap), i32(F), i32(F * 4), i32(F)
    k_cur, n_cur = d_keys.data_ptr() + F * cap * 28, d_cnt.data_ptr() + F * 4
    d_P, d_mdall = view.dev["points"], view.dev["mp_desc"]
    mt = gpu.ORBmatcher(0.8, True)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = st.cuda_stream
    with torch.cuda.stream(st):
        mt.search_by_projection_frame_batch(
            F, k_cur, d_desc.data_ptr(), 0, 0, n_cur, cap, d_pcur.data_ptr(), d_plast.data_ptr(),
            d_keys.data_ptr(), d_cnt.data_ptr(), d_lidx.data_ptr(), 0, d_P.data_ptr(),
            d_mdall.data_ptr(), 0, cam, 0.0, float(W), 0.0, float(H), scale, 15.0, True, 20,
            d_km.data_ptr(), d_info3.data_ptr(), stream=s)
        km3 = d_km.clone()
        mt.pose_optimization_batch(F, n_cur, k_cur, d_ur.data_ptr(), cap, d_km.data_ptr(),
                                   d_P.data_ptr(), PSZ, 0, levels, cam, d_pcur.data_ptr(),
                                   d_pout.data_ptr(), d_outl.data_ptr(), d_info4.data_ptr(), stream=s)
        mt.track_discard_outliers_batch(F, n_cur, cap, d_km.data_ptr(), d_outl.data_ptr(),
                                        d_P.data_ptr(), 0, False, d_info3.data_ptr(),
                                        d_out5.data_ptr(), stream=s)
        km5 = d_km.clone()
        mt.update_local_map_batch(F, view, n_cur, d_km.data_ptr(), cap, d_lkf.data_ptr(),
                                  d_nlkf.data_ptr(), F * K, d_li.data_ptr(), d_mps.data_ptr(),
                                  d_md8.data_ptr(), d_nmps.data_ptr(), MS, d_locked.data_ptr(),
                                  d_info8.data_ptr(), stream=s)
        km8 = d_km.clone()
        mt.frustum_batch(F, d_mps.data_ptr(), d_nmps.data_ptr(), MS, d_pout.data_ptr(), cam, 0.0,
                         float(W), 0.0, float(H), 0.5, LS, 8, d_tr.data_ptr(), d_cnt6.data_ptr(),
                         stream=s)
        mt.search_by_projection_batch(F, k_cur, d_desc.data_ptr(), n_cur, d_locked.data_ptr(), cap,
                                      d_tr.data_ptr(), d_md8.data_ptr(), d_nmps.data_ptr(), MS, W, H,
                                      scale, 3.0, d_km7.data_ptr(), d_nm7.data_ptr(), stream=s)
        mt.track_local_merge_batch(F, n_cur, cap, d_km7.data_ptr(), d_li.data_ptr(), MS,
                                   d_km.data_ptr(), stream=s)
        km9 = d_km.clone()
        mt.pose_optimization_batch(F, n_cur, k_cur, d_ur.data_ptr(), cap, d_km.data_ptr(),
                                   d_P.data_ptr(), PSZ, 0, levels, cam, d_pout.data_ptr(),
                                   d_pout2.data_ptr(), d_outl2.data_ptr(), d_info10.data_ptr(),
                                   stream=s)
        mt.track_local_map_finish_batch(F, n_cur, cap, d_km.data_ptr(), d_outl2.data_ptr(),
                                        d_P.data_ptr(), 0, False, True, d_inl.data_ptr(), stream=s)
    torch.cuda.synchronize()
    H_ = lambda x, dt=np.int32: x.cpu().numpy().reshape(-1).view(dt)
    h_km3, h_km5, h_km8, h_km9, h_km11 = (H_(x).reshape(F, cap) for x in (km3, km5, km8, km9, d_km))
    info3 = H_(d_info3, TR.INFO_DTYPE)
    info4, info10 = H_(d_info4, gpu.POSE_OPT_INFO_DTYPE), H_(d_info10, gpu.POSE_OPT_INFO_DTYPE)
    out5, info8 = H_(d_out5, TR.DISCARD_DTYPE), H_(d_info8, R.INFO_DTYPE)
    pout, pout2 = H_(d_pout, gpu.POSE_DTYPE), H_(d_pout2, gpu.POSE_DTYPE)
    outl2 = H_(d_outl2, np.uint8).reshape(F, cap)
    li, nmps = H_(d_li).reshape(F, MS), H_(d_nmps)
    mps = H_(d_mps, np.uint8).reshape(F, MS, PSZ)
    md8 = H_(d_md8, np.uint8).reshape(F, MS, 32)
    locked = H_(d_locked, np.uint8).reshape(F, cap)
    tr6 = H_(d_tr, gpu.MP_TRACK_DTYPE).reshape(F, MS)
    km7, nm7, cnt6, inl = H_(d_km7).reshape(F, cap), H_(d_nm7), H_(d_cnt6), H_(d_inl)
    po = ("n_inliers", "n_edges", "lm_iterations", "rejected_trials")
    for f, c in enumerate(q):
        n, e8 = c["n"], c["e8"]
        # motion-model match over the shared points (global indices)
        assert np.array_equal(h_km3[f, :n], glob(c["km3"], f)) and (h_km3[f, n:] == JUNK).all(), f
        assert info3[f].tolist() == c["info3"].tolist(), f
        # PoseOptimization, discard (no marking: the shared map is read only)
        assert tuple(int(info4[f][k]) for k in po) == tuple(c["r4"][k] for k in po), f
        for k in ("rcw", "tcw", "ow"):
            assert pout[f][k].tobytes() == np.asarray(c["r4"][k], f32).tobytes(), (f, k)
        assert np.array_equal(h_km5[f, :n], glob(c["km5"], f)), f
        assert out5[f].tolist() == c["out5"].tolist(), f
        # UpdateLocalMap
        assert info8[f].tolist() == e8["info"].tolist(), (f, info8[f], e8["info"])
        assert np.array_equal(h_km8[f, :n], e8["kp_match"]) and (h_km8[f, n:] == JUNK).all(), f
        k8 = len(e8["local_index"])
        assert nmps[f] == k8 and np.array_equal(li[f, :k8], e8["local_index"]), f
        assert mps[f, :k8].tobytes() == e8["mps"].tobytes() and (mps[f, k8:] == JUNK).all(), f
        assert md8[f, :k8].tobytes() == e8["desc"].tobytes(), f
        assert np.array_equal(locked[f, :n], e8["locked"]), f
        # isInFrustum and SearchByProjection(F, localMap) on the gathered arrays
        assert cnt6[f] == c["n6"] and tr6[f, :k8].tobytes() == c["tr6"].tobytes(), f
        assert nm7[f] == c["nm7"] and np.array_equal(km7[f, :n], c["km7"]), f
        # merge, PoseOptimization over the view's points, finish
        assert np.array_equal(h_km9[f, :n], c["km9"]) and (h_km9[f, n:] == JUNK).all(), f
        assert tuple(int(info10[f][k]) for k in po) == tuple(c["r10"][k] for k in po), f
        for k in ("rcw", "tcw", "ow"):
            assert pout2[f][k].tobytes() == np.asarray(c["r10"][k], f32).tobytes(), (f, k)
        assert np.array_equal(outl2[f, :n], c["r10"]["outlier"]), f
        assert inl[f] == c["n11"] and np.array_equal(h_km11[f, :n], c["km11"]), f
        assert (h_km11[f, n:] == JUNK).all(), f
    # the shared map was never written
    assert view.dev["points"].cpu().numpy().tobytes() == Pall.tobytes()
