"""The device-batched SearchByProjection(CurrentFrame, LastFrame) with
TrackWithMotionModel's retry (k_frame_batch) and the discard / marking kernel
(k_track_discard) against the CPU: the C++ oracle's match_projection_frame on
the records tests/track_motion_ref.py derives from the poses, once per problem
and a second time for a retry.  kp_match index-exact, every info field exact,
the slots past a problem's keypoint count untouched."""
import functools

import numpy as np
import pytest

import matcher_edge_cases as E
import scenarios as S
import track_motion_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
JUNK = 77
INFO_FIELDS = ("n_matches", "n_matches_first_pass", "retried", "forward", "backward")


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def matchers(gpu):
    return {ori: gpu.ORBmatcher(0.9, bool(ori)) for ori in (0, 1)}


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


class Packed:
    pass


def pack(torch, probs, stride, mp_stride, shared=None):
    """Device arrays of a batch in the extractor batch's layout; the padding
    keypoints are NaN, the padding last-frame entries NULL."""
    P = len(probs)
    keys = np.zeros(P * stride, R.KEYPOINT_DTYPE)
    keys["x"] = keys["y"] = np.nan
    desc = np.zeros((P * stride, 32), np.uint8)
    ur = np.full(P * stride, -1, f32)
    lk = np.zeros(P * stride, np.uint8)
    nk, ln = np.zeros(P, np.int32), np.zeros(P, np.int32)
    pc, pl = np.zeros(P, R.POSE_DTYPE), np.zeros(P, R.POSE_DTYPE)
    lkeys = np.zeros(P * stride, R.KEYPOINT_DTYPE)
    lidx = np.full(P * stride, -1, np.int32)
    lout = np.zeros(P * stride, np.uint8)
    if shared is None:
        pts = np.zeros(max(P * mp_stride, 1), R.MAP_POINT_DTYPE)
        md = np.zeros((max(P * mp_stride, 1), 32), np.uint8)
    else:
        assert mp_stride == 0
        pts, md = shared
    for p, pr in enumerate(probs):
        n, m, b = len(pr["keys"]), len(pr["last_keys"]), p * stride
        assert n <= stride and m <= stride
        keys[b:b + n], desc[b:b + n] = pr["keys"], pr["desc"]
        if pr.get("u_right") is not None:
            ur[b:b + n] = pr["u_right"]
        if pr.get("locked") is not None:
            lk[b:b + n] = pr["locked"]
        nk[p], ln[p], pc[p], pl[p] = n, m, pr["pose_cur"][0], pr["pose_last"][0]
        lkeys[b:b + m], lidx[b:b + m] = pr["last_keys"], pr["last_point_index"]
        if pr.get("last_outlier") is not None:
            lout[b:b + m] = pr["last_outlier"]
        if shared is None:
            k = len(pr["points"])
            assert k <= mp_stride
            pts[p * mp_stride:p * mp_stride + k] = pr["points"]
            md[p * mp_stride:p * mp_stride + k] = pr["mp_desc"]
    d = Packed()
    d.P, d.stride, d.mp_stride, d.nk = P, stride, mp_stride, nk
    for name, a in dict(keys=keys, desc=desc, ur=ur, lk=lk, nkeys=nk, ln=ln, pc=pc, pl=pl,
                        lkeys=lkeys, lidx=lidx, lout=lout, pts=pts, md=md).items():
        setattr(d, name, _dev(torch, a))
    d.km = torch.full((P * stride,), JUNK, dtype=torch.int32, device="cuda")
    d.info = torch.full((P * 5,), JUNK, dtype=torch.int32, device="cuda")
    return d


def launch(m, d, th, mono, retry, cam=E.CAM, scale=E.SCALE, w=E.W, h=E.H, ur=True, locked=True,
           outlier=True, stream=0, **over):
    a = dict(n_problems=d.P, kp_stride=d.stride, mp_stride=d.mp_stride, d_keys=d.keys.data_ptr(),
             max_x=float(w), min_x=0.0, scale=scale, retry=retry, cam=cam)
    a.update(over)
    m.search_by_projection_frame_batch(
        a["n_problems"], a["d_keys"], d.desc.data_ptr(), d.ur.data_ptr() if ur else 0,
        d.lk.data_ptr() if locked else 0, d.nkeys.data_ptr(), a["kp_stride"], d.pc.data_ptr(),
        d.pl.data_ptr(), d.lkeys.data_ptr(), d.ln.data_ptr(), d.lidx.data_ptr(),
        d.lout.data_ptr() if outlier else 0, d.pts.data_ptr(), d.md.data_ptr(), a["mp_stride"],
        a["cam"], a["min_x"], a["max_x"], 0.0, float(h), a["scale"], th, bool(mono), a["retry"],
        d.km.data_ptr(), d.info.data_ptr(), stream)


def results(torch, d):
    torch.cuda.synchronize()
    km = d.km.cpu().numpy().reshape(d.P, d.stride)
    info = d.info.cpu().numpy().view(R.INFO_DTYPE).reshape(d.P)
    return km, info


def check(km, info, d, refs, tag):
    for p, (rkm, rinfo) in enumerate(refs):
        n = int(d.nk[p])
        got = tuple(int(info[p][f]) for f in INFO_FIELDS)
        want = tuple(int(rinfo[f]) for f in INFO_FIELDS)
        bad = np.nonzero(km[p, :n] != rkm)[0]
        assert len(bad) == 0, (tag, p, bad[:8], km[p, :n][bad[:8]], rkm[bad[:8]])
        assert got == want, (tag, p, got, want)
        assert (km[p, n:] == JUNK).all(), (tag, p, "slots past the count were written")


def run(gpu, torch, oracle, m, probs, th, mono, retry, stride=None, mp_stride=None, shared=None,
        tag="", cam=E.CAM, scale=E.SCALE, w=E.W, h=E.H, refs=None, **opt):
    stride = stride or max(1, max(max(len(p["keys"]), len(p["last_keys"])) for p in probs))
    if mp_stride is None:
        mp_stride = 0 if shared is not None else max(len(p["points"]) for p in probs)
    d = pack(torch, probs, stride, mp_stride, shared)
    launch(m, d, th, mono, retry, cam, scale, w, h, **opt)
    km, info = results(torch, d)
    if refs is None:
        refs = [R.search(oracle, ref_view(p, **opt), cam, scale, w, h, th, mono,
                         m.mbCheckOrientation, retry) for p in probs]
    check(km, info, d, refs, tag)
    return km, info, refs


def ref_view(p, ur=True, locked=True, outlier=True, **_):
    """The problem as the call sees it when an optional array is passed as NULL."""
    q = dict(p)
    if not ur:
        q["u_right"] = None
    if not locked:
        q["locked"] = None
    if not outlier:
        q["last_outlier"] = None
    return q


# -------------------------------------------------------------------- scenes
@functools.lru_cache(maxsize=None)
def crowd(nkeys, n, seed, stereo=False, tlc_z=0.0, th=10.0):
    c = E.crowded_frame(nkeys=nkeys, n=n, seed=seed, stereo=stereo, tlc_z=tlc_z, th=th)
    return R.problem_from_records(c["keys"], c["desc"], c["last"], c["last_desc"], c["tlc_z"],
                                  c["locked"], c["u_right"])


def moved(prob, Rm, t, dz):
    """The same scene seen through the pose (Rm, t): the points go to the world
    frame (R^T (Pc - t), rounded to float), the last pose is the current one
    pushed dz along the optical axis, so tlc.z ~ dz."""
    q = dict(prob)
    pts = prob["points"].copy()
    pcam = pts["pos"].astype(np.float64)
    pts["pos"] = ((pcam - np.asarray(t, np.float64)) @ np.asarray(Rm, np.float64)).astype(f32)
    q["points"] = pts
    q["pose_cur"] = R.pose(Rm, t)
    q["pose_last"] = R.pose(Rm, np.asarray(t, f32) + np.array([0, 0, dz], f32))
    return q


SIZES_LAST = (0, 1, 63, 64, 65, 257)
SIZES_CUR = (0, 1, 31, 32, 33, 1000)


@functools.lru_cache(maxsize=None)
def size_grid():
    return tuple(crowd(n, m, 200 + 7 * i + j) for i, m in enumerate(SIZES_LAST)
                 for j, n in enumerate(SIZES_CUR))


# --------------------------------------------------------------------- sizes
def test_sizes_and_mixed_counts(gpu, torch, oracle, matchers):
    """Every (n_last, n) pair in one batch of 36 problems at stride 1000: mixed
    counts, empty problems in the middle, 0 / 1 / 63 / 64 / 65 / 257 points
    around the replay's 64-point window, 0 / 1 / 31 / 32 / 33 / 1000 keypoints
    around the lock bitmap's word edge."""
    probs = list(size_grid())
    assert len(probs[14]["keys"]) > 0 and len(probs[18]["keys"]) == 0
    _, info, _ = run(gpu, torch, oracle, matchers[1], probs, 10.0, True, 0, stride=1000, tag="grid")
    assert info["n_matches"].max() > 50


@pytest.mark.parametrize("n_problems", [1, 16, 300])
def test_batch_sizes(gpu, torch, oracle, matchers, n_problems):
    """1, 16 and 300 problems (more workgroups than the chip has CUs)."""
    grid = size_grid()
    probs = [grid[(5 * i + 35) % len(grid)] for i in range(n_problems)]
    cache = {}
    refs = []
    for p in probs:
        if id(p) not in cache:
            cache[id(p)] = R.search(oracle, p, E.CAM, E.SCALE, E.W, E.H, 10.0, True, True, 20)
        refs.append(cache[id(p)])
    run(gpu, torch, oracle, matchers[1], probs, 10.0, True, 20, stride=1000, refs=refs,
        tag=n_problems)


# -------------------------------------------------------------------- motion
ROT = S._rot(0.05, -0.08, 0.11).astype(f32)
T = np.array([0.4, -0.3, 0.7], f32)


@pytest.mark.parametrize("kind", ["mono", "fwd", "bwd", "neither"])
def test_motion_cases_decided_on_the_device(gpu, torch, oracle, matchers, kind):
    mono = kind == "mono"
    dz = dict(mono=1.0, fwd=1.0, bwd=-1.0, neither=0.0)[kind]
    base = [crowd(400, 600, 31 + i, stereo=not mono) for i in range(3)]
    probs = [moved(p, ROT, T, dz) for p in base] + [moved(base[0], np.eye(3), (0, 0, 0), dz)]
    _, info, _ = run(gpu, torch, oracle, matchers[1], probs, 10.0, mono, 0, tag=kind)
    want = dict(mono=(0, 0), fwd=(1, 0), bwd=(0, 1), neither=(0, 0))[kind]
    assert all((int(i["forward"]), int(i["backward"])) == want for i in info)
    assert info["n_matches"].min() > 50


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_tlc_z_equal_to_mb(gpu, torch, oracle, matchers, sign):
    """tlc.z == +-mb exactly is neither forward nor backward; one float further it is."""
    mb = f32(E.CAM[5])
    up = np.nextafter(mb, f32(np.inf))
    probs = []
    for z in (sign * mb, sign * up):
        p = dict(crowd(300, 200, 41, stereo=True))
        p["pose_last"] = R.pose(t=(0, 0, z))
        probs.append(p)
    _, info, _ = run(gpu, torch, oracle, matchers[1], probs, 10.0, False, 0, tag=sign)
    assert (int(info[0]["forward"]), int(info[0]["backward"])) == (0, 0)
    assert (int(info[1]["forward"]), int(info[1]["backward"])) == ((1, 0) if sign > 0 else (0, 1))


@pytest.mark.parametrize("seed,mono,th", [(2, True, 15.0), (5, False, 7.0)])
def test_rotated_natural_scene(gpu, torch, oracle, matchers, seed, mono, th):
    """scenarios.frame_pair scenes (extracted frames, KITTI camera), the map
    points back-projected through a rotated pose."""
    fp = S.frame_pair(oracle, seed, rng_seed=seed)
    rng = np.random.default_rng(seed)
    n = len(fp["kb"])
    ur = None if mono else np.where(rng.random(n) < 0.6,
                                    fp["kb"]["x"] - rng.uniform(3, 60, n), -1).astype(f32)
    locked = (rng.random(n) < 0.1).astype(np.uint8)
    base = R.problem_from_records(fp["kb"], fp["db"], fp["last"], fp["last_desc"], 0.0, locked, ur)
    Rm, t, _ = S.pose(rng)
    probs = [moved(base, Rm, t, 1.0), moved(base, Rm, t, -1.0)]
    _, info, _ = run(gpu, torch, oracle, matchers[1], probs, th, mono, 20, cam=S.camera(),
                     scale=fp["scale"], w=fp["w"], h=fp["h"], tag=seed)
    assert info["n_matches"].min() > 100


# --------------------------------------------------------------------- retry
def retry_problem(n_near, n_far, seed):
    """n_near + n_far keypoints 40 px apart, octave 0, each with a point carrying
    its exact descriptor: n_near project 1 px from their keypoint (inside th =
    3), n_far 5 px from it (outside 3, inside 6)."""
    rng = np.random.default_rng(seed)
    n = n_near + n_far
    kx = (40.0 + 40.0 * (np.arange(n) % 14)).astype(f32)
    ky = (40.0 + 40.0 * (np.arange(n) // 14)).astype(f32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    keys = E.keypoints(kx, ky)
    off = np.where(np.arange(n) < n_near, 1.0, 5.0).astype(f32)
    last = E.last_points(kx + off, ky, 0)
    return R.problem_from_records(keys, desc, last, desc, 0.0)


def test_retry_per_problem(gpu, torch, oracle, matchers):
    m = matchers[0]
    a, b, c = retry_problem(19, 0, 1), retry_problem(20, 0, 2), retry_problem(19, 5, 3)
    probs = [b, c, a, b, c]
    km, info, refs = run(gpu, torch, oracle, m, probs, 3.0, True, 20, tag="retry")
    assert [int(i["retried"]) for i in info] == [0, 1, 1, 0, 1]
    assert [int(i["n_matches_first_pass"]) for i in info] == [20, 19, 19, 20, 19]
    assert [int(i["n_matches"]) for i in info] == [20, 24, 19, 20, 24]
    # the retried output is the oracle's second call alone
    last, ld = R.last_records(c["pose_cur"], c["last_keys"], c["last_point_index"], None,
                              c["points"], c["mp_desc"])
    n2, km2 = oracle.match_projection_frame(c["keys"], c["desc"], E.SCALE, E.W, E.H, last, ld,
                                            E.CAM, 0.0, 6.0, 1, 0)
    assert n2 == 24 and np.array_equal(km[1, :24], km2) and np.array_equal(km[4, :24], km2)
    # retry_below 0: nothing is rerun
    _, info0, _ = run(gpu, torch, oracle, m, probs, 3.0, True, 0, tag="no retry")
    assert not info0["retried"].any() and [int(i["n_matches"]) for i in info0] == [20, 19, 19, 20, 19]


# ------------------------------------------------- the directed edge-case inputs
def frame_case_names():
    return sorted(n for n in E.CASES if "frame" in n and not n.startswith("bow"))


@functools.lru_cache(maxsize=None)
def edge_case(name):
    c = E.CASES[name][0]()
    assert c["family"] == "frame"
    p = R.problem_from_records(c["keys"], c["desc"], c["last"], c["last_desc"], c["tlc_z"],
                               c["locked"], c["u_right"])
    return c, p


@pytest.mark.parametrize("name", frame_case_names())
def test_edge_case_alone(gpu, torch, oracle, matchers, name):
    c, p = edge_case(name)
    km, info, _ = run(gpu, torch, oracle, matchers[int(bool(c["check_ori"]))], [p], c["th"],
                      c["mono"], 0, tag=name)
    n, ref = E.run_oracle(oracle, c)   # the generator's own records and tlc_z
    assert int(info[0]["n_matches"]) == n
    assert np.array_equal(km[0, :len(ref)], np.where(ref >= 0, ref - 1000, ref))
    if c.get("expect") is not None:
        assert np.array_equal(ref, c["expect"])


def test_edge_cases_together(gpu, torch, oracle, matchers):
    """All of them in as few batches as their host parameters (th, mono,
    check_orientation) allow, at one stride."""
    groups = {}
    for name in frame_case_names():
        c, p = edge_case(name)
        groups.setdefault((float(c["th"]), int(c["mono"]), int(bool(c["check_ori"]))), []).append(p)
    stride = max(max(len(p["keys"]), len(p["last_keys"])) for g in groups.values() for p in g)
    assert len(groups) < len(frame_case_names())
    for (th, mono, ori), probs in sorted(groups.items()):
        run(gpu, torch, oracle, matchers[ori], probs, th, mono, 0, stride=stride,
            tag=(th, mono, ori))


# ----------------------------------------------------------- optional inputs
@pytest.mark.parametrize("ur,locked,outlier", [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0),
                                               (0, 0, 0)])
def test_optional_inputs(gpu, torch, oracle, matchers, ur, locked, outlier):
    rng = np.random.default_rng(9)
    probs = []
    for i in range(3):
        p = dict(crowd(400, 600, 51 + i, stereo=True))
        p["last_outlier"] = (rng.random(600) < 0.2).astype(np.uint8)
        probs.append(p)
    full = [R.search(oracle, p, E.CAM, E.SCALE, E.W, E.H, 10.0, False, True, 0)[0] for p in probs]
    km, _, _ = run(gpu, torch, oracle, matchers[1], probs, 10.0, False, 0, ur=bool(ur),
                   locked=bool(locked), outlier=bool(outlier), tag=(ur, locked, outlier))
    if not (ur and locked and outlier):   # each array changes the answer when given
        assert any(not np.array_equal(km[i, :400], full[i]) for i in range(3))


# ------------------------------------------- map arrays and last-frame indices
def index_variants():
    """Three problems over one map-point array: the scene as it is; the last
    frame in reverse order; and one with a point held by two last-frame
    keypoints and with -1 and -2 entries."""
    a = dict(crowd(400, 600, 61))
    b = dict(a)
    b["last_keys"] = a["last_keys"][::-1].copy()
    b["last_point_index"] = a["last_point_index"][::-1].copy()
    c = dict(a)
    idx = a["last_point_index"].copy()
    live = np.nonzero(idx >= 0)[0]
    idx[live[1:40:2]] = idx[live[0:39:2]]      # two keypoints, one map point
    idx[live[40:60]] = -1
    idx[live[60:80]] = -2
    c["last_point_index"] = idx
    return [a, b, c]


def test_shared_and_per_problem_map_arrays(gpu, torch, oracle, matchers):
    probs = index_variants()
    shared = (probs[0]["points"], probs[0]["mp_desc"])
    k0, i0, refs = run(gpu, torch, oracle, matchers[1], probs, 10.0, True, 0, shared=shared,
                       tag="shared")
    k1, i1, _ = run(gpu, torch, oracle, matchers[1], probs, 10.0, True, 0, mp_stride=700,
                    refs=refs, tag="per problem")
    assert np.array_equal(k0, k1) and i0.tobytes() == i1.tobytes()
    assert not np.array_equal(refs[0][0], refs[2][0])
    held_twice = probs[2]["last_point_index"]
    assert (np.bincount(held_twice[held_twice >= 0]) == 2).sum() >= 15


def test_batch_of_one_equals_the_one_problem_entry(gpu, torch, oracle, matchers):
    """orb_match_projection_frame on host-projected inputs (mp_id = index)."""
    m = matchers[1]
    for p, mono, z in ((crowd(400, 600, 71), True, 0.0),
                       (moved(crowd(400, 600, 72, stereo=True), ROT, T, 1.0), False, None)):
        km, info, _ = run(gpu, torch, oracle, m, [p], 10.0, mono, 0, tag="one")
        last, ld = R.last_records(p["pose_cur"], p["last_keys"], p["last_point_index"], None,
                                  p["points"], p["mp_desc"])
        tz = float(R.tlc(p["pose_cur"], p["pose_last"])[2])
        F = gpu.Frame(p["keys"], p["desc"], E.SCALE, E.W, E.H, p["u_right"])
        n1, km1 = m.SearchByProjectionFrame(F, last, ld, E.CAM, tz, 10.0, mono, p["locked"])
        assert n1 == int(info[0]["n_matches"]) and np.array_equal(km1, km[0, :len(km1)])


# -------------------------------------------------------------------- errors
def test_capacity_and_bad_arguments(gpu, torch, oracle, matchers):
    m = matchers[1]
    cap = gpu.ORBmatcher.search_by_projection_frame_batch_max_stride()
    assert 4096 <= cap < (1 << 14)
    p = crowd(300, 200, 41)
    d = pack(torch, [p], 300, 200)

    def refused(status, **over):
        with pytest.raises(gpu.OrbError) as err:
            launch(m, d, 10.0, True, **dict(dict(retry=0), **over))
        assert err.value.status == status, over
        km, info = results(torch, d)
        assert (km == JUNK).all() and (info.view(np.int32) == JUNK).all(), over  # nothing ran

    refused(gpu.ORB_ECAPACITY, kp_stride=cap + 1)
    for over in (dict(n_problems=-1), dict(kp_stride=0), dict(kp_stride=-5), dict(mp_stride=-1),
                 dict(scale=np.zeros(0, f32)), dict(scale=np.ones(17, f32)), dict(max_x=0.0),
                 dict(retry=-1), dict(d_keys=0), dict(n_problems=65536)):
        refused(gpu.ORB_EINVAL, **over)
    # the largest stride runs (dynamic LDS above 64 KiB), and the handle still works after
    probs = [crowd(1000, 257, 235), crowd(33, 65, 221)]
    run(gpu, torch, oracle, m, probs, 10.0, True, 0, stride=cap, tag="largest stride")
    launch(m, d, 10.0, True, 0)
    km, info = results(torch, d)
    check(km, info, d, [R.search(oracle, p, E.CAM, E.SCALE, E.W, E.H, 10.0, True, True, 0)], "after")


def test_octave_out_of_range(gpu, torch, oracle, matchers):
    """Found on the device, that problem alone: n_matches -1, kp_match all -1."""
    good = crowd(300, 200, 41)
    probs = []
    for octave in (E.N_LEVELS, -1, 1 << 20):
        q = dict(good)
        lk = good["last_keys"].copy()
        live = np.nonzero(good["last_point_index"] >= 0)[0]
        lk["octave"][live[5]] = octave
        q["last_keys"] = lk
        probs.append(q)
    ignored = dict(good)       # a NULL entry's octave is never read
    lk = good["last_keys"].copy()
    lk["octave"][np.nonzero(good["last_point_index"] < 0)[0]] = 99
    ignored["last_keys"] = lk
    probs = [good, probs[0], ignored, probs[1], probs[2], good]
    d = pack(torch, probs, 300, 200)
    launch(matchers[1], d, 10.0, True, 20)
    km, info = results(torch, d)
    ref = R.search(oracle, good, E.CAM, E.SCALE, E.W, E.H, 10.0, True, True, 20)
    assert ref[1]["n_matches"] > 20
    for p in (0, 2, 5):
        check(km[p:p + 1], info[p:p + 1], sub(d, p), [ref], ("good", p))
    for p in (1, 3, 4):
        assert (int(info[p]["n_matches"]), int(info[p]["n_matches_first_pass"]),
                int(info[p]["retried"])) == (-1, -1, 0)
        assert (km[p, :300] == -1).all()


def sub(d, p):
    s = Packed()
    s.nk = d.nk[p:p + 1]
    return s


# --------------------------------------------------------------- stream order
def test_two_streams_no_synchronisation(gpu, torch, oracle, matchers):
    """Two calls on two streams, nothing between them, the sizes changing: the
    second reuses the handle's grid scratch (CallOrder)."""
    m = gpu.ORBmatcher(0.9, True)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    grid = size_grid()
    big = [grid[35 - (i % 12)] for i in range(96)]
    small = [crowd(300, 200, 41 + i) for i in range(4)]
    d1, d2 = pack(torch, big, 1000, 257), pack(torch, small, 300, 200)
    torch.cuda.synchronize()
    launch(m, d1, 10.0, True, 20, stream=s1.cuda_stream)
    launch(m, d2, 10.0, True, 20, stream=s2.cuda_stream)
    launch(m, d1, 10.0, True, 0, stream=s1.cuda_stream)
    km2, info2 = results(torch, d2)
    km1, info1 = results(torch, d1)
    cache = {}
    for p in big:
        cache.setdefault(id(p), R.search(oracle, p, E.CAM, E.SCALE, E.W, E.H, 10.0, True, True, 0))
    check(km1, info1, d1, [cache[id(p)] for p in big], "stream 1")
    check(km2, info2, d2, [R.search(oracle, p, E.CAM, E.SCALE, E.W, E.H, 10.0, True, True, 20)
                           for p in small], "stream 2")


# ------------------------------------------------------------ discard and mark
def discard_case(rng, n, n_pts):
    km = np.where(rng.random(n) < 0.6, rng.integers(0, n_pts, n), -1).astype(np.int32)
    km[rng.random(n) < 0.05] = -2
    ol = (rng.random(n) < 0.3).astype(np.uint8)
    pts = np.zeros(n_pts, R.MAP_POINT_DTYPE)
    pts["has_obs"] = rng.random(n_pts) < 0.7
    pts["bad"] = rng.random(n_pts) < 0.1
    pts["seen"] = rng.random(n_pts) < 0.05
    pts["pos"] = rng.normal(size=(n_pts, 3))
    return km, ol, pts


@pytest.mark.parametrize("mark", [0, 1])
def test_discard_and_mark(gpu, torch, matchers, mark):
    rng = np.random.default_rng(5)
    hand_pts = np.zeros(6, R.MAP_POINT_DTYPE)
    hand_pts["has_obs"], hand_pts["bad"] = [1, 0, 1, 1, 1, 1], [0, 0, 0, 1, 0, 0]
    cases = [(np.array([-1, -2, 0, 2, 1, 3, -1], np.int32),
              np.array([0, 0, 1, 0, 0, 0, 1], np.uint8), hand_pts)]
    cases += [discard_case(rng, n, 500) for n in (0, 1, 63, 64, 65, 257, 1000)]
    P, stride, mps = len(cases), 1000, 500
    km = np.full((P, stride), JUNK, np.int32)
    ol = np.full((P, stride), 1, np.uint8)
    pts = np.zeros((P, mps), R.MAP_POINT_DTYPE)
    nk = np.zeros(P, np.int32)
    info = np.zeros(P, R.INFO_DTYPE)
    for p, (k, o, pt) in enumerate(cases):
        n = len(k)
        km[p, :n], ol[p, :n], pts[p, :len(pt)], nk[p] = k, o, pt, n
        info[p]["n_matches"] = 400 + p
    d_km, d_ol, d_pts = _dev(torch, km).view(torch.int32), _dev(torch, ol), _dev(torch, pts)
    d_nk, d_info = _dev(torch, nk), _dev(torch, info)
    d_out = torch.full((P * 3,), JUNK, dtype=torch.int32, device="cuda")
    matchers[1].track_discard_outliers_batch(P, d_nk.data_ptr(), stride, d_km.data_ptr(),
                                             d_ol.data_ptr(), d_pts.data_ptr(), mps, mark,
                                             d_info.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    g_km = d_km.cpu().numpy().reshape(P, stride)
    g_ol = d_ol.cpu().numpy().reshape(P, stride)
    g_pts = d_pts.cpu().numpy().view(R.MAP_POINT_DTYPE).reshape(P, mps)
    g_out = d_out.cpu().numpy().view(R.DISCARD_DTYPE).reshape(P)
    for p, (k, o, pt) in enumerate(cases):
        n = len(k)
        rk, ro, rp, rout = R.discard_outliers(k, o, pt, 400 + p, mark)
        assert np.array_equal(g_km[p, :n], rk) and np.array_equal(g_ol[p, :n], ro), p
        assert (g_km[p, n:] == JUNK).all() and (g_ol[p, n:] == 1).all(), p
        assert g_pts[p, :len(pt)].tobytes() == rp.tobytes(), p
        assert g_out[p].tolist() == rout.tolist(), (p, g_out[p], rout)
    assert g_out[0].tolist() == (400 - 1, 2, 1)
    with pytest.raises(gpu.OrbError) as err:   # marking needs the problem's own records
        matchers[1].track_discard_outliers_batch(P, d_nk.data_ptr(), stride, d_km.data_ptr(),
                                                 d_ol.data_ptr(), d_pts.data_ptr(), 0, 1,
                                                 d_info.data_ptr(), d_out.data_ptr())
    assert err.value.status == gpu.ORB_EINVAL


# --------------------------------------------------------------------- chain
def test_tracking_chain_device_resident(gpu, torch, oracle):
    """Four problems, every intermediate in device memory: extract two
    consecutive frames -> (the last frame's matches against a synthetic map,
    set up on the host) -> motion-model match -> PoseOptimization on its
    d_kp_match -> discard and mark -> isInFrustum at the optimised pose ->
    SearchByProjection(F, localMap); each stage against its CPU reference on
    the same inputs."""
    import poseopt_cases as pc
    W, H, F, M, NF = 1241, 376, 4, 3000, 1000
    cam = S.camera()
    scale = oracle.params(NF)["scale"]
    levels = (f32(1.0) / (scale * scale)).astype(f32)
    LS = f32(E.LS)
    imgs = np.stack([oracle.synth_image(80 + f, fr, W, H) for fr in (0, 1) for f in range(F)])
    q = []
    for f in range(F):
        rng = np.random.default_rng(80 + f)
        ka, da, _ = oracle.extract(imgs[f], NF)
        kb, db, _ = oracle.extract(imgs[F + f], NF)
        pose, P, mpd = S.local_map_3d(oracle, kb, db, M, W, H, rng_seed=80 + f)
        P["seen"] = 0
        _, tr0 = oracle.frustum(P, pose, cam, W, H, 0.5, LS, 8)
        # the last frame holds the map point that projects nearest to where its
        # keypoint moved (the sequence's ego shift), on about 80 % of its keypoints
        px = np.where(tr0["in_view"] != 0, tr0["proj_x"], 1e9)
        d2 = ((ka["x"][:, None] + S._ego_shift(80 + f) - px[None, :]) ** 2
              + (ka["y"][:, None] - tr0["proj_y"][None, :]) ** 2)
        near = d2.argmin(1)
        lidx = np.where((d2[np.arange(len(ka)), near] < 16.0) & (rng.random(len(ka)) < 0.9),
                        near, -1).astype(np.int32)
        last_pose = R.pose(pose["rcw"][0].reshape(3, 3), pose["tcw"][0] + np.array([0, 0, 0.3], f32))
        prob = dict(keys=kb, desc=db, u_right=None, locked=None, pose_cur=pose, pose_last=last_pose,
                    last_keys=ka, last_point_index=lidx, last_outlier=None, points=P, mp_desc=mpd)
        km3, info3 = R.search(oracle, prob, cam, scale, W, H, 15.0, True, True, 20)
        ur = np.full(len(kb), -1, f32)
        r4 = pc.ref.pose_optimization(np.stack([kb["x"], kb["y"]], 1), kb["octave"], ur, km3,
                                      P["pos"], levels, cam, pose["rcw"][0], pose["tcw"][0],
                                      pose["ow"][0], np.full(len(kb), pc.SENTINEL, np.uint8))
        km5, ol5, P5, out5 = R.discard_outliers(km3, r4["outlier"], P, info3["n_matches"], True)
        pose2 = np.zeros(1, gpu.POSE_DTYPE)
        pose2["rcw"], pose2["tcw"], pose2["ow"] = r4["rcw"], r4["tcw"], r4["ow"]
        n6, tr6 = oracle.frustum(P5, pose2, cam, W, H, 0.5, LS, 8)
        locked = ((km5 >= 0) & (P5["has_obs"][np.maximum(km5, 0)] != 0)).astype(np.uint8)
        nm7, km7 = oracle.match_projection_local(kb, db, scale, W, H, tr6, mpd, 3.0, 0.8, locked)
        assert (lidx >= 0).sum() > 300 and info3["n_matches"] > 100 and r4["n_inliers"] > 50
        assert out5["n_discarded"] > 0 and P5["seen"].sum() > 100 and nm7 > 50
        assert not (tr6["in_view"][P5["seen"] != 0]).any()
        q.append(dict(ka=ka, da=da, kb=kb, db=db, pose=pose, last_pose=last_pose, P=P, mpd=mpd,
                      lidx=lidx, km3=km3, info3=info3, r4=r4, km5=km5, ol5=ol5, P5=P5, out5=out5,
                      n6=n6, tr6=tr6, locked=locked, nm7=nm7, km7=km7))
    ext = gpu.ORBextractor(NF, 1.2, 8, 20, 7)
    cap = ext.capacity(W, H)
    assert cap <= gpu.ORBmatcher.search_by_projection_frame_batch_max_stride()
    lidx = np.full((F, cap), -1, np.int32)
    Pall = np.zeros((F, M), gpu.MAP_POINT_DTYPE)
    md = np.zeros((F, M, 32), np.uint8)
    pcur, plast = np.zeros(F, gpu.POSE_DTYPE), np.zeros(F, gpu.POSE_DTYPE)
    for f, c in enumerate(q):
        lidx[f, :len(c["lidx"])] = c["lidx"]
        Pall[f], md[f], pcur[f], plast[f] = c["P"], c["mpd"], c["pose"][0], c["last_pose"][0]
    d_img = torch.from_numpy(imgs).cuda()
    d_kps = torch.zeros((2 * F, cap, 7), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((2 * F, cap, 32), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(2 * F, dtype=torch.int32, device="cuda")
    d_lidx, d_P, d_md, d_pcur, d_plast = (_dev(torch, a) for a in (lidx, Pall, md, pcur, plast))
    d_ur = torch.full((F * cap,), -1.0, dtype=torch.float32, device="cuda")
    d_nm = torch.full((F,), M, dtype=torch.int32, device="cuda")
    d_km = torch.full((F, cap), JUNK, dtype=torch.int32, device="cuda")
    d_info3 = torch.zeros(F * 5, dtype=torch.int32, device="cuda")
    d_pout = torch.zeros(F * gpu.POSE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_outl = torch.full((F * cap,), pc.SENTINEL, dtype=torch.uint8, device="cuda")
    d_info4 = torch.zeros(F * 4, dtype=torch.int32, device="cuda")
    d_out5 = torch.zeros(F * 3, dtype=torch.int32, device="cuda")
    tsz = gpu.MP_TRACK_DTYPE.itemsize
    d_tr = torch.zeros(F * M * tsz, dtype=torch.uint8, device="cuda")
    d_cnt6 = torch.zeros(F, dtype=torch.int32, device="cuda")
    d_km7 = torch.full((F * cap,), JUNK, dtype=torch.int32, device="cuda")
    d_nm7 = torch.zeros(F, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # the current frames are images F..2F-1 of the extraction batch
    k_cur = d_kps.data_ptr() + F * cap * 28
    dsc_cur = d_desc.data_ptr() + F * cap * 32
    n_cur = d_cnt.data_ptr() + F * 4
    m = gpu.ORBmatcher(0.8, True)
    ext.extract_batch(d_img.data_ptr(), 2 * F, W, H, W, W * H, d_kps.data_ptr(),
                      d_desc.data_ptr(), cap, d_cnt.data_ptr())
    torch.cuda.synchronize()   # the extractor runs on its own stream
    # one stream for the library's calls and torch's gather between them
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        m.search_by_projection_frame_batch(
            F, k_cur, dsc_cur, 0, 0, n_cur, cap, d_pcur.data_ptr(), d_plast.data_ptr(),
            d_kps.data_ptr(), d_cnt.data_ptr(), d_lidx.data_ptr(), 0, d_P.data_ptr(), d_md.data_ptr(),
            M, cam, 0.0, float(W), 0.0, float(H), scale, 15.0, True, 20, d_km.data_ptr(),
            d_info3.data_ptr(), stream=st.cuda_stream)
        km3 = d_km.clone()
        m.pose_optimization_batch(F, n_cur, k_cur, d_ur.data_ptr(), cap, d_km.data_ptr(),
                                  d_P.data_ptr(), gpu.MAP_POINT_DTYPE.itemsize, M, levels, cam,
                                  d_pcur.data_ptr(), d_pout.data_ptr(), d_outl.data_ptr(),
                                  d_info4.data_ptr(), stream=st.cuda_stream)
        m.track_discard_outliers_batch(F, n_cur, cap, d_km.data_ptr(), d_outl.data_ptr(),
                                       d_P.data_ptr(), M, True, d_info3.data_ptr(), d_out5.data_ptr(),
                                       stream=st.cuda_stream)
        m.frustum_batch(F, d_P.data_ptr(), d_nm.data_ptr(), M, d_pout.data_ptr(), cam, 0.0, float(W),
                        0.0, float(H), 0.5, LS, 8, d_tr.data_ptr(), d_cnt6.data_ptr(),
                        stream=st.cuda_stream)
        # the keypoints the local-map search may not take: matched to a point with
        # observations (one gather; merging the match arrays is the caller's)
        has_obs = d_P.view(F, M, gpu.MAP_POINT_DTYPE.itemsize)[:, :, 34]
        locked = ((d_km >= 0) & (torch.gather(has_obs, 1, d_km.clamp(0, M - 1).long()) != 0))
        d_locked = locked.to(torch.uint8).contiguous()
        m.search_by_projection_batch(F, k_cur, dsc_cur, n_cur, d_locked.data_ptr(), cap,
                                     d_tr.data_ptr(), d_md.data_ptr(), d_nm.data_ptr(), M, W, H, scale,
                                     3.0, d_km7.data_ptr(), d_nm7.data_ptr(), stream=st.cuda_stream)
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy()
    kps = d_kps.cpu().numpy().view(gpu.KEYPOINT_DTYPE).reshape(2 * F, cap)
    desc = d_desc.cpu().numpy()
    h_km3 = km3.cpu().numpy()
    info3 = d_info3.cpu().numpy().view(R.INFO_DTYPE)
    h_km5 = d_km.cpu().numpy()
    outl = d_outl.cpu().numpy().reshape(F, cap)
    pout = d_pout.cpu().numpy().view(gpu.POSE_DTYPE)
    info4 = d_info4.cpu().numpy().view(gpu.POSE_OPT_INFO_DTYPE)
    out5 = d_out5.cpu().numpy().view(R.DISCARD_DTYPE)
    P5 = d_P.cpu().numpy().view(gpu.MAP_POINT_DTYPE).reshape(F, M)
    tr6 = d_tr.cpu().numpy().view(gpu.MP_TRACK_DTYPE).reshape(F, M)
    km7 = d_km7.cpu().numpy().reshape(F, cap)
    for f, c in enumerate(q):
        n = len(c["kb"])
        # 1. extraction
        assert cnt[f] == len(c["ka"]) and cnt[F + f] == n, f
        assert kps[f, :cnt[f]].tobytes() == c["ka"].tobytes(), f
        assert kps[F + f, :n].tobytes() == c["kb"].tobytes(), f
        assert desc[F + f, :n].tobytes() == c["db"].tobytes(), f
        # 3. motion-model match
        assert np.array_equal(h_km3[f, :n], c["km3"]) and (h_km3[f, n:] == JUNK).all(), f
        assert info3[f].tolist() == c["info3"].tolist(), (f, info3[f], c["info3"])
        # 4. PoseOptimization on d_kp_match
        r4 = c["r4"]
        got = tuple(int(info4[f][k]) for k in ("n_inliers", "n_edges", "lm_iterations",
                                               "rejected_trials"))
        assert got == (r4["n_inliers"], r4["n_edges"], r4["lm_iterations"], r4["rejected_trials"]), f
        for k in ("rcw", "tcw", "ow"):
            assert pout[f][k].tobytes() == np.asarray(r4[k], f32).tobytes(), (f, k)
        # 5. discard and mark
        assert np.array_equal(h_km5[f, :n], c["km5"]) and (h_km5[f, n:] == JUNK).all(), f
        assert np.array_equal(outl[f, :n], c["ol5"]) and (outl[f, n:] == pc.SENTINEL).all(), f
        assert out5[f].tolist() == c["out5"].tolist(), (f, out5[f], c["out5"])
        assert P5[f].tobytes() == c["P5"].tobytes(), f
        # 6. isInFrustum at the optimised pose skips what was marked
        assert int(d_cnt6[f].item()) == c["n6"] and tr6[f].tobytes() == c["tr6"].tobytes(), f
        # 7. SearchByProjection(F, localMap)
        assert np.array_equal(d_locked[f, :n].cpu().numpy(), c["locked"]), f
        assert int(d_nm7[f].item()) == c["nm7"] and np.array_equal(km7[f, :n], c["km7"]), f
