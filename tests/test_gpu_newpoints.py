"""LocalMapping::CreateNewMapPoints as a device batch
(orb_scene_median_depth_batch / orb_create_new_map_points_batch, k_median_depth /
k_new_points) against tests/newpoints_ref.py: status, x3D, the new map point
records byte for byte, the pairs, both point_index rows, the cursor and info;
slots past each count and points past the cursor untouched (junk prefill).
Float fields are compared by bit pattern, except that any NaN equals any NaN."""
import numpy as np
import pytest

import newpoints_cases as C
import newpoints_ref as R

pytestmark = pytest.mark.gpu
STRIDE = 384  # above one workgroup (256) and the largest natural keyframe (350)
J_STATUS, J_X3D, J_PAIR, J_PIDX = 0xEE, np.float32(-7.25), -77, -9  # as Case.run prefills


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def matcher(gpu):
    return gpu.ORBmatcher(0.6, False)


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def same_f(a, b, what):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    ok = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    assert ok.all(), (what, a[~ok][:4], b[~ok][:4], np.argwhere(~ok)[:4])


def same_rec(a, b, what):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.shape, b.shape)
    for name in a.dtype.names:
        if a[name].dtype.kind == "f":
            same_f(a[name], b[name], f"{what}.{name}")
        else:
            assert (a[name] == b[name]).all(), (what, name, a[name], b[name])


def check_case(c, status, x3d, pairs, points, pidx1, pidx2, cursor, info, base, what):
    """One problem's outputs (rows of `stride` slots, the problem's window of
    points, indices shifted by `base`) against the restatement."""
    ref = c.ref()
    n1, n2 = len(c.kf1["keys"]), len(c.kf2["keys"])
    assert (status[:n1] == ref["status"]).all(), (what, "status", status[:n1], ref["status"])
    assert (status[n1:] == J_STATUS).all(), (what, "status past the count")
    same_f(x3d[:n1], ref["x3d"], f"{what} x3d")
    same_f(x3d[n1:], np.full_like(x3d[n1:], J_X3D), f"{what} x3d past the count")
    assert (pairs[:n1] == ref["pairs"]).all(), (what, "pairs")
    assert (pairs[n1:] == J_PAIR).all(), (what, "pairs past the count")
    same_rec(points, ref["points"], f"{what} points")  # junk past the cursor included
    unshift = lambda a: np.where(a >= 0, a - base, a)
    assert (unshift(pidx1[:n1]) == ref["pidx1"]).all(), (what, "point_index of KF1")
    assert (unshift(pidx2[:n2]) == ref["pidx2"]).all(), (what, "point_index of KF2")
    assert (pidx1[n1:] == J_PIDX).all() and (pidx2[n2:] == J_PIDX).all(), (what, "index rows")
    inf = info.copy()
    if not inf["overflow"]:
        inf["first_point"] -= base
    same_rec(inf, ref["info"], f"{what} info")
    assert cursor - base == ref["cursor"], (what, "cursor", cursor - base, ref["cursor"])


def run_group(torch, matcher, cases, stride=STRIDE, capacity=None, stream=0):
    b = C.pack(cases, stride)
    n = len(cases)
    mono_kf = all(c.kf1["u_right"] is None for c in cases)
    d = {k: _dev(torch, b[k]) for k in ("keys", "u_right", "depth", "point_index", "pose",
                                         "nkeys", "match12", "kf1_slot", "kf2_slot", "median",
                                         "points", "cursor", "cursor_index")}
    status = torch.full((n * stride,), J_STATUS, dtype=torch.uint8, device="cuda")
    x3d = torch.full((n * stride * 3,), float(J_X3D), dtype=torch.float32, device="cuda")
    pairs = torch.full((n * stride * 2,), J_PAIR, dtype=torch.int32, device="cuda")
    info = torch.full((n * 64,), 0x5A, dtype=torch.uint8, device="cuda")
    c0 = cases[0]
    matcher.create_new_map_points_batch(
        n, d["kf1_slot"].data_ptr(), d["kf2_slot"].data_ptr(), d["keys"].data_ptr(),
        d["nkeys"].data_ptr(), d["point_index"].data_ptr(), d["pose"].data_ptr(),
        0 if mono_kf else d["u_right"].data_ptr(), 0 if mono_kf else d["depth"].data_ptr(), stride,
        d["match12"].data_ptr(), d["median"].data_ptr(), c0.cam1, c0.cam2, C.SCALE_FACTORS,
        C.LEVEL_SIGMA2, c0.monocular, d["points"].data_ptr(),
        int(b["base"][-1]) if capacity is None else capacity, d["cursor"].data_ptr(),
        d["cursor_index"].data_ptr(), status.data_ptr(), x3d.data_ptr(), pairs.data_ptr(),
        info.data_ptr(), stream)
    torch.cuda.synchronize()
    st = status.cpu().numpy().reshape(n, stride)
    xs = x3d.cpu().numpy().reshape(n, stride, 3)
    pr = pairs.cpu().numpy().reshape(n, stride, 2)
    inf = _host(info, R.NEW_POINT_INFO_DTYPE)
    pts = _host(d["points"], R.MAP_POINT_DTYPE)
    pidx = _host(d["point_index"], np.int32).reshape(2 * n, stride)
    cur = _host(d["cursor"], np.int32)
    for p, c in enumerate(cases):
        lo, hi = int(b["base"][p]), int(b["base"][p + 1])
        check_case(c, st[p], xs[p], pr[p], pts[lo:hi], pidx[2 * p], pidx[2 * p + 1], int(cur[p]),
                   inf[p], lo, c.name)


def test_every_case_through_the_batch_call(torch, matcher):
    """Every case, grouped by the host values one call shares; a group is many
    independent problems in one call."""
    normal = [c for c in C.all_cases() if not c.tags & {"cap_exact", "cap_over"}]
    groups = C.groups(normal)
    assert any(len(g) >= 2 for g in groups)
    for g in groups:
        run_group(torch, matcher, g)


def test_cursor_at_and_past_the_capacity(torch, matcher):
    for c in C.all_cases():
        if c.tags & {"cap_exact", "cap_over"}:
            assert bool(c.ref()["info"]["overflow"]) == ("cap_over" in c.tags)
            run_group(torch, matcher, [c], capacity=c.capacity)


def test_every_case_through_the_one_problem_call(matcher):
    for c in C.all_cases():
        n1 = len(c.kf1["keys"])
        kf1 = dict(c.kf1, point_index=c.kf1["point_index"].copy())
        kf2 = dict(c.kf2, point_index=c.kf2["point_index"].copy())
        points = C.junk_points(c.capacity)
        if c.points is not None:
            points[:len(c.points)] = c.points
        status = np.full(n1, J_STATUS, np.uint8)
        x3d = np.full((n1, 3), J_X3D, np.float32)
        pairs = np.full((n1, 2), J_PAIR, np.int32)
        info, cur, *_ = matcher.CreateNewMapPoints(
            kf1, kf2, c.match12, c.cam1, c.cam2, C.SCALE_FACTORS, C.LEVEL_SIGMA2, c.monocular,
            points, c.cursor, c.median, status, x3d, pairs)
        ref = c.ref()
        what = f"{c.name} (one problem)"
        assert (status == ref["status"]).all(), (what, status, ref["status"])
        same_f(x3d, ref["x3d"], what)
        assert (pairs == ref["pairs"]).all(), what
        same_rec(points, ref["points"], what)
        assert (kf1["point_index"] == ref["pidx1"]).all(), what
        assert (kf2["point_index"] == ref["pidx2"]).all(), what
        same_rec(info, ref["info"], what)
        assert cur == ref["cursor"], what


def test_three_neighbour_chain_on_one_stream(torch, matcher):
    """The neighbours of one keyframe in successive calls on one stream, the
    median batch ahead of them, no host copy in between: equal to the restated
    loop.  The matcher is replaced by fixed match12 rows; neighbour k takes the
    keypoints with i1 % 3 == k, which respects the masks the earlier calls update."""
    baselines = ((0.9, 0.05, 0.1), (-0.7, 0.1, 0.2), (0.2, -0.6, 0.3))
    cs = [C.natural_case(f"chain{k}", 31, 150, True, baseline=bl) for k, bl in enumerate(baselines)]
    kf1 = cs[0].kf1
    for c in cs[1:]:
        assert c.kf1["keys"].tobytes() == kf1["keys"].tobytes()
        assert (c.kf1["pose"] == kf1["pose"]) and (c.points == cs[0].points).all()
    n1, S = len(kf1["keys"]), STRIDE
    i1 = np.arange(n1)
    m12 = [np.where(i1 % 3 == k, c.match12, -1).astype(np.int32) for k, c in enumerate(cs)]
    n_exist, cap = cs[0].cursor, cs[0].cursor + n1
    # the restated loop
    points = C.junk_points(cap)
    points[:n_exist] = cs[0].points
    r_kf1 = dict(kf1, point_index=kf1["point_index"].copy())
    r_kf2 = [dict(c.kf2, point_index=c.kf2["point_index"].copy()) for c in cs]
    r_status = np.full((3, n1), J_STATUS, np.uint8)
    r_x3d = np.full((3, n1, 3), J_X3D, np.float32)
    r_pairs = np.full((3, n1, 2), J_PAIR, np.int32)
    cursor, r_info, r_med = n_exist, [], []
    for k in range(3):
        med, _ = R.scene_median_depth(r_kf2[k]["point_index"], r_kf2[k]["pose"], points["pos"], 2)
        r_med.append(med)
        info, cursor = R.create_new_map_points(
            r_kf1, r_kf2[k], m12[k], med, C.CAM_N, C.CAM_N, C.SCALE_FACTORS, C.LEVEL_SIGMA2, True,
            points, cursor, r_status[k], r_x3d[k], r_pairs[k])
        r_info.append(info)
    assert sum(int(i["n_new"]) for i in r_info) > 60 and all(int(i["n_new"]) > 5 for i in r_info)
    # the device: slot 0 = the current keyframe, slots 1..3 = the neighbours
    keys = np.zeros((4, S), R.KEYPOINT_DTYPE)
    pidx = np.full((4, S), J_PIDX, np.int32)
    pose = np.zeros(4, R.POSE_DTYPE)
    nkeys = np.zeros(4, np.int32)
    for s, kf in enumerate([kf1] + [c.kf2 for c in cs]):
        k = len(kf["keys"])
        keys[s, :k], pidx[s, :k], pose[s], nkeys[s] = kf["keys"], kf["point_index"], kf["pose"], k
    mrows = np.full((3, S), 5, np.int32)
    for k in range(3):
        mrows[k, :n1] = m12[k]
    pts = C.junk_points(cap)
    pts[:n_exist] = cs[0].points
    d = {k: _dev(torch, v) for k, v in dict(
        keys=keys, pidx=pidx, pose=pose, nkeys=nkeys, m12=mrows, points=pts,
        slots=np.arange(4, dtype=np.int32), cursor=np.array([n_exist], np.int32),
        cidx=np.zeros(1, np.int32)).items()}
    med = torch.full((4,), -1.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    status = torch.full((3 * S,), J_STATUS, dtype=torch.uint8, device="cuda")
    x3d = torch.full((3 * S * 3,), float(J_X3D), dtype=torch.float32, device="cuda")
    pairs = torch.full((3 * S * 2,), J_PAIR, dtype=torch.int32, device="cuda")
    info = torch.zeros(3 * 64, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    sp = stream.cuda_stream
    for k in range(3):
        # the neighbour's median over the map as the earlier calls left it
        matcher.scene_median_depth_batch(
            1, d["slots"].data_ptr() + 4 * (k + 1), d["nkeys"].data_ptr(), d["pidx"].data_ptr(),
            d["pose"].data_ptr(), S, d["points"].data_ptr(), med.data_ptr() + 4 * (k + 1),
            cnt.data_ptr() + 4 * (k + 1), 2, sp)
        matcher.create_new_map_points_batch(
            1, d["slots"].data_ptr(), d["slots"].data_ptr() + 4 * (k + 1), d["keys"].data_ptr(),
            d["nkeys"].data_ptr(), d["pidx"].data_ptr(), d["pose"].data_ptr(), 0, 0, S,
            d["m12"].data_ptr() + 4 * S * k, med.data_ptr() + 4 * (k + 1), C.CAM_N, C.CAM_N,
            C.SCALE_FACTORS, C.LEVEL_SIGMA2, True, d["points"].data_ptr(), cap,
            d["cursor"].data_ptr(), d["cidx"].data_ptr(), status.data_ptr() + S * k,
            x3d.data_ptr() + 12 * S * k, pairs.data_ptr() + 8 * S * k, info.data_ptr() + 64 * k, sp)
    stream.synchronize()
    same_f(med.cpu().numpy()[1:], np.array(r_med, np.float32), "chain medians")
    st = status.cpu().numpy().reshape(3, S)
    assert (st[:, :n1] == r_status).all() and (st[:, n1:] == J_STATUS).all()
    same_f(x3d.cpu().numpy().reshape(3, S, 3)[:, :n1], r_x3d, "chain x3d")
    assert (pairs.cpu().numpy().reshape(3, S, 2)[:, :n1] == r_pairs).all()
    same_rec(_host(d["points"], R.MAP_POINT_DTYPE), points, "chain points")
    got = _host(d["pidx"], np.int32).reshape(4, S)
    assert (got[0, :n1] == r_kf1["point_index"]).all()
    for k in range(3):
        n2 = len(r_kf2[k]["point_index"])
        assert (got[k + 1, :n2] == r_kf2[k]["point_index"]).all(), k
        assert (got[k + 1, n2:] == J_PIDX).all()
    same_rec(_host(info, R.NEW_POINT_INFO_DTYPE), np.array(r_info), "chain info")
    assert int(_host(d["cursor"], np.int32)[0]) == cursor


def test_median_batch_and_one_problem_form(torch, matcher):
    mc = C.median_cases()
    n = len(mc)
    S = max(len(c[1]) for c in mc) + 2
    pos = mc[0][3]
    points = np.zeros(len(pos), R.MAP_POINT_DTYPE)
    points["pos"] = pos
    pidx = np.full((n, S), 3, np.int32)  # junk past the count: a valid index
    pose = np.zeros(n, R.POSE_DTYPE)
    nkeys = np.zeros(n, np.int32)
    for p, (_, idx, ps, _, _) in enumerate(mc):
        pidx[p, :len(idx)], pose[p], nkeys[p] = idx, ps, len(idx)
    for q in sorted({c[4] for c in mc}):
        d = [_dev(torch, a) for a in (nkeys, pidx, pose, points)]
        med = torch.full((n,), -5.0, dtype=torch.float32, device="cuda")
        cnt = torch.full((n,), -5, dtype=torch.int32, device="cuda")
        matcher.scene_median_depth_batch(n, 0, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                         S, d[3].data_ptr(), med.data_ptr(), cnt.data_ptr(), q)
        torch.cuda.synchronize()
        med, cnt = med.cpu().numpy(), cnt.cpu().numpy()
        for p, (name, idx, ps, pp, cq) in enumerate(mc):
            if cq != q:
                continue
            r_med, r_cnt = R.scene_median_depth(idx, ps, pp, q)
            same_f(med[p], r_med, name)
            assert cnt[p] == r_cnt, name
            h_med, h_cnt = matcher.ComputeSceneMedianDepth(idx, ps, points, q)
            same_f(h_med, r_med, f"{name} (one problem)")
            assert h_cnt == r_cnt, name
    # the natural monocular cases' medians (what their gate reads)
    for c in C.natural_cases():
        if c.monocular:
            h_med, _ = matcher.ComputeSceneMedianDepth(c.kf2["point_index"], c.kf2["pose"],
                                                       c.points, 2)
            same_f(h_med, c.median, c.name)
