"""GPU parity of Optimizer::PoseOptimization (pose_kernels.hip) against the
numpy restatement tests/poseopt_ref.py: every output bit for bit -- the pose
floats, the outlier flags, the untouched sentinel slots and all four info
fields -- for one frame, both storage tiers, batches, degenerate inputs, the
device-resident chain and two streams on one handle."""
import functools
import math

import numpy as np
import pytest

import poseopt_cases as pc
import scenarios

pytestmark = pytest.mark.gpu
f32 = np.float32


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _host(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def _same_floats(a, b):
    """Bitwise equal, NaN positions comparing equal to NaN."""
    a, b = np.asarray(a, f32).reshape(-1), np.asarray(b, f32).reshape(-1)
    nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | nan).all())


def _assert_result(pose, outlier, info, r, tag):
    got = tuple(int(info[k]) for k in ("n_inliers", "n_edges", "lm_iterations", "rejected_trials"))
    want = (r["n_inliers"], r["n_edges"], r["lm_iterations"], r["rejected_trials"])
    assert got == want, (tag, got, want)
    assert np.array_equal(outlier, r["outlier"]), (tag, np.nonzero(outlier != r["outlier"])[0][:8])
    for k in ("rcw", "tcw", "ow"):
        assert _same_floats(pose[k], r[k]), (tag, k, pose[k], r[k])


@functools.lru_cache(maxsize=None)
def _case(seed, n_kp, n_edges, kind, noise=1.0):
    c = pc.make_case(seed, n_kp, n_edges, kind, noise)
    return c, pc.run_ref(c)


def _one_frame(gpu, c):
    return gpu.ORBmatcher().PoseOptimization(
        c["keys"], c["u_right"], c["point_index"], c["points"], c.get("levels", pc.INV_LEVEL_SIGMA2),
        c.get("cam", pc.CAM), c["pose"], c["outlier"])


# ------------------------------------------------------------------- one frame
@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
@pytest.mark.parametrize("n_edges", [0, 2, 3, 9, 10, 63, 64, 65, 129, 800])
def test_one_frame(gpu, n_edges, kind):
    c, r = _case(3000 + n_edges, 1000, n_edges, kind)
    n, pose, outlier, info = _one_frame(gpu, c)
    _assert_result(pose, outlier, info, r, (n_edges, kind))
    assert n == r["n_inliers"]
    no_edge = c["point_index"] < 0
    assert (outlier[no_edge] == pc.SENTINEL).all() and no_edge.sum() == 1000 - n_edges
    if n_edges >= 3:
        assert r["trace"]["lm_iterations"] > 0 and (outlier[~no_edge] <= 1).all()
        assert r["trace"]["rounds"] == (4 if n_edges >= 10 else 1)
    else:
        assert n == 0 and pose.tobytes() == c["pose"][0].tobytes()


@pytest.mark.parametrize("above", [0, 1])
def test_storage_tiers(gpu, above):
    """A frame whose edge records just fit LDS and one a slot above it, which
    runs from the handle's device scratch; every slot carries an edge."""
    n = gpu.ORBmatcher.pose_optimization_lds_edges() + above
    c, r = _case(4000 + above, n, n, "mixed")
    _, pose, outlier, info = _one_frame(gpu, c)
    assert r["n_edges"] == n
    _assert_result(pose, outlier, info, r, n)


# --------------------------------------------------------------------- batches
_BATCH_EDGES = (40, 0, 2, 64, 3, 9, 200, 10, 65, 1, 129, 100, 63, 0, 150, 30)


@functools.lru_cache(maxsize=None)
def _batch_case(i):
    e = _BATCH_EDGES[i % len(_BATCH_EDGES)]
    return _case(5000 + i, e + 5 + i % 7, e, ("mixed", "mono", "stereo")[i % 3], float(i % 2))


def _pack_batch(gpu, torch, cases, kp_stride, layout, share=False, levels=None, cam=None):
    """Packs the cases into one device batch; returns the call that runs it.  layout: "f3" packed
    float3 points, "mp" orb_map_point_t records.  share: one point array for
    all problems (pt_stride 0), the indices offset into it.  levels, cam: the
    level table and camera of the call when they are not pc.INV_LEVEL_SIGMA2
    and pc.CAM."""
    levels = pc.INV_LEVEL_SIGMA2 if levels is None else levels
    cam = pc.CAM if cam is None else cam
    P = len(cases)
    keys = np.zeros((P, kp_stride), gpu.KEYPOINT_DTYPE)
    ur = np.full((P, kp_stride), 55.0, f32)
    idx = np.full((P, kp_stride), 7, np.int32)      # beyond the count: never read
    outl = np.full((P, kp_stride), pc.SENTINEL, np.uint8)
    poses = np.zeros(P, gpu.POSE_DTYPE)
    nk = np.zeros(P, np.int32)
    offs = np.cumsum([0] + [len(c["points"]) for c in cases])
    pt_stride = 0 if share else max(len(c["points"]) for c in cases)
    pts = np.zeros((offs[-1],) if share else (P, pt_stride), gpu.MAP_POINT_DTYPE)
    pts["normal"], pts["bad"] = 9.0, 1                # fields the optimisation must not read
    for i, c in enumerate(cases):
        n = len(c["keys"])
        nk[i] = n
        keys[i, :n], idx[i, :n], poses[i] = c["keys"], c["point_index"], c["pose"][0]
        ur[i, :n] = -1.0 if c["u_right"] is None else c["u_right"]
        if share:
            idx[i, :n][c["point_index"] >= 0] += offs[i]
            pts["pos"][offs[i]:offs[i + 1]] = c["points"]
        else:
            pts["pos"][i, :len(c["points"])] = c["points"]
    if layout == "f3":
        pbuf, stride_bytes = np.ascontiguousarray(pts["pos"]), 12
    else:
        pbuf, stride_bytes = pts, gpu.MAP_POINT_DTYPE.itemsize
    d_keys, d_ur, d_idx, d_outl, d_pin, d_nk, d_pts = (
        _dev(torch, a) for a in (keys, ur, idx, outl, poses, nk, pbuf))
    d_pout = torch.zeros(P * gpu.POSE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_info = torch.full((P * 4,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def launch(m, stream=0):
        m.pose_optimization_batch(P, d_nk.data_ptr(), d_keys.data_ptr(), d_ur.data_ptr(),
                                  kp_stride, d_idx.data_ptr(), d_pts.data_ptr(), stride_bytes,
                                  pt_stride, levels, cam, d_pin.data_ptr(),
                                  d_pout.data_ptr(), d_outl.data_ptr(), d_info.data_ptr(),
                                  stream=stream)
        return d_pout, d_outl, d_info
    return launch


def _check_batch(gpu, cases_refs, kp_stride, d_pout, d_outl, d_info):
    P = len(cases_refs)
    pout = _host(d_pout, gpu.POSE_DTYPE, (P,))
    outl = _host(d_outl, np.uint8, (P, kp_stride))
    info = _host(d_info, gpu.POSE_OPT_INFO_DTYPE, (P,))
    for i, (c, r) in enumerate(cases_refs):
        n = len(c["keys"])
        _assert_result(pout[i], outl[i, :n], info[i], r, i)
        assert (outl[i, n:] == pc.SENTINEL).all(), i   # slots past the count


@pytest.mark.parametrize("layout", ["f3", "mp"])
@pytest.mark.parametrize("P", [1, 16, 128])
def test_batch(gpu, P, layout):
    """Mixed edge counts, empty and < 3-edge problems in the middle of the
    batch, kp_stride greater than every count, both point layouts."""
    torch = pytest.importorskip("torch")
    cr = [_batch_case(i) for i in range(P)]
    kp_stride = 230
    assert max(len(c["keys"]) for c, _ in cr) < kp_stride
    if P >= 16:
        edges = [r["n_edges"] for _, r in cr]
        assert 0 in edges[1:-1] and 2 in edges[1:-1] and max(edges) == 200
    d_pout, d_outl, d_info = _pack_batch(gpu, torch, [c for c, _ in cr], kp_stride, layout)(
        gpu.ORBmatcher())
    torch.cuda.synchronize()
    _check_batch(gpu, cr, kp_stride, d_pout, d_outl, d_info)


def test_batch_shared_points(gpu):
    """Problems that index one point array (pt_stride 0)."""
    torch = pytest.importorskip("torch")
    cr = [_batch_case(i) for i in range(16)]
    d_pout, d_outl, d_info = _pack_batch(gpu, torch, [c for c, _ in cr], 230, "mp", share=True)(
        gpu.ORBmatcher())
    torch.cuda.synchronize()
    _check_batch(gpu, cr, 230, d_pout, d_outl, d_info)


def test_rejects_bad_arguments(gpu):
    c, _ = _case(3003, 1000, 3, "mixed")
    m = gpu.ORBmatcher()
    with pytest.raises(gpu.OrbError):       # 17 levels
        m.PoseOptimization(c["keys"], c["u_right"], c["point_index"], c["points"],
                           np.ones(17, f32), pc.CAM, c["pose"])
    pts = np.zeros(len(c["points"]), np.dtype([("pos", "<f4", 3), ("pad", "u1", 2)]))  # stride 14
    with pytest.raises(gpu.OrbError):
        m.PoseOptimization(c["keys"], c["u_right"], c["point_index"], pts, pc.INV_LEVEL_SIGMA2,
                           pc.CAM, c["pose"])


# ------------------------------------------------------------------ degenerate
def _behind_camera():
    c = pc.make_case(6001, 90, 70, "mixed")
    used = c["point_index"][c["point_index"] >= 0]
    c["points"][used[::2], 2] -= f32(60.0)   # half of the points far behind the camera
    return c


def _z_exactly_zero():
    # identity start pose, one point in the camera plane: 1 / z is infinite there
    c = pc.make_case(6002, 40, 30, "mixed", at_optimum=True)
    c["pose"]["rcw"][0] = np.eye(3, dtype=f32).reshape(9)
    c["pose"]["tcw"][0], c["pose"]["ow"][0] = 0, 0
    c["points"][c["point_index"][c["slots"][3]]] = [f32(1.5), f32(-0.5), f32(0.0)]
    return c


def _all_identical():
    c = pc.make_case(6003, 50, 40, "mixed")
    c["points"][:] = c["points"][0]
    return c


def _at_optimum():
    """The start pose is the optimum with every error exactly zero: points on
    the optical axis of the identity pose observed at (cx, cy).  b is zero, the
    step is zero, the trial repeats the chi2 and rho == 0 ends each round."""
    n = 24
    keys = np.zeros(n, gpu_keypoint_dtype())
    keys["x"], keys["y"], keys["size"], keys["class_id"] = pc.CAM[2], pc.CAM[3], 31.0, -1
    keys["octave"] = np.arange(n) % pc.N_LEVELS
    pts = np.zeros((n, 3), f32)
    pts[:, 2] = np.linspace(4, 40, n)
    pose = np.zeros(1, pc.POSE_DTYPE)
    pose["rcw"] = np.eye(3, dtype=f32).reshape(1, 9)
    idx = np.arange(n, dtype=np.int32)
    idx[::5] = -1
    return dict(keys=keys, u_right=None, point_index=idx, points=pts, pose=pose,
                outlier=np.full(n, pc.SENTINEL, np.uint8))


def gpu_keypoint_dtype():
    from rgbd_cases import KEYPOINT_DTYPE
    return KEYPOINT_DTYPE


def _bad_octave():
    c = pc.make_case(6005, 60, 48, "mixed")
    c["keys"]["octave"][c["slots"][5]] = pc.N_LEVELS       # an edge: out of range
    c["keys"]["octave"][np.nonzero(c["point_index"] < 0)[0][0]] = -3   # no edge: never read
    return c


_DEGENERATE = {"behind_camera": _behind_camera, "z_exactly_zero": _z_exactly_zero,
               "all_identical": _all_identical, "at_optimum": _at_optimum,
               "bad_octave": _bad_octave}


@pytest.mark.parametrize("name", list(_DEGENERATE))
def test_degenerate(gpu, name):
    """Inputs where an unbounded loop or a mis-ordered NaN compare would show."""
    c = _DEGENERATE[name]()
    r = pc.run_ref(c)
    _, pose, outlier, info = _one_frame(gpu, c)
    _assert_result(pose, outlier, info, r, name)
    if name == "bad_octave":
        assert int(info["n_edges"]) == -1 and (outlier == pc.SENTINEL).all()
        assert pose.tobytes() == c["pose"][0].tobytes()
    if name == "at_optimum":
        assert r["trace"]["term_rho0"] == 4 and r["lm_iterations"] == 4 and r["n_inliers"] == 19
        # (mOw comes back as -0: it is recomputed from the unchanged rcw and tcw)
        assert pose["rcw"].tobytes() == c["pose"]["rcw"][0].tobytes() and not pose["tcw"].any()


# ----------------------------------------------------------------------- chain
LS = np.float32(math.log(np.float32(1.2)))


def test_tracking_chain_device_resident(gpu, oracle):
    """isInFrustum -> SearchByProjection(F, localMap) with mvuRight ->
    PoseOptimization on its d_kp_match and the map points -> isInFrustum at
    d_pose_out, with no host copy in between; each stage against its reference
    on the same inputs."""
    torch = pytest.importorskip("torch")
    W, H, F, M = 1241, 376, 2, 3000
    cam = scenarios.camera()
    scale = oracle.params(1000)["scale"]
    levels = (f32(1.0) / (scale * scale)).astype(f32)
    refs = []
    for f in range(F):
        k, d, _ = oracle.extract(oracle.synth_image(70 + f, 0, W, H), 1000)
        pose, P, mpd = scenarios.local_map_3d(oracle, k, d, M, W, H, rng_seed=70 + f)
        _, tr = oracle.frustum(P, pose, cam, W, H, 0.5, LS, 8)
        _, km_mono = oracle.match_projection_local(k, d, scale, W, H, tr, mpd, 3.0, 0.8, None)
        ur = np.full(len(k), -1, f32)
        hit = (km_mono >= 0) & (np.arange(len(k)) % 3 != 0)
        ur[hit] = tr["proj_xr"][km_mono[hit]]
        nm, km = oracle.match_projection_local(k, d, scale, W, H, tr, mpd, 3.0, 0.8, None, ur)
        r = pc.ref.pose_optimization(np.stack([k["x"], k["y"]], 1), k["octave"], ur, km, P["pos"],
                                     levels, cam, pose["rcw"][0], pose["tcw"][0], pose["ow"][0],
                                     np.full(len(k), pc.SENTINEL, np.uint8))
        pose2 = np.zeros(1, gpu.POSE_DTYPE)
        pose2["rcw"], pose2["tcw"], pose2["ow"] = r["rcw"], r["tcw"], r["ow"]
        n2, tr2 = oracle.frustum(P, pose2, cam, W, H, 0.5, LS, 8)
        # (nmatches also counts assignments a later map point overwrote)
        assert nm > 100 and r["n_edges"] == (km >= 0).sum() > 100 and 10 < r["n_inliers"]
        assert (ur >= 0).sum() > 50
        refs.append(dict(k=k, d=d, pose=pose, P=P, mpd=mpd, ur=ur, tr=tr, km=km, nm=nm, r=r,
                         n2=n2, tr2=tr2))
    cap = 1100
    kk = np.zeros((F, cap), gpu.KEYPOINT_DTYPE)
    dd = np.zeros((F, cap, 32), np.uint8)
    ur = np.full((F, cap), -1, f32)
    Pall = np.zeros((F, M), gpu.MAP_POINT_DTYPE)
    md = np.zeros((F, M, 32), np.uint8)
    poses = np.zeros(F, gpu.POSE_DTYPE)
    nk = np.zeros(F, np.int32)
    for f, q in enumerate(refs):
        n = len(q["k"])
        nk[f] = n
        kk[f, :n], dd[f, :n], ur[f, :n] = q["k"], q["d"], q["ur"]
        Pall[f], md[f], poses[f] = q["P"], q["mpd"], q["pose"][0]
    d_k, d_d, d_ur, d_P, d_md, d_pose, d_nk = (
        _dev(torch, a) for a in (kk, dd, ur, Pall, md, poses, nk))
    d_nm = torch.full((F,), M, dtype=torch.int32, device="cuda")
    tsz = gpu.MP_TRACK_DTYPE.itemsize
    d_tr = torch.zeros(F * M * tsz, dtype=torch.uint8, device="cuda")
    d_tr2 = torch.zeros(F * M * tsz, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(F, dtype=torch.int32, device="cuda")
    d_cnt2 = torch.zeros(F, dtype=torch.int32, device="cuda")
    d_km = torch.full((F * cap,), -7, dtype=torch.int32, device="cuda")
    d_nmatch = torch.zeros(F, dtype=torch.int32, device="cuda")
    d_pout = torch.zeros(F * gpu.POSE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_outl = torch.full((F * cap,), pc.SENTINEL, dtype=torch.uint8, device="cuda")
    d_info = torch.zeros(F * 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m = gpu.ORBmatcher(0.8)
    m.frustum_batch(F, d_P.data_ptr(), d_nm.data_ptr(), M, d_pose.data_ptr(), cam, 0.0, float(W),
                    0.0, float(H), 0.5, LS, 8, d_tr.data_ptr(), d_cnt.data_ptr())
    m.search_by_projection_batch_stereo(F, d_k.data_ptr(), d_d.data_ptr(), d_ur.data_ptr(),
                                        d_nk.data_ptr(), 0, cap, d_tr.data_ptr(), d_md.data_ptr(),
                                        d_nm.data_ptr(), M, W, H, scale, 3.0, d_km.data_ptr(),
                                        d_nmatch.data_ptr())
    m.pose_optimization_batch(F, d_nk.data_ptr(), d_k.data_ptr(), d_ur.data_ptr(), cap,
                              d_km.data_ptr(), d_P.data_ptr(), gpu.MAP_POINT_DTYPE.itemsize, M,
                              levels, cam, d_pose.data_ptr(), d_pout.data_ptr(),
                              d_outl.data_ptr(), d_info.data_ptr())
    m.frustum_batch(F, d_P.data_ptr(), d_nm.data_ptr(), M, d_pout.data_ptr(), cam, 0.0, float(W),
                    0.0, float(H), 0.5, LS, 8, d_tr2.data_ptr(), d_cnt2.data_ptr())
    torch.cuda.synchronize()
    km = _host(d_km, np.int32, (F, cap))
    tr = _host(d_tr, gpu.MP_TRACK_DTYPE, (F, M))
    tr2 = _host(d_tr2, gpu.MP_TRACK_DTYPE, (F, M))
    pout = _host(d_pout, gpu.POSE_DTYPE, (F,))
    outl = _host(d_outl, np.uint8, (F, cap))
    info = _host(d_info, gpu.POSE_OPT_INFO_DTYPE, (F,))
    for f, q in enumerate(refs):
        n = len(q["k"])
        assert tr[f].tobytes() == q["tr"].tobytes(), f
        assert int(d_nmatch[f].item()) == q["nm"] and np.array_equal(km[f, :n], q["km"]), f
        _assert_result(pout[f], outl[f, :n], info[f], q["r"], f)
        assert int(d_cnt2[f].item()) == q["n2"] and tr2[f].tobytes() == q["tr2"].tobytes(), f


# ---------------------------------------------------------------- stream order
def test_two_streams_one_handle(gpu):
    """Two batch calls on one handle, each on its own stream, with no host
    synchronisation between them: both run in the handle's scratch tier (the
    stride is above the LDS boundary), so the second must wait for the first."""
    torch = pytest.importorskip("torch")
    kp_stride = gpu.ORBmatcher.pose_optimization_lds_edges() + 16
    a = [_batch_case(i) for i in (6, 10, 0, 14)]
    b = [_batch_case(i) for i in (11, 3, 8)]
    run_a = _pack_batch(gpu, torch, [c for c, _ in a], kp_stride, "f3")
    run_b = _pack_batch(gpu, torch, [c for c, _ in b], kp_stride, "mp")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    m = gpu.ORBmatcher()
    o1 = run_a(m, s1.cuda_stream)
    o2 = run_b(m, s2.cuda_stream)
    torch.cuda.synchronize()
    _check_batch(gpu, a, kp_stride, *o1)
    _check_batch(gpu, b, kp_stride, *o2)
