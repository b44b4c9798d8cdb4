"""GPU parity of the RGB-D depth path (depth_kernels.hip) and of the stereo
form of the batched local-map matcher, bit for bit against tests/rgbd_ref.py
and the CPU oracle: Frame::ComputeStereoFromRGBD with GrabImageRGBD's
conversion, Frame::UnprojectStereo, the closest-point selection and counts of
Tracking, and SearchByProjection(F, localMap) with mvuRight in a device batch."""
import numpy as np
import pytest

import rgbd_ref
import scenarios
from rgbd_cases import BREAK_CASES, keypoints

pytestmark = pytest.mark.gpu
f32 = np.float32


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def _host(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# --------------------------------------------------------------- depth sampling
COLS, ROWS, PITCH_ELEMS = 64, 48, 67   # rows of 67 elements: 268 B (f32) / 134 B (u16)
_CONV = [(np.float32, 1.0), (np.float32, 1.0 + 2e-5), (np.uint16, 1.0), (np.uint16, 1.0 / 5000.0)]
_CONV_IDS = ["f32_1", "f32_1p2e-5", "u16_1", "u16_5000"]
# pixels (row, col) holding the special values, and a keypoint on each
_SPECIAL = [(3, 5), (4, 6), (5, 7), (6, 8), (7, 9), (8, 10)]


def _depth_image(dtype, seed):
    """Padded 64 x 48 image (a view into rows of PITCH_ELEMS elements)."""
    rng = np.random.default_rng(seed)
    buf = np.zeros((ROWS, PITCH_ELEMS), dtype)
    if dtype == np.float32:
        buf[:] = rng.uniform(0.3, 12.0, buf.shape).astype(f32)
        special = [0.0, -2.5, np.nan, np.inf, 1e-40, 0.004]   # 1e-40: a denormal
    else:
        buf[:] = rng.integers(300, 60000, buf.shape)
        special = [0, 65535, 1, 0, 65535, 2]
    buf[rng.random(buf.shape) < 0.1] = 0
    for (r, c), v in zip(_SPECIAL, special):
        buf[r, c] = v
    buf[ROWS - 1, COLS - 1] = 7   # the last pixel holds a valid depth
    buf[:, COLS:] = 0xFFFF if dtype == np.uint16 else 1e9   # padding: never sampled
    return buf


def _sample_keys(n, seed):
    """mvKeys (fractional, as on levels >= 1) and mvKeysUn for n >= 12 slots."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform([0, 0], [COLS, ROWS], (n, 2)).astype(f32)
    fixed = [(c + 0.37, r + 0.81) for r, c in _SPECIAL]
    fixed += [(19.999, 5.5),                  # truncates to column 19
              (COLS - 1 + 0.9, ROWS - 1 + 0.9),   # last column, last row
              (float(COLS), 3.0),             # outside: -1 / -1
              (3.0, -1.0),                    # outside
              (10.4, 8.6),                    # the 0.004 pixel / u16 2: u_right far negative
              (np.nan, 2.0)]
    m = min(n, len(fixed))
    xy[:m] = np.array(fixed[:m], f32)
    keys = keypoints(xy)
    un = keys.copy()
    un["x"] += rng.uniform(-1.5, 1.5, n).astype(f32)
    un["y"] += rng.uniform(-1.5, 1.5, n).astype(f32)
    return keys, un


@pytest.mark.parametrize("dtype,factor", _CONV, ids=_CONV_IDS)
def test_stereo_from_rgbd_one_frame(gpu, dtype, factor):
    buf = _depth_image(dtype, 1)
    img = buf[:, :COLS]
    assert img.strides[0] % 16 != 0 and img.strides[0] > COLS * img.itemsize
    keys, un = _sample_keys(200, 2)
    bf = f32(40.0)
    m = gpu.ORBmatcher()
    ur, z = m.ComputeStereoFromRGBD(keys, un, img, factor, bf)
    ur_ref, z_ref = rgbd_ref.stereo_from_rgbd(keys, un, img, factor, bf)
    assert _bits(z) == _bits(z_ref), np.nonzero(z.view(np.uint32) != z_ref.view(np.uint32))[0][:10]
    assert _bits(ur) == _bits(ur_ref)
    # the cases the image was built for are really there
    assert z_ref[8] == -1 and ur_ref[8] == -1 and z_ref[11] == -1   # outside / NaN position
    assert z_ref[7] > 0                                             # last pixel
    assert (ur_ref[z_ref > 0] < 0).any() and (z_ref == -1).sum() > 10
    if dtype == np.float32:
        assert np.isinf(z_ref[3]) and z_ref[2] == -1 and z_ref[1] == -1 and 0 < z_ref[4] < 1e-37
    ur0, z0 = m.ComputeStereoFromRGBD(keys[:0], un[:0], img, factor, bf)
    assert len(ur0) == 0 and len(z0) == 0


@pytest.mark.parametrize("dtype,factor", _CONV, ids=_CONV_IDS)
def test_stereo_from_rgbd_batch(gpu, dtype, factor):
    torch = pytest.importorskip("torch")
    stride = 130
    counts = np.array([0, 1, 64, 65, stride], np.int32)
    F = len(counts)
    imgs = np.stack([_depth_image(dtype, 10 + f) for f in range(F)])
    keys = np.zeros((F, stride), gpu.KEYPOINT_DTYPE)
    un = np.zeros((F, stride), gpu.KEYPOINT_DTYPE)
    for f in range(F):
        keys[f], un[f] = _sample_keys(stride, 20 + f)
    es = imgs.itemsize
    d_img, d_keys, d_un, d_n = (_dev(torch, a) for a in (imgs, keys, un, counts))
    d_ur = torch.full((F * stride,), 7.0, dtype=torch.float32, device="cuda")
    d_z = torch.full((F * stride,), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    bf = f32(40.0)
    m = gpu.ORBmatcher()
    m.stereo_from_rgbd_batch(F, d_n.data_ptr(), d_keys.data_ptr(), d_un.data_ptr(), stride,
                             d_img.data_ptr(), gpu.ORB_DEPTH_U16 if dtype == np.uint16
                             else gpu.ORB_DEPTH_F32, COLS, ROWS, PITCH_ELEMS * es,
                             ROWS * PITCH_ELEMS * es, factor, bf, d_ur.data_ptr(), d_z.data_ptr())
    torch.cuda.synchronize()
    ur = _host(d_ur, f32, (F, stride))
    z = _host(d_z, f32, (F, stride))
    for f in range(F):
        n = int(counts[f])
        ur_ref, z_ref = rgbd_ref.stereo_from_rgbd(keys[f, :n], un[f, :n], imgs[f][:, :COLS],
                                                  factor, bf)
        assert _bits(z[f, :n]) == _bits(z_ref), f
        assert _bits(ur[f, :n]) == _bits(ur_ref), f
        assert (z[f, n:] == 7.0).all() and (ur[f, n:] == 7.0).all()   # untouched past the count


def test_stereo_from_rgbd_rejects_bad_images(gpu):
    m = gpu.ORBmatcher()
    keys, un = _sample_keys(20, 0)
    with pytest.raises(gpu.OrbError):
        m.ComputeStereoFromRGBD(keys, un, np.zeros((4, 4), np.uint8), 1.0, 40.0)
    L = gpu.lib()
    img = np.zeros((4, 8), np.uint16)
    out = np.zeros(20, f32)
    args = lambda typ, row_bytes: (m.handle, 20, gpu._ptr(keys), gpu._ptr(un), gpu._ptr(img), typ,
                                   8, 4, row_bytes, 1.0, 40.0, gpu._ptr(out), gpu._ptr(out))
    assert L.orb_stereo_from_rgbd(*args(2, 16)) == gpu.ORB_EINVAL    # unknown type
    assert L.orb_stereo_from_rgbd(*args(0, 14)) == gpu.ORB_EINVAL    # pitch below cols x 2
    assert L.orb_stereo_from_rgbd(*args(0, 17)) == gpu.ORB_EINVAL    # pitch not a multiple of 2


# -------------------------------------------------------------------- unproject
def _unproject_inputs(n, seed):
    rng = np.random.default_rng(seed)
    keys = keypoints(rng.uniform([0, 0], [1241, 376], (n, 2)).astype(f32))
    z = rng.uniform(0.5, 60.0, n).astype(f32)
    z[rng.random(n) < 0.2] = -1.0
    # (no +inf: inf - inf is a NaN whose sign differs between processors)
    special = [0.0, -0.0, np.nan, 1e-40, 2.5, -3.0]
    z[:min(n, len(special))] = special[:min(n, len(special))]
    return keys, z


@pytest.mark.parametrize("general", [False, True], ids=["identity", "general"])
def test_unproject_stereo_one_frame(gpu, general):
    keys, z = _unproject_inputs(300, 5)
    if general:
        R, t, ow = scenarios.pose(np.random.default_rng(3))
    else:
        R, t, ow = np.eye(3, dtype=f32), np.zeros(3, f32), np.zeros(3, f32)
    pose = np.zeros(1, gpu.POSE_DTYPE)
    pose["rcw"], pose["tcw"], pose["ow"] = R.reshape(1, 9), t, ow
    cam = scenarios.camera()
    x3d, valid = gpu.ORBmatcher().UnprojectStereo(keys, z, pose, cam)
    x_ref, v_ref = rgbd_ref.unproject_stereo(keys, z, R.reshape(9), ow, *cam[:4])
    assert _bits(valid) == _bits(v_ref)
    assert _bits(x3d) == _bits(x_ref), np.nonzero((x3d.view(np.uint32) != x_ref.view(np.uint32)).any(1))[0][:10]
    assert 0 < v_ref.sum() < len(z) and not v_ref[:3].any() and v_ref[3] and v_ref[4]


def test_unproject_stereo_batch(gpu):
    torch = pytest.importorskip("torch")
    stride = 130
    counts = np.array([0, 1, 64, 65, stride], np.int32)
    F = len(counts)
    rng = np.random.default_rng(9)
    keys = np.zeros((F, stride), gpu.KEYPOINT_DTYPE)
    z = np.zeros((F, stride), f32)
    poses = np.zeros(F, gpu.POSE_DTYPE)
    for f in range(F):
        keys[f], z[f] = _unproject_inputs(stride, 30 + f)
        R, t, ow = scenarios.pose(rng)
        poses[f]["rcw"], poses[f]["tcw"], poses[f]["ow"] = R.reshape(9), t, ow
    z[1, 0] = 3.25
    d_keys, d_z, d_pose, d_n = (_dev(torch, a) for a in (keys, z, poses, counts))
    d_x = torch.full((F * stride * 3,), 7.0, dtype=torch.float32, device="cuda")
    d_v = torch.full((F * stride,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    cam = scenarios.camera()
    gpu.ORBmatcher().unproject_stereo_batch(F, d_n.data_ptr(), d_keys.data_ptr(), d_z.data_ptr(),
                                            stride, d_pose.data_ptr(), cam, d_x.data_ptr(),
                                            d_v.data_ptr())
    torch.cuda.synchronize()
    x = _host(d_x, f32, (F, stride, 3))
    v = _host(d_v, np.uint8, (F, stride))
    for f in range(F):
        n = int(counts[f])
        x_ref, v_ref = rgbd_ref.unproject_stereo(keys[f, :n], z[f, :n], poses[f]["rcw"],
                                                 poses[f]["ow"], *cam[:4])
        assert _bits(v[f, :n]) == _bits(v_ref), f
        assert _bits(x[f, :n]) == _bits(x_ref), f
        assert (v[f, n:] == 9).all() and (x[f, n:] == 7.0).all()


# ----------------------------------------------------------------- close points
def _random_frame(n, seed, th=f32(6.0)):
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.2, 40.0, n).astype(f32)
    z[rng.random(n) < 0.15] = -1.0
    z[rng.random(n) < 0.05] = 0.0
    if n > 20:
        z[3], z[9], z[11], z[17] = th, np.inf, np.nan, z[5]   # z == th, +inf, NaN, a tie
    return z, th


def _close_cases():
    """name -> (depth, th): the break-rule frames of test_rgbd_ref and random
    frames at the wave / workgroup boundaries and beyond the LDS tier."""
    cases = {}
    for name in sorted(BREAK_CASES):
        z, th, _, _ = BREAK_CASES[name]()
        cases[name] = (z, th)
    for n in (63, 64, 65, 1000, 20000):
        cases[f"random_{n}"] = _random_frame(n, n)
    cases["empty"] = (np.zeros(0, f32), f32(6.0))
    cases["none_positive"] = (np.array([0.0, -1.0, np.nan], f32), f32(6.0))
    return cases


def _states(n, seed):
    rng = np.random.default_rng(seed + 77)
    return (rng.integers(0, 3, n).astype(np.uint8), (rng.random(n) < 0.2).astype(np.uint8))


def _close_ref(z, ms, ol, th):
    order, create = rgbd_ref.close_points(z, ms, th)
    return order, create, rgbd_ref.close_counts(z, ms, ol, th)


@pytest.fixture(scope="module")
def close_refs():
    out = {}
    for i, (name, (z, th)) in enumerate(_close_cases().items()):
        ms, ol = _states(len(z), i)
        out[name] = (z, th, ms, ol, _close_ref(z, ms, ol, th))
    return out


@pytest.mark.parametrize("name", list(_close_cases()))
def test_close_points_one_frame(gpu, close_refs, name):
    z, th, ms, ol, (order_ref, create_ref, counts_ref) = close_refs[name]
    m = gpu.ORBmatcher()
    if name == "random_20000":   # the global-scratch tier
        assert len(z) > m.close_points_lds_keys()
    elif len(z):
        assert len(z) <= m.close_points_lds_keys()
    order, create, tracked, non_tracked = m.ClosePoints(z, ms, ol, th)
    assert np.array_equal(order, order_ref)
    assert _bits(create) == _bits(create_ref)
    assert (tracked, non_tracked) == counts_ref
    if name in BREAK_CASES:
        _, _, n_sorted, n_visit = BREAK_CASES[name]()
        assert (len(order), len(create)) == (n_sorted, n_visit)


@pytest.mark.parametrize("stride", [1024, 20000], ids=["lds", "global_scratch"])
def test_close_points_batch(gpu, close_refs, stride):
    torch = pytest.importorskip("torch")
    m = gpu.ORBmatcher()
    assert (stride > m.close_points_lds_keys()) == (stride == 20000)
    names = [k for k, v in close_refs.items() if len(v[0]) <= stride]
    assert "empty" in names and ("random_20000" in names) == (stride == 20000)
    F = len(names)
    z = np.full((F, stride), 5.0, f32)          # slots past the count hold valid-looking data
    ms = np.zeros((F, stride), np.uint8)
    ol = np.zeros((F, stride), np.uint8)
    counts = np.zeros(F, np.int32)
    for f, k in enumerate(names):
        n = len(close_refs[k][0])
        counts[f] = n
        z[f, :n], ms[f, :n], ol[f, :n] = close_refs[k][0], close_refs[k][2], close_refs[k][3]
    th = f32(5.0)   # one threshold per call: every frame's reference is taken at this one
    d_z, d_ms, d_ol, d_n = (_dev(torch, a) for a in (z, ms, ol, counts))
    d_order = torch.full((F * stride,), 12345, dtype=torch.int32, device="cuda")
    d_create = torch.full((F * stride,), 9, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((F * 4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):   # the second call reuses the scratch of the first
        m.close_points_batch(F, d_n.data_ptr(), d_z.data_ptr(), d_ms.data_ptr(), d_ol.data_ptr(),
                             stride, th, d_order.data_ptr(), d_create.data_ptr(),
                             d_counts.data_ptr())
    torch.cuda.synchronize()
    order = _host(d_order, np.int32, (F, stride))
    create = _host(d_create, np.uint8, (F, stride))
    got = _host(d_counts, np.int32, (F, 4))
    for f, k in enumerate(names):
        n = int(counts[f])
        order_ref, create_ref, (tr, non) = _close_ref(z[f, :n], ms[f, :n], ol[f, :n], th)
        assert got[f].tolist() == [len(order_ref), len(create_ref), tr, non], k
        assert np.array_equal(order[f, :len(order_ref)], order_ref), k
        assert (order[f, len(order_ref):] == -1).all(), k
        assert _bits(create[f, :len(create_ref)]) == _bits(create_ref), k
        assert not create[f, len(create_ref):].any(), k


# -------------------------------------------------- stereo batch SearchByProjection
W, H = 640, 480
N_BASE = 4


@pytest.fixture(scope="module")
def stereo_problems(oracle):
    """128 problems of about 300 keypoints and 600 map points: four extracted
    frames, a local map and an mvuRight per problem.  mvuRight is -1 for a
    third of the keypoints; for the others it agrees with the stereo
    projection of the map point the monocular search assigns (passes the
    check) or is 100 px off it (fails the check for the best candidate)."""
    scale = oracle.params(300)["scale"]
    frames = []
    for s in range(N_BASE):
        k, d, _ = oracle.extract(oracle.synth_image(40 + s, 0, W, H), 300)
        frames.append((k, d))
    probs = []
    for p in range(128):
        k, d = frames[p % N_BASE]
        rng = np.random.default_rng(500 + p)
        mps, mpd, locked = oracle.synth_local_map(500 + p, k, d, 600, W, H)
        mps["proj_xr"] = mps["proj_x"] - rng.uniform(5, 40, len(mps)).astype(f32)
        n_mono, km_mono = oracle.match_projection_local(k, d, scale, W, H, mps, mpd, 3.0, 0.8, locked)
        kind = rng.integers(0, 3, len(k))
        ur = (k["x"] - rng.uniform(5, 40, len(k))).astype(f32)
        hit = km_mono >= 0
        ur[hit] = mps["proj_xr"][km_mono[hit]]
        ur[kind == 1] += f32(100.0)
        ur[kind == 2] = -1.0
        n_ref, km_ref = oracle.match_projection_local(k, d, scale, W, H, mps, mpd, 3.0, 0.8,
                                                      locked, ur)
        probs.append(dict(k=k, d=d, mps=mps, mpd=mpd, locked=locked, ur=ur, n=n_ref, km=km_ref,
                          differs=not np.array_equal(km_ref, km_mono)))
    return scale, probs


def _pack(gpu, torch, probs, kp_stride, mp_stride):
    P = len(probs)
    kk = np.zeros((P, kp_stride), gpu.KEYPOINT_DTYPE)
    dd = np.zeros((P, kp_stride, 32), np.uint8)
    lk = np.zeros((P, kp_stride), np.uint8)
    ur = np.full((P, kp_stride), 3.0, f32)
    mp = np.zeros((P, mp_stride), gpu.MP_TRACK_DTYPE)
    md = np.zeros((P, mp_stride, 32), np.uint8)
    nk = np.zeros(P, np.int32)
    nm = np.zeros(P, np.int32)
    for i, q in enumerate(probs):
        n, M = len(q["k"]), len(q["mps"])
        nk[i], nm[i] = n, M
        kk[i, :n], dd[i, :n], lk[i, :n], ur[i, :n] = q["k"], q["d"], q["locked"], q["ur"]
        mp[i, :M], md[i, :M] = q["mps"], q["mpd"]
    return [_dev(torch, a) for a in (kk, dd, ur, nk, lk, mp, md, nm)]


_SCHED = [("auto", 0), ("fixed_point", 2), ("jacobi", 3)]


@pytest.mark.parametrize("P", [1, 16, 128])
@pytest.mark.parametrize("name,schedule", _SCHED, ids=[s[0] for s in _SCHED])
def test_search_by_projection_batch_stereo(gpu, stereo_problems, name, schedule, P):
    torch = pytest.importorskip("torch")
    scale, probs = stereo_problems
    probs = probs[:P]
    assert any(q["differs"] for q in probs)   # the stereo check changes a result
    kp_stride, mp_stride = 330, 600
    assert max(len(q["k"]) for q in probs) <= kp_stride
    m = gpu.ORBmatcher(0.8)
    m.set_resolve(schedule, 4)
    want = {"fixed_point": "k_proj_resolve_fp<1024>", "jacobi": "k_proj_jacobi+k_proj_resolve_fp",
            "auto": {1: "k_proj_resolve_fp<1024>", 16: "k_proj_resolve<4>",
                     128: "k_proj_resolve<1>"}[P]}[name]
    assert m.resolve_kernel(P, kp_stride, mp_stride) == want
    dk, dd, dur, dnk, dlk, dmp, dmd, dnm = _pack(gpu, torch, probs, kp_stride, mp_stride)
    km = torch.full((P, kp_stride), -7, dtype=torch.int32, device="cuda")
    nmatch = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.search_by_projection_batch_stereo(P, dk.data_ptr(), dd.data_ptr(), dur.data_ptr(),
                                        dnk.data_ptr(), dlk.data_ptr(), kp_stride, dmp.data_ptr(),
                                        dmd.data_ptr(), dnm.data_ptr(), mp_stride, W, H, scale,
                                        3.0, km.data_ptr(), nmatch.data_ptr())
    torch.cuda.synchronize()
    km, nmatch = km.cpu().numpy(), nmatch.cpu().numpy()
    for i, q in enumerate(probs):
        assert int(nmatch[i]) == q["n"], i
        assert np.array_equal(km[i, :len(q["k"])], q["km"]), i


def test_search_by_projection_batch_stereo_eight_waves(gpu, oracle, stereo_problems):
    """Two problems above the 20,000-point threshold of k_proj_resolve<8> (the
    prefix schedule; the default takes the fixed-point kernel there)."""
    torch = pytest.importorskip("torch")
    scale, base = stereo_problems
    probs = []
    for p in range(2):
        q = base[p]
        k, d = q["k"], q["d"]
        rng = np.random.default_rng(900 + p)
        mps, mpd, locked = oracle.synth_local_map(900 + p, k, d, 20000 + 500 * p, W, H)
        mps["proj_xr"] = mps["proj_x"] - rng.uniform(5, 40, len(mps)).astype(f32)
        n_mono, km_mono = oracle.match_projection_local(k, d, scale, W, H, mps, mpd, 3.0, 0.8, locked)
        ur = (k["x"] - rng.uniform(5, 40, len(k))).astype(f32)
        hit = km_mono >= 0
        ur[hit] = mps["proj_xr"][km_mono[hit]]
        kind = rng.integers(0, 3, len(k))
        ur[kind == 1] += f32(100.0)
        ur[kind == 2] = -1.0
        n_ref, km_ref = oracle.match_projection_local(k, d, scale, W, H, mps, mpd, 3.0, 0.8,
                                                      locked, ur)
        assert not np.array_equal(km_ref, km_mono)
        probs.append(dict(k=k, d=d, mps=mps, mpd=mpd, locked=locked, ur=ur, n=n_ref, km=km_ref))
    kp_stride, mp_stride = 330, 20500
    m = gpu.ORBmatcher(0.8)
    m.set_resolve(m.RESOLVE_PREFIX)
    assert m.resolve_kernel(2, kp_stride, mp_stride) == "k_proj_resolve<8>"
    dk, dd, dur, dnk, dlk, dmp, dmd, dnm = _pack(gpu, torch, probs, kp_stride, mp_stride)
    km = torch.full((2, kp_stride), -7, dtype=torch.int32, device="cuda")
    nmatch = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.search_by_projection_batch_stereo(2, dk.data_ptr(), dd.data_ptr(), dur.data_ptr(),
                                        dnk.data_ptr(), dlk.data_ptr(), kp_stride, dmp.data_ptr(),
                                        dmd.data_ptr(), dnm.data_ptr(), mp_stride, W, H, scale,
                                        3.0, km.data_ptr(), nmatch.data_ptr())
    torch.cuda.synchronize()
    km, nmatch = km.cpu().numpy(), nmatch.cpu().numpy()
    for i, q in enumerate(probs):
        assert int(nmatch[i]) == q["n"], i
        assert np.array_equal(km[i, :len(q["k"])], q["km"]), i


def test_stereo_batch_requires_u_right(gpu):
    m = gpu.ORBmatcher(0.8)
    sc = np.ones(8, f32)
    st = gpu.lib().orb_match_projection_local_batch_stereo(
        m.handle, 1, 1, 1, None, 1, None, 8, 1, 1, 1, 8, 0.0, 640.0, 0.0, 480.0, 8, gpu._ptr(sc),
        1.0, 0.8, 1, 1, None)
    assert st == gpu.ORB_EINVAL   # (checked before any device work)


# ------------------------------------------------------------------------ chain
def test_rgbd_chain_device_resident(gpu, oracle):
    """extract -> undistort -> RGB-D depth -> stereo batch SearchByProjection on
    device buffers only, against the same chain through the oracle and
    rgbd_ref (TUM1 intrinsics, DepthMapFactor 5000)."""
    torch = pytest.importorskip("torch")
    nf, F = 1000, 2
    K, D = scenarios.cameras()["tum1"]
    bf, factor = f32(40.0), 1.0 / 5000.0
    imgs = np.stack([gpu.synth_image(11, f, W, H) for f in range(F)])
    rng = np.random.default_rng(4)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.stack([(4000 + 6 * xx + 9 * yy + 2500 * (imgs[f] > 128)).astype(np.uint16)
                      for f in range(F)])
    depth[rng.random(depth.shape) < 0.1] = 0
    ext = gpu.ORBextractor(nf, 1.2, 8, 20, 7)
    scale = np.float32(ext.GetScaleFactors())
    cap = ext.capacity(W, H)
    # host side of the comparison (also the source of the synthetic local maps)
    ref = []
    for f in range(F):
        k, d, _ = oracle.extract(imgs[f], nf)
        un = oracle.undistort_keypoints(k, K, D)
        ur, z = rgbd_ref.stereo_from_rgbd(k, un, depth[f], factor, bf)
        mps, mpd, locked = oracle.synth_local_map(60 + f, un, d, 3000, W, H)
        mps["proj_xr"] = mps["proj_x"] - rng.uniform(2, 12, len(mps)).astype(f32)
        n_ref, km_ref = oracle.match_projection_local(un, d, scale, W, H, mps, mpd, 3.0, 0.8,
                                                      locked, ur)
        n_mono, _ = oracle.match_projection_local(un, d, scale, W, H, mps, mpd, 3.0, 0.8, locked)
        ref.append(dict(n=len(k), ur=ur, z=z, mps=mps, mpd=mpd, locked=locked, nm=n_ref,
                        km=km_ref, mono=n_mono))
    assert any(r["nm"] != r["mono"] for r in ref)
    M = 3000
    lk = np.zeros((F, cap), np.uint8)
    mp = np.zeros((F, M), gpu.MP_TRACK_DTYPE)
    md = np.zeros((F, M, 32), np.uint8)
    for f, r in enumerate(ref):
        lk[f, :r["n"]], mp[f], md[f] = r["locked"], r["mps"], r["mpd"]
    d_img, d_depth, d_lk, d_mp, d_md = (_dev(torch, a) for a in (imgs, depth, lk, mp, md))
    d_nm = torch.full((F,), M, dtype=torch.int32, device="cuda")
    d_keys = torch.zeros(F * cap * 28, dtype=torch.uint8, device="cuda")
    d_un = torch.zeros(F * cap * 28, dtype=torch.uint8, device="cuda")
    d_desc = torch.zeros(F * cap * 32, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(F, dtype=torch.int32, device="cuda")
    d_ur = torch.zeros(F * cap, dtype=torch.float32, device="cuda")
    d_z = torch.zeros(F * cap, dtype=torch.float32, device="cuda")
    d_km = torch.full((F * cap,), -7, dtype=torch.int32, device="cuda")
    d_nmatch = torch.zeros(F, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m = gpu.ORBmatcher(0.8)
    s = ext.stream()
    ext.extract_batch(d_img.data_ptr(), F, W, H, W, W * H, d_keys.data_ptr(), d_desc.data_ptr(),
                      cap, d_n.data_ptr(), stream=s)
    m.undistort_keypoints_batch(F, d_n.data_ptr(), d_keys.data_ptr(), cap, K, D, d_un.data_ptr(),
                                stream=s)
    m.stereo_from_rgbd_batch(F, d_n.data_ptr(), d_keys.data_ptr(), d_un.data_ptr(), cap,
                             d_depth.data_ptr(), gpu.ORB_DEPTH_U16, W, H, W * 2, W * H * 2, factor,
                             bf, d_ur.data_ptr(), d_z.data_ptr(), stream=s)
    m.search_by_projection_batch_stereo(F, d_un.data_ptr(), d_desc.data_ptr(), d_ur.data_ptr(),
                                        d_n.data_ptr(), d_lk.data_ptr(), cap, d_mp.data_ptr(),
                                        d_md.data_ptr(), d_nm.data_ptr(), M, W, H, scale, 3.0,
                                        d_km.data_ptr(), d_nmatch.data_ptr(), stream=s)
    torch.cuda.synchronize()
    n = d_n.cpu().numpy()
    ur = _host(d_ur, f32, (F, cap))
    z = _host(d_z, f32, (F, cap))
    km = _host(d_km, np.int32, (F, cap))
    nmatch = d_nmatch.cpu().numpy()
    for f, r in enumerate(ref):
        assert int(n[f]) == r["n"]
        assert _bits(ur[f, :r["n"]]) == _bits(r["ur"]) and _bits(z[f, :r["n"]]) == _bits(r["z"])
        assert int(nmatch[f]) == r["nm"] and r["nm"] > 0
        assert np.array_equal(km[f, :r["n"]], r["km"]), f
