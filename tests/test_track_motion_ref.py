"""CPU checks of tests/track_motion_ref.py, the numpy float32 restatement the
GPU tests of the device-batched SearchByProjection(CurrentFrame, LastFrame)
compare against: hand-computed answers, the identity-pose round trip of every
frame-flavour generator of matcher_edge_cases.py, and pyref against the oracle
on the helper's records."""
import functools

import numpy as np
import pytest

import matcher_edge_cases as E
import pyref
import scenarios as S
import track_motion_ref as R

f32 = np.float32


def frame_case_names():
    return sorted(n for n in E.CASES if "frame" in n and not n.startswith("bow"))


@functools.lru_cache(maxsize=None)
def case(name):
    return E.CASES[name][0]()


# ---------------------------------------------------------------- hand-computed
def test_rotated_pose_one_point():
    # 90 degrees about z, t = (1, 2, 3), x3Dw = (4, 5, 6): x3Dc = (-5 + 1, 4 + 2, 6 + 3)
    Rz = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    xc, yc, invzc = R.project(R.pose(Rz, (1, 2, 3)), (4, 5, 6))
    assert (xc, yc) == (f32(-4), f32(6)) and invzc == f32(1.0) / f32(9.0)
    # twc = -R^T t = -(2, -1, 3); identity last pose with tlw = (0, 0, 10): tlc.z = 7
    assert np.array_equal(R.twc(R.pose(Rz, (1, 2, 3))), np.array([-2, 1, -3], f32))
    assert R.tlc(R.pose(Rz, (1, 2, 3)), R.pose(t=(0, 0, 10)))[2] == f32(7)
    pts = np.zeros(1, R.MAP_POINT_DTYPE)
    pts["pos"][0] = (4, 5, 6)
    pts["has_obs"] = 1
    keys = np.zeros(1, R.KEYPOINT_DTYPE)
    keys["octave"], keys["angle"] = 3, 45.0
    last, desc = R.last_records(R.pose(Rz, (1, 2, 3)), keys, [0], None, pts,
                                np.full((1, 32), 7, np.uint8))
    L = last[0]
    assert (L["xc"], L["yc"], L["invzc"]) == (f32(-4), f32(6), f32(1.0) / f32(9.0))
    assert (L["last_octave"], L["last_angle"], L["valid"], L["has_obs"], L["mp_id"]) == \
        (3, f32(45.0), 1, 1, 0)
    assert (desc == 7).all()


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_tlc_z_equal_to_mb_is_neither(sign):
    mb = E.CAM[5]
    cur, last = R.pose(), R.pose(t=(0, 0, sign * mb))
    assert R.tlc(cur, last)[2].tobytes() == f32(sign * mb).tobytes()   # tlc = tlw bit for bit
    assert R.forward_backward(cur, last, mb, mono=False) == (False, False)
    up = np.nextafter(f32(mb), f32(np.inf))
    fb = R.forward_backward(cur, R.pose(t=(0, 0, sign * up)), mb, mono=False)
    assert fb == ((True, False) if sign > 0 else (False, True))
    assert R.forward_backward(cur, R.pose(t=(0, 0, sign * up)), mb, mono=True) == (False, False)


def test_point_behind_the_camera():
    xc, yc, invzc = R.project(R.pose(), (1, 2, -4))
    assert invzc == f32(-0.25) and invzc < 0
    pts = np.zeros(2, R.MAP_POINT_DTYPE)
    pts["pos"][0], pts["pos"][1] = (1, 2, -4), (0, 0, 0)
    last, _ = R.last_records(R.pose(), np.zeros(2, R.KEYPOINT_DTYPE), [0, 1], None, pts,
                             np.zeros((2, 32), np.uint8))
    assert last["invzc"][0] < 0 and last["valid"][0] == 1      # the matcher's invzc < 0 gate drops it
    assert np.isinf(last["invzc"][1]) and last["invzc"][1] > 0  # z = 0: +inf, not negative


def test_null_and_outlier_entries_are_invalid():
    pts = np.zeros(3, R.MAP_POINT_DTYPE)
    pts["pos"][:, 2] = 5
    keys = np.zeros(4, R.KEYPOINT_DTYPE)
    last, _ = R.last_records(R.pose(), keys, [-1, -2, 2, 1], [0, 0, 1, 0], pts,
                             np.zeros((3, 32), np.uint8))
    assert last["valid"].tolist() == [0, 0, 0, 1] and last["mp_id"].tolist() == [-1, -1, -1, 1]


@pytest.mark.parametrize("first,retried", [(19, 1), (20, 0)])
def test_retry_rule(first, retried):
    calls = []

    def match(th):
        calls.append(th)
        return (first if len(calls) == 1 else 33), np.full(3, len(calls), np.int32)

    km, n, n_first, r = R.with_retry(match, 7.0, 20)
    assert r == retried and n_first == first and calls[0] == f32(7.0)
    if retried:
        assert calls == [f32(7.0), f32(14.0)] and n == 33 and (km == 2).all()
    else:
        assert len(calls) == 1 and n == 20 and (km == 1).all()
    calls.clear()
    assert R.with_retry(match, 7.0, 0)[3] == 0 and len(calls) == 1   # retry_below 0: never


def test_discard_loop_branches():
    pts = np.zeros(6, R.MAP_POINT_DTYPE)
    pts["has_obs"] = [1, 0, 1, 1, 1, 1]
    pts["bad"] = [0, 0, 0, 1, 0, 0]
    #        NULL, -2, outlier, kept obs, kept no obs, kept bad, outlier flag on a NULL
    km = np.array([-1, -2, 0, 2, 1, 3, -1], np.int32)
    ol = np.array([0, 0, 1, 0, 0, 0, 1], np.uint8)
    k2, o2, p2, out = R.discard_outliers(km, ol, pts, 10, mark_seen=False)
    assert k2.tolist() == [-1, -2, -1, 2, 1, 3, -1]
    assert o2.tolist() == [0, 0, 0, 0, 0, 0, 1]           # an unmatched keypoint's flag stays
    assert (out["n_matches"], out["n_matches_map"], out["n_discarded"]) == (9, 2, 1)
    assert not p2["seen"].any()
    k3, o3, p3, out3 = R.discard_outliers(km, ol, pts, 10, mark_seen=True)
    assert k3.tolist() == [-1, -2, -1, 2, 1, -1, -1]      # the kept bad point becomes NULL
    assert out3.tolist() == out.tolist() and np.array_equal(o3, o2)
    assert p3["seen"].tolist() == [1, 1, 1, 0, 0, 0]      # discarded 0, kept 2 and 1; bad 3 not


# ------------------------------------------------------------------ identity pose
@pytest.mark.parametrize("name", frame_case_names())
def test_identity_pose_reproduces_the_records(name):
    c = case(name)
    assert c["family"] == "frame"
    p = R.problem_from_records(c["keys"], c["desc"], c["last"], c["last_desc"], c["tlc_z"],
                               c["locked"], c["u_right"])
    last, desc = R.last_records(p["pose_cur"], p["last_keys"], p["last_point_index"], None,
                                p["points"], p["mp_desc"])
    ref = np.asarray(c["last"], R.LAST_MP_DTYPE)
    v = ref["valid"] != 0
    assert np.array_equal(last["valid"] != 0, v)
    for f in ("xc", "yc", "invzc"):
        assert last[f][v].tobytes() == ref[f][v].tobytes(), f
    for f in ("last_octave", "last_angle", "has_obs"):
        assert np.array_equal(last[f][v], ref[f][v]), f
    assert np.array_equal(desc[v], np.asarray(c["last_desc"]).reshape(-1, 32)[v])
    assert R.tlc(p["pose_cur"], p["pose_last"])[2].tobytes() == f32(c["tlc_z"]).tobytes()
    fwd = c["tlc_z"] > E.CAM[5] and not c["mono"]
    bwd = -c["tlc_z"] > E.CAM[5] and not c["mono"]
    assert R.forward_backward(p["pose_cur"], p["pose_last"], E.CAM[5], c["mono"]) == (fwd, bwd)


@pytest.mark.parametrize("name", ["gates_frame", "crowded_frame_stereo_fwd"])
def test_helper_search_equals_the_generators_oracle_run(oracle, name):
    """The whole helper path at the identity pose: the same matches as the
    oracle on the generator's own records, ids mapped to indices."""
    c = case(name)
    p = R.problem_from_records(c["keys"], c["desc"], c["last"], c["last_desc"], c["tlc_z"],
                               c["locked"], c["u_right"])
    km, info = R.search(oracle, p, E.CAM, E.SCALE, E.W, E.H, c["th"], c["mono"], c["check_ori"], 0)
    n, ref = E.run_oracle(oracle, c)
    assert info["n_matches"] == n and info["retried"] == 0
    assert np.array_equal(km, np.where(ref >= 0, ref - 1000, ref))


# -------------------------------------------------------------------- cross-check
@pytest.mark.parametrize("seed,mono,th", [(2, 1, 15.0), (5, 0, 7.0)])
def test_pyref_equals_oracle_on_helper_records(oracle, seed, mono, th):
    """Two natural scenes, the map points back-projected through a rotated
    current pose: pyref's frame matcher and the oracle agree on the records the
    helper derives."""
    fp = S.frame_pair(oracle, seed, rng_seed=seed)
    rng = np.random.default_rng(seed)
    Rm, t, _ = S.pose(rng)
    last0 = fp["last"]
    with np.errstate(divide="ignore"):
        pc = np.stack([last0["xc"], last0["yc"], 1.0 / last0["invzc"].astype(np.float64)], 1)
    pw = ((pc - t.astype(np.float64)) @ Rm.astype(np.float64)).astype(f32)   # R^T (Pc - t)
    pts = np.zeros(len(last0), R.MAP_POINT_DTYPE)
    pts["pos"], pts["has_obs"] = pw, last0["has_obs"]
    idx = np.where(last0["valid"] != 0, np.arange(len(last0)), -1)
    cur = R.pose(Rm, t)
    last, desc = R.last_records(cur, R.keys_from_last(last0), idx, None, pts, fp["last_desc"])
    v = last0["valid"] != 0
    assert np.allclose(last["xc"][v] * last["invzc"][v], last0["xc"][v] * last0["invzc"][v],
                       atol=1e-3)
    tz = float(R.tlc(cur, R.pose(Rm, t + np.array([0, 0, 1.0], f32)))[2])
    args = (fp["kb"], fp["db"], fp["scale"], fp["w"], fp["h"], last, desc, S.camera(), tz, th,
            mono, 1, None, None)
    ref = oracle.match_projection_frame(*args)
    got = pyref.search_by_projection_frame(*args)
    assert ref[0] > 100
    assert ref[0] == got[0] and np.array_equal(ref[1], got[1])
