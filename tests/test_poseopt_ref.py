"""Hand-checkable answers for tests/poseopt_ref.py, the numpy restatement of
Optimizer::PoseOptimization that the GPU kernel is compared with (CPU tests)."""
import json
import math

import numpy as np
import pytest

import poseopt_cases as pc
import poseopt_ref as ref

f32, f64 = np.float32, np.float64


def _rng_quat(rng):
    q = rng.normal(0, 1, 4)
    q /= np.linalg.norm(q)
    return [float(v) for v in (q if q[3] >= 0 else -q)]


# ------------------------------------------------------------- whole problems
def test_noise_free_recovers_generating_pose():
    """Exact observations (up to their float32 storage) from a perturbed start:
    no flag is set and the pose comes back at the float32 rounding of the
    generating pose.  The bound: a stored observation is off by at most half a
    float32 ulp at 1,024 px (3.1e-5 px); one edge moves the translation by at
    most that times z / f <= 40 / 718 (1.7e-6 m) and the average over the 200
    edges by about 1 / sqrt(200) of it (1.2e-7, one ulp of a float32 near 1);
    the narrowing adds half an ulp.  Four ulps (4.8e-7) is the assertion."""
    c = pc.make_case(11, 260, 200, "mixed", noise=0.0, outlier_frac=0.0)
    r = pc.run_ref(c)
    assert r["n_edges"] == 200 and r["n_inliers"] == 200
    assert not r["outlier"][c["slots"]].any()
    R, t, ow = ref.pose_from_se3quat(c["truth"])
    start = np.concatenate([c["pose"]["rcw"][0], c["pose"]["tcw"][0]])
    got, want = np.concatenate([r["rcw"], r["tcw"]]), np.concatenate([R, t])
    residual = float(np.abs(got.astype(f64) - want.astype(f64)).max())
    moved = float(np.abs(start.astype(f64) - want.astype(f64)).max())
    print(f"residual {residual:.3e} (start pose off by {moved:.3e})")
    assert moved > 1e-2               # the start really was perturbed
    assert residual <= 4 * 2.0 ** -23
    assert float(np.abs(r["ow"].astype(f64) - ow.astype(f64)).max()) <= 8 * 2.0 ** -23


@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
def test_planted_outliers_are_the_flagged_set(kind):
    c = pc.make_case(21, 150, 120, kind, noise=0.0, outlier_frac=0.2)
    r = pc.run_ref(c)
    assert len(c["planted"]) > 10
    assert set(np.nonzero(r["outlier"] == 1)[0]) == set(c["planted"])
    assert r["n_inliers"] == 120 - len(c["planted"])
    no_edge = c["point_index"] < 0
    assert (r["outlier"][no_edge] == pc.SENTINEL).all()   # written only where there is an edge


def test_fewer_than_three_edges_returns_zero():
    c = pc.make_case(31, 20, 2, "mixed")
    r = pc.run_ref(c)
    assert r["n_inliers"] == 0 and r["n_edges"] == 2 and r["trace"]["rounds"] == 0
    assert r["rcw"].tobytes() == c["pose"]["rcw"][0].tobytes()
    assert r["tcw"].tobytes() == c["pose"]["tcw"][0].tobytes()
    assert not r["outlier"][c["slots"]].any()             # cleared at :301 / :342 all the same
    assert (r["outlier"][c["point_index"] < 0] == pc.SENTINEL).all()


def test_fewer_than_ten_edges_runs_one_round():
    assert pc.run_ref(pc.make_case(32, 20, 9, "mixed"))["trace"]["rounds"] == 1
    assert pc.run_ref(pc.make_case(33, 20, 10, "mixed"))["trace"]["rounds"] == 4
    assert pc.run_ref(pc.make_case(34, 20, 3, "mono"))["trace"]["rounds"] == 1


def test_bad_octave_is_reported():
    c = pc.make_case(35, 20, 12, "mixed")
    c["keys"]["octave"][c["slots"][0]] = -1
    r = pc.run_ref(c)
    assert r["n_edges"] == -1 and r["n_inliers"] == 0 and (r["outlier"] == pc.SENTINEL).all()


# ------------------------------------------------------------------- the parts
@pytest.mark.parametrize("scale,tol", [(0.3, 1e-12), (1e-6, 1e-10)])
def test_exp_against_expm(scale, tol):
    """SE3Quat::exp against the matrix exponential of the twist.  Below
    theta = 1e-5 the reference uses R = V = I + Omega + Omega^2 (its own TODO):
    R is off the true exponential by theta^2 / 2 <= 5e-11, and V, whose series
    is I + Omega / 2 + ..., by theta / 2 in first order, so the translation is
    compared within theta |upsilon|."""
    from scipy.linalg import expm
    rng = np.random.default_rng(5)
    for _ in range(20):
        u = np.concatenate([rng.normal(0, 1, 3) * scale, rng.normal(0, 1, 3)])
        theta = float(np.linalg.norm(u[:3]))
        small = theta < 1e-5
        assert small == (scale < 1e-5)
        tr = dict(exp_small=0, exp_large=0)
        q, t = ref.se3_exp([float(v) for v in u], trace=tr)
        assert tr["exp_small" if small else "exp_large"] == 1
        T = np.zeros((4, 4))
        T[:3, :3] = [[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]]
        T[:3, 3] = u[3:]
        E = expm(T)
        assert np.abs(np.array(ref.quat_to_matrix(q)) - E[:3, :3]).max() < tol
        t_tol = theta * float(np.linalg.norm(u[3:])) if small else tol * 10
        assert np.abs(np.array(t) - E[:3, 3]).max() < t_tol


def test_pinned_sincos_matches_libm():
    for x in [1e-5, 0.01, 0.7, 1.5, 1.6, 3.1, 3.2, 4.7, 6.2, 100.0]:
        s, c = ref.pinned_sincos_d(x)
        assert abs(s - math.sin(x)) <= 2.3e-16 and abs(c - math.cos(x)) <= 2.3e-16, x
    assert all(math.isnan(v) for v in ref.pinned_sincos_d(math.inf))


@pytest.mark.parametrize("n", [6, 7])
def test_ldlt_against_numpy_solve(n):
    rng = np.random.default_rng(7)
    for _ in range(20):
        A = rng.normal(0, 1, (n, 9))
        H = A @ A.T + 0.1 * np.eye(n)      # (test data only: the restatement never uses @)
        b = rng.normal(0, 1, n)
        lower = np.tril(H) + np.triu(np.full((n, n), np.nan), 1)   # the upper triangle is never read
        ok, x = ref.ldlt_solve(lower.tolist(), b.tolist(), [9.0] * n)
        assert ok
        want = np.linalg.solve(H, b)
        assert np.abs(np.array(x) - want).max() <= 1e-10 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("d, want_piv, want_x", [
    # diagonal 3 1 6 2 5 4: the pivots are taken in the order 6 5 4 3 2 1
    ([3.0, 1.0, 6.0, 2.0, 5.0, 4.0], [2, 4, 5, 5, 5, 5], [2.0, 5.0, 4.0 / 6.0, 1.5, 0.4, 0.25]),
    # diagonal 3 1 6 2 5 4 7: in the order 7 6 5 4 3 2 1
    ([3.0, 1.0, 6.0, 2.0, 5.0, 4.0, 7.0], [6, 2, 4, 5, 6, 5, 6],
     [7.0 / 3.0, 6.0, 5.0 / 6.0, 2.0, 0.6, 0.5, 1.0 / 7.0]),
], ids=["6", "7"])
def test_ldlt_pivot_order_and_sign(d, want_piv, want_x):
    n = len(d)
    H = [[d[i] if i == j else 0.0 for j in range(n)] for i in range(n)]
    piv = [0] * n
    ok, x = ref.ldlt_solve(H, [float(n - i) for i in range(n)], [0.0] * n, piv)
    assert ok and piv == want_piv
    assert x == want_x
    # equal magnitudes: the first one wins
    H2 = [[2.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    ref.ldlt_solve(H2, [1.0] * n, [0.0] * n, piv)
    assert piv == list(range(n))
    # a negative pivot: not positive, x keeps its previous value
    H[1][1] = -1.0
    ok, x = ref.ldlt_solve(H, [1.0] * n, [7.0] * n)
    assert not ok and x == [7.0] * n


def test_quaternion_matrix_round_trip():
    rng = np.random.default_rng(9)
    qs = [_rng_quat(rng) for _ in range(50)]
    # rotations by nearly pi about each axis take the three largest-diagonal branches
    for ax in range(3):
        v = [0.0, 0.0, 0.0, 0.02]
        v[ax] = 1.0
        qs.append(ref.normalize_rotation(v))
    branches = set()
    for q in qs:
        m = ref.quat_to_matrix(q)
        tr = m[0][0] + m[1][1] + m[2][2]
        branches.add("trace" if tr > 0 else int(np.argmax([m[0][0], m[1][1], m[2][2]])))
        q2 = ref.normalize_rotation(ref.quat_from_matrix(m))
        assert np.abs(np.array(q2) - np.array(q)).max() < 1e-14
        R = np.array(m)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14
        x, y, z = ref.quat_rotate(q, 0.3, -1.2, 2.5)
        assert np.abs(R @ [0.3, -1.2, 2.5] - [x, y, z]).max() < 1e-14
    assert branches == {"trace", 0, 1, 2}
    a, b = qs[0], qs[1]
    Rab = np.array(ref.quat_to_matrix(ref.quat_mul(a, b)))
    assert np.abs(Rab - np.array(ref.quat_to_matrix(a)) @ np.array(ref.quat_to_matrix(b))).max() < 1e-14


def test_huber_at_and_around_the_threshold():
    d = ref.DELTA_MONO
    dsqr = d * d
    e = np.array([np.nextafter(dsqr, 0), dsqr, np.nextafter(dsqr, 10), 4 * dsqr])
    r0, r1, inl = ref.huber(e, d)
    assert inl.tolist() == [True, True, False, False]
    assert r0[0] == e[0] and r1[0] == 1.0 and r0[1] == dsqr and r1[1] == 1.0
    assert r0[2] == 2 * math.sqrt(e[2]) * d - dsqr and r1[2] == d / math.sqrt(e[2])
    assert abs(r0[3] - 3 * dsqr) < 1e-12 and abs(r1[3] - 0.5) < 1e-15
    assert ref.DELTA_MONO == float(f32(math.sqrt(5.991))) != math.sqrt(5.991)


def test_stale_error_rule():
    """pop() restores the vertex, not the edges' _error: after a rejected last
    trial an active edge is classified from the error at the rejected estimate,
    a level-1 edge from the final estimate.  On a case of the shared list whose
    trace reports it, the chi2 values the classification compares are not the
    ones the final estimate gives."""
    stale = [(c, r) for c, r in pc.shared_results() if r["trace"]["stale_chi_differs"] > 0]
    assert stale
    c, r = stale[0]
    q = pc.run_ref(c, classify_from_final=True)
    assert q["trace"]["stale_chi_differs"] == 0 and r["trace"]["stale_rounds"] > 0
    # wherever the rule changes a flag, the two classifications part
    changed = [(c, r) for c, r in stale if r["trace"]["stale_changed_flags"] > 0]
    for c, r in changed:
        q = pc.run_ref(c, classify_from_final=True)
        assert (q["outlier"] != r["outlier"]).any() or q["n_inliers"] != r["n_inliers"]


# ------------------------------------------------------------------- coverage
def test_shared_list_covers_every_path():
    tr = [r["trace"] for _, r in pc.shared_results()]
    def any_(f):
        return any(f(t) for t in tr)
    assert any_(lambda t: t["rejected_trials"] > 0)
    assert any_(lambda t: t["term_qmax"] > 0 or t["term_rho0"] > 0)
    assert any_(lambda t: t["term_nbad"] > 0)
    assert any_(lambda t: t["stale_rounds"] > 0 and t["stale_chi_differs"] > 0)
    assert any_(lambda t: t["outlier_to_inlier"] > 0)
    assert any_(lambda t: t["exp_small"] > 0) and any_(lambda t: t["exp_large"] > 0)
    assert any_(lambda t: t["huber_inlier"]) and any_(lambda t: t["huber_outlier"])
    assert any_(lambda t: t["n_mono"] > 0 and t["n_stereo"] == 0)
    assert any_(lambda t: t["n_stereo"] > 0 and t["n_mono"] == 0)
    assert any_(lambda t: t["n_mono"] > 0 and t["n_stereo"] > 0)
    assert any_(lambda t: t["rounds"] == 1) and any_(lambda t: t["rounds"] == 4)


def test_libm_study_runs_and_is_recorded():
    """The libm pins measured over the shared list (tools/poseopt_libm.py writes
    the record): the figures are measurements, printed here, not fixed."""
    res = pc.libm_study()
    print(json.dumps(res))
    from conftest import ROOT
    rec = json.loads((ROOT / "profiles" / "poseopt_libm.json").read_text())
    assert set(rec) == set(res) and rec["problems"] == res["problems"] == len(pc.SHARED)
    assert all(isinstance(res[k], int) and res[k] >= 0 for k in res if k.startswith("differing"))
