"""tests/sim3_ref.py (the parity target of the Sim3Solver device batch) checked
on its own: hand-checkable answers, the Jacobi pin's results, the census of
tests/sim3_cases.py, the rule switches, the iteration-count formula and the
pinned functions against libm."""
import math

import numpy as np
import pytest

import sim3_cases as C
import sim3_ref as R

f32 = np.float32
EPS = float(np.finfo(np.float32).eps)


def answer(s, n=None):
    """Everything a caller can see after iterate(n) (find() when n is None)."""
    T, no_more, vb, n_in = s.iterate(s.mRansacMaxIts if n is None else n)
    return (s.state_record().tobytes(), s.corr_records().tobytes(),
            s.result_record(T, no_more, n_in).tobytes(), vb.tobytes())


# ------------------------------------------------------- hand-checkable answers
@pytest.mark.parametrize("fix", [False, True])
def test_noise_free_all_inliers_of_the_first_hypothesis(fix):
    p = C.make_problem("clean", 11, n_corr=50, n_outliers=0, fix_scale=fix, scale=1.0,
                       plan=("g",))
    s = p.solver()
    assert s.N == 50
    T, no_more, vb, n_in = s.iterate(5)
    assert T is not None and not no_more and s.mnIterations == 1 and s.iterations_run == 1
    assert n_in == 50 and s.mvbBestInliers.all()
    assert np.array_equal(np.nonzero(vb)[0], s.mvnIndices1)
    if fix:
        assert s.GetEstimatedScale().tobytes() == f32(1.0).tobytes()  # exactly 1.0f
    else:
        assert abs(float(s.GetEstimatedScale()) - 1.0) < 1e-5
    # the similarity the data was built with: X1 = R X2 + t
    assert np.allclose(s.GetEstimatedRotation(), C.rot(0.3, -0.2, 0.1), atol=1e-5)
    assert np.allclose(s.GetEstimatedTranslation(), [0.5, -0.3, 0.2], atol=1e-4)
    assert np.array_equal(s.mBestT12[3], [0, 0, 0, 1])


def test_scaled_similarity_recovered():
    p = C.directed()["free_scale"]
    s = p.solver()
    T, vb, n = s.find()
    assert T is not None and abs(float(s.GetEstimatedScale()) - 1.3) < 1e-4


# ------------------------------------------------------------- the Jacobi pin
def _sym4(rng, scale):
    a = rng.normal(0, scale, (4, 4))
    return ((a + a.T) / 2).astype(f32)


@pytest.mark.parametrize("scale", [1e-3, 1.0, 50.0, 1e4])
def test_jacobi_eigenpairs(scale):
    """N v = lambda v, orthonormal rows, descending values.  Tolerances: a
    rotation perturbs the matrix by a few float epsilons of its norm, the pin
    stops once the pivot is <= FLT_EPSILON (absolute), and at most 480 rotations
    run, of which a 4 x 4 matrix needs about a dozen: 64 eps ||N||_F + 4 eps for
    the residual, 64 eps for V V^T - I."""
    rng = np.random.default_rng(int(scale * 1000) % 97)
    for _ in range(20):
        N = _sym4(rng, scale)
        W, V, sweeps = R.jacobi_eigen4(N)
        W = np.array(W, np.float64)
        V = np.array(V, np.float64)
        Nd = N.astype(np.float64)
        norm = math.sqrt(float((Nd * Nd).sum()))
        assert sweeps < 40
        assert all(W[i] >= W[i + 1] for i in range(3))
        for k in range(4):
            resid = Nd @ V[k] - W[k] * V[k]
            assert np.abs(resid).max() <= 64 * EPS * norm + 4 * EPS
        assert np.abs(V @ V.T - np.eye(4)).max() <= 64 * EPS


def test_jacobi_diagonal_and_quaternion_row():
    W, V, sweeps = R.jacobi_eigen4(np.diag([1.0, 4.0, 2.0, 3.0]).astype(f32))
    assert sweeps == 0 and [float(w) for w in W] == [4.0, 3.0, 2.0, 1.0]
    assert [[float(v) for v in row] for row in V] == [[0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0],
                                                      [1, 0, 0, 0]]


def test_rodrigues_and_atan2_against_libm():
    rng = np.random.default_rng(2)
    worst = 0.0
    for _ in range(2000):
        y, x = rng.normal(0, 1), rng.normal(0, 1)
        a, b = R.pinned_atan2(abs(y), x), math.atan2(abs(y), x)
        worst = max(worst, abs(a - b) / max(abs(b), 1e-300))
    assert worst <= 4 * np.finfo(np.float64).eps  # fdlibm's atan2 is < 1 ulp, libm's too
    assert R.pinned_atan2(0.0, 1.0) == 0.0 and R.pinned_atan2(0.0, -1.0) == math.pi
    for x in (0.013, 0.3, 0.5, 0.99, 1e-9, 0.75, 1 - 2 ** -20):
        assert abs(R.pinned_log(x) - math.log(x)) <= 2 * np.finfo(np.float64).eps * abs(math.log(x))
    Rm = np.array(R.rodrigues([f32(0.3), f32(-0.2), f32(0.1)]), np.float64)
    assert np.allclose(Rm, C.rot(float(f32(0.3)), float(f32(-0.2)), float(f32(0.1))), atol=1e-7)
    assert np.array_equal(np.array(R.rodrigues([f32(0)] * 3)), np.eye(3, dtype=f32))


# ------------------------------------------------------------------ the census
def test_census():
    """Each condition the GPU test lists occurs in the directed inputs."""
    D = C.directed()
    tags = set().union(*(p.tags for p in D.values()))
    for n in (19, 20, 21, 63, 64, 65, 80, 81, 200):
        assert D[f"n{n}"].solver().N == n
    assert D["full_stride"].solver().N == C.STRIDE and "N=stride" in tags
    # the cap of max_iterations is reached from N = 81
    assert D["n80"].solver().mRansacMaxIts < 300 and D["n81"].solver().mRansacMaxIts == 300
    assert D["n19"].solver().mRansacMaxIts == 0 and D["n20"].solver().mRansacMaxIts == 1
    # skips: the skipped slots hold a match the constructor drops, each kind alone
    for kind in ("null_match", "null_mp1", "bad1", "bad2", "neg1", "neg2"):
        p = D[f"skip_{kind}"]
        s = p.solver()
        assert s.N == 40 and s.status == 0
        n_slots = s.mN1 - 5  # all but the unmatched ones
        assert n_slots == 43
        if kind != "null_match":
            assert np.count_nonzero(p.match12[:s.mN1] >= 0) == 43
        else:
            assert np.count_nonzero(p.match12[:s.mN1] == -7) == 3
    s = D["skip_all"].solver()
    assert s.N == 40 and s.status == 0 and s.mN1 == 52
    assert s.mvnIndices1[0] != 0  # compact position != i1
    # where the success falls
    for name, at in (("first_of_chunk", C.CHUNK + 1), ("last_of_chunk", C.CHUNK),
                     ("last_of_window", 5)):
        s = D[name].solver()
        T, _, _ = s.find()
        assert T is not None and s.mnIterations == at
    s = D["at_max_its"].solver()
    T, no_more, _, _ = s.iterate(300)
    assert T is not None and not no_more and s.mnIterations == s.mRansacMaxIts > 1
    T, no_more, vb, n = s.iterate(5)
    assert T is None and no_more and s.iterations_run == 0 and not vb.any()
    # ties
    s = D["tie"].solver()
    s.iterate(1)
    b1 = s.mnBestInliers
    s.iterate(1)
    assert s.mnBestInliers == b1 and s.best_iteration == 2 and 0 < b1 <= 20
    # degenerate samples
    s = D["identical"].solver()
    s.iterate(1)
    assert math.isnan(float(s.ms12i)) and s.mnInliersi == 0  # den = 0
    s = D["collinear"].solver()
    s.iterate(1)
    X = s.mvX3Dc2[:3].astype(np.float64)
    assert np.linalg.matrix_rank(X - X.mean(0), tol=1e-5) == 1
    s = D["zero_rotation"].solver()
    s.iterate(1)
    assert all(math.isnan(float(v)) for row in s.mR12i for v in row)  # vec / 0
    s = D["z_zero"].solver()
    assert not np.isfinite(s.mvP1im1).all() and (s.mvX3Dc1[:, 2] == 0).sum() == 1
    assert D["fix_scale"].fix_scale and not D["free_scale"].fix_scale
    for name in ("identical", "collinear", "zero_rotation", "z_zero"):  # both fix_scale settings
        assert D[name + "_fix"].fix_scale and not D[name].fix_scale
        a, b = D[name].solver(), D[name + "_fix"].solver()
        a.iterate(1)
        b.iterate(1)
        assert b.ms12i.tobytes() == f32(1).tobytes() and a.N == b.N == 40
    # the draws: a repeated position, another rand_max
    s = D["repeat_position"].solver()
    assert R.random_int(int(s.draws[0]), s.rand_max, 40) == 0
    assert R.random_int(int(s.draws[1]), s.rand_max, 39) == 0
    assert D["small_rand_max"].rand_max == 32767 and D["small_rand_max"].index1 is not None
    for kind, p in C.malformed().items():
        s = p.solver()
        if kind == "draw_big":
            assert s.status == 0
            s.iterate(5)
            assert s.status == -1 and s.mnIterations == 1
        else:
            assert s.status == -1 and s.N == 0
    assert {"exhaust", "tie", "threshold:truncated"} <= tags
    s = D["exhaust"].solver()
    T, _, _ = s.find()
    assert T is None and s.mnIterations == s.mRansacMaxIts


# ------------------------------------------------------------- rule switches
@pytest.mark.parametrize("switch,name", [
    ("best_gt", "tie"),                   # > for >= on the best
    ("min_ge", "n20"),                    # >= for > on min_inliers
    ("thr_double", "borderline"),         # thresholds left as doubles
    ("draw_replace", "repeat_position"),  # draws with replacement
    ("inliers_compact", "skip_all"),      # vbInliers indexed by compact position
    ("nomore_on_success", "at_max_its"),  # bNoMore set on a success at the last iteration
    ("ignore_fix_scale", "fix_scale_wrong"),  # fix_scale ignored
    ("skip_order", "skip_all"),           # the skip order in the constructor
])
def test_rule_switch_changes_the_answer(switch, name):
    p = C.directed()[name]
    assert answer(p.solver()) == answer(p.solver())
    assert answer(p.solver(switch=switch)) != answer(p.solver())


def test_switch_details():
    D = C.directed()
    # count == min_inliers: the strict comparison never returns
    s = D["n20"].solver()
    T, _, _ = s.find()
    assert T is None and s.mnBestInliers == 20
    assert D["n20"].solver(switch="min_ge").find()[0] is not None
    # one correspondence between the truncated bound 9 and 9.21
    s = D["borderline"].solver()
    T, _, _ = s.find()
    assert T is None and s.mnBestInliers == 20
    s = D["borderline"].solver(switch="thr_double")
    T, _, n = s.find()
    assert T is not None and n == 21
    assert float(R.max_error(f32(1.0))) == 9.0 and float(R.max_error(f32(1.44))) == 13.0


# --------------------------------------------------- the iteration-count formula
def test_iteration_count_formula(orb):
    top = orb.sim3_solver_max_stride()
    assert top >= 2048
    closest = 1.0
    for N in range(20, top + 1):
        a = R.ransac_iterations(N, 0.99, 20, 300)
        b = R.ransac_iterations(N, 0.99, 20, 300, libm=True)
        assert a == b, N
        if N > 20:
            e = float(f32(20) / f32(N))
            q = math.log(1.0 - 0.99) / math.log(1.0 - math.pow(e, 3))
            assert (a == 300) == (math.ceil(q) >= 300)
            if q < 300:  # beyond the cap the quotient's fraction decides nothing
                closest = min(closest, abs(q - round(q)) / q)
    assert R.ransac_iterations(20, 0.99, 20, 300) == 1
    assert R.ransac_iterations(80, 0.99, 20, 300) < 300 == R.ransac_iterations(81, 0.99, 20, 300)
    assert closest > 1e-5  # (2.9e-5 at N = 58) a last-bit difference in log cannot move the count


# ------------------------------------------------------------ pinned vs libm
def test_pinned_and_libm_select_the_same(capsys):
    worst = 0.0
    for name, p in C.directed().items():
        a, b = p.solver(), p.solver(libm=True)
        Ta, va, na = a.find()
        Tb, vb, nb = b.find()
        assert (Ta is None) == (Tb is None), name
        assert a.mnIterations == b.mnIterations and a.best_iteration == b.best_iteration, name
        assert na == nb and np.array_equal(va, vb), name
        assert np.array_equal(a.mvbBestInliers, b.mvbBestInliers), name
        ta, tb = np.asarray(a.mBestT12, np.float64), np.asarray(b.mBestT12, np.float64)
        if np.isfinite(ta).all() and np.isfinite(tb).all():
            worst = max(worst, float(np.abs(ta - tb).max()))
    with capsys.disabled():
        print(f"\nsim3 pinned vs libm: largest |T12 difference| = {worst:.3e}")
