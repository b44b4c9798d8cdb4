"""tests/sim3opt_ref.py on tests/sim3opt_cases.py (CPU): the cases reach what
they are named for (census minimums from the reference's trace), noise-free
problems keep every correspondence, each wrong neighbour of the restatement
changes a named case's output, and pinned_exp is fdlibm's exp."""
import math

import numpy as np
import pytest

import sim3opt_cases as C
import sim3opt_ref as R

_cases, _refs = C.all_cases(), {}


def ref_of(name):
    if name not in _refs:
        _refs[name] = C.run_ref(_cases[name])
    return _refs[name]


def key(r):
    return (r["status"], r["n_corr"], r["n_bad"], r["n_inliers"], r["q"].tobytes(), r["t"].tobytes(),
            np.float64(r["s"]).tobytes(), r["R"].tobytes(), r["match12"].tobytes())


# ------------------------------------------------------------------- census
@pytest.mark.parametrize("name,left,bad", [
    ("gate0_clean", 0, False), ("gate1_clean", 1, False), ("gate9_clean", 9, False),
    ("gate10_clean", 10, False), ("gate11_clean", 11, False), ("z0_point", 0, True),
    ("gate1_bad", 1, True), ("gate9_bad", 9, True), ("gate10_bad", 10, True),
    ("gate11_bad", 11, True)])
def test_gate_cases(name, left, bad):
    """nCorrespondences - nBad on both sides of 10, with nBad == 0 (5 more
    iterations) and nBad > 0 (10 more)."""
    r = ref_of(name)
    t = r["trace"]
    assert r["status"] == 0 and r["n_corr"] - r["n_bad"] == left and (r["n_bad"] > 0) == bad
    if left < 10:
        assert t["gate"] == "early" and r["n_inliers"] == 0
        assert r["s"] == float(np.float32(_cases[name]["start"][2]))  # g2oS12 is not assigned
        assert len(t["iterations"]) == (1 if r["n_corr"] else 0)
    else:
        assert t["gate"] == ("second_10" if bad else "second_5") and len(t["iterations"]) == 2
        assert r["n_inliers"] > 0
    # the first check's removals are stored whichever way the gate goes
    assert int((r["match12"][:_cases[name]["n1"]] < 0).sum()) >= \
        int((np.asarray(_cases[name]["match12"])[:_cases[name]["n1"]] < 0).sum()) + r["n_bad"]


@pytest.mark.parametrize("n", [32, 33, 64, 65, 129])
def test_pair_counts(n):
    r = ref_of("pairs%d" % n)
    assert r["n_corr"] == n and r["n_bad"] > 0 and r["trace"]["gate"] == "second_10"


def test_skip_rules_and_malformed():
    r = ref_of("skips")
    sk = r["trace"]["skipped"]
    assert sk["null_mp1"] == 1 and sk["bad"] == 2 and sk["i2_negative"] == 2 and sk["null_match"] >= 1
    assert r["n_corr"] == 40 - 6 and r["status"] == 0
    for name in ("bad_i2", "bad_i2_big", "bad_oct1", "bad_oct1_neg", "bad_oct2", "bad_oct2_neg"):
        m = ref_of(name)
        assert m["status"] == -1 and m["n_corr"] == m["n_bad"] == m["n_inliers"] == 0, name
        assert np.array_equal(m["match12"], _cases[name]["match12"]), name
    assert ref_of("bad_oct_skipped")["status"] == 0 and ref_of("bad_oct_skipped")["n_corr"] == 29
    assert ref_of("junk")["n_corr"] == 40


def test_exp_and_quaternion_branches():
    """(|sigma| < eps, theta < eps) per LM step, and Quaterniond(Matrix3d)'s
    branches from the start value."""
    assert ref_of("start_exact")["trace"]["exp_step"] == {(True, True)}
    assert (True, False) in ref_of("fix50")["trace"]["exp_step"]
    assert (False, True) in ref_of("start_scale_only")["trace"]["exp_step"]
    assert (False, False) in ref_of("start_far")["trace"]["exp_step"]
    steps, perturb, start, inside = set(), set(), set(), set()
    for n in _cases:
        t = ref_of(n)["trace"]
        steps |= t["exp_step"]
        perturb |= t["exp_perturb"]
        start |= t["quat_start"]
        inside |= t["quat_step"] | t["quat_perturb"]
    assert steps == {(a, b) for a in (False, True) for b in (False, True)}
    assert perturb == {(True, True)}  # +-1e-9 always takes the (small, small) branch
    assert ref_of("quat_x")["trace"]["quat_start"] == {0}
    assert ref_of("quat_y")["trace"]["quat_start"] == {1}
    assert ref_of("quat_z")["trace"]["quat_start"] == {2}
    assert start == {"trace", 0, 1, 2}
    # inside exp, in LM steps: the trace branch and each largest-diagonal branch
    # (the first is what the NaN steps take, the other two need a step near
    # half a turn: quat_exp_y, quat_exp_z)
    assert 1 in ref_of("quat_exp_y")["trace"]["quat_step"]
    assert 2 in ref_of("quat_exp_z")["trace"]["quat_step"]
    assert 0 in ref_of("nan_point")["trace"]["quat_step"]
    for name in ("quat_exp_y", "quat_exp_z"):
        r = ref_of(name)
        assert r["status"] == 0 and np.isfinite(r["q"]).all() and np.isfinite(r["t"]).all()
    assert inside == {"trace", 0, 1, 2}


def test_lm_census():
    ended, pivots, rej, stale, np_, hub_in, hub_out, its2 = set(), set(), 0, 0, 0, False, False, set()
    for n in _cases:
        t = ref_of(n)["trace"]
        ended |= set(t["ended"])
        pivots |= t["pivots"]
        rej += t["rejected_trials"]
        stale += t["stale_rounds"]
        np_ += t["not_positive"]
        hub_in |= t["huber_inlier"]
        hub_out |= t["huber_outlier"]
        if t["gate"] and t["gate"].startswith("second"):
            its2.add(t["gate"])
    assert ended == {"iterations", "nbad", "rho0", "qmax"}  # every termination rule
    assert its2 == {"second_5", "second_10"}
    assert rej > 50 and stale >= 5 and hub_in and hub_out
    assert pivots == {(k, i) for k in range(7) for i in range(k, 7)}  # all 28 (k, idx) pairs
    for name, pair in (("pivot_14", (1, 4)), ("pivot_03", (0, 3)), ("pivot_04", (0, 4)),
                       ("pivot_02", (0, 2)), ("quat_exp_z", (1, 2))):
        assert pair in ref_of(name)["trace"]["pivots"], name
    assert ref_of("neg_all")["trace"]["not_positive"] >= 10 and ref_of("neg_level0")["trace"]["not_positive"] > 0
    assert np_ >= 20


def test_exact_thresholds():
    """Host "flat": chi2 == th2 (== delta^2) stays, the double above it goes."""
    c, r = _cases["threshold"], ref_of("threshold")
    assert r["trace"]["ended"] == ["rho0", "rho0"] and r["trace"]["iterations"] == [1, 1]
    assert r["n_corr"] == 12 and r["n_bad"] == 1 and r["n_inliers"] == 11
    gone = np.nonzero((r["match12"] < 0) & (c["match12"] >= 0))[0]
    assert list(gone) == [6] and c["keys1"][6, 1] == np.float32(0.5) + np.float32(2.0 ** -24)
    assert c["keys1"][5, 0] == 5.0 and c["keys1"][5, 1] == 0.5  # chi2 = 16 exactly: kept
    assert np.array_equal(r["q"], [0.0, 0.0, 0.0, 1.0]) and r["s"] == 1.0
    g = ref_of("threshold_gate")
    assert g["n_corr"] == 11 and g["n_bad"] == 1 and g["n_inliers"] == 10


def test_nan_inf_and_zero_inputs_end():
    for name in ("nan_point", "inf_point", "nan_key", "nan_start", "inf_scale", "zero_scale", "z0_point"):
        r = ref_of(name)
        assert r["status"] == 0 and sum(r["trace"]["iterations"]) <= 15, name


# --------------------------------------------------------------- noise-free
@pytest.mark.parametrize("name", sorted(C.noise_free()))
def test_noise_free_keeps_every_correspondence(name):
    r = ref_of(name)
    assert r["n_inliers"] == r["n_corr"] > 0 and r["n_bad"] == 0
    first, second = r["trace"]["final_chi2"]
    assert second <= first


# ---------------------------------------------------------- wrong neighbours
@pytest.mark.parametrize("variant,name", [
    ("unary_assoc", "nat30"), ("forward_diff", "nat75"), ("normalize_quat", "gate1_clean"),
    ("chi2_float", "threshold"), ("classify_from_final", "nan_point"), ("e21_first", "clean40")])
def test_wrong_neighbour_changes_the_output(variant, name):
    assert key(C.run_ref(_cases[name], variants=(variant,))) != key(ref_of(name))


@pytest.mark.parametrize("variant", ["huber_lt", "tie_last"])
def test_neighbours_that_cannot_change_the_output(variant):
    """Recorded: no case separates these two from the reference.
    huber_lt: at chi2 == delta^2 both branches give rho0 = delta^2 and rho1 = 1
    bit for bit wherever sqrt(delta^2) == delta ("threshold" has chi2 == 16 ==
    delta^2), so < and <= cannot differ.  tie_last: two of the seven remaining
    |diagonal| entries of H + lambda I would have to be equal doubles; the
    census counts no such step on any case but the all-zero H of host "flat",
    whose solve returns 0 whichever pivot is taken."""
    for name in _cases:
        assert key(C.run_ref(_cases[name], variants=(variant,))) == key(ref_of(name)), name


# ------------------------------------------------------------------ pinned_exp
def test_pinned_exp_is_fdlibm_exp():
    """Special values exactly; elsewhere within one ulp of the platform's exp
    (the count over the arguments the cases reach is reported, not asserted)."""
    assert R.pinned_exp(0.0) == 1.0 and R.pinned_exp(-0.0) == 1.0
    assert R.pinned_exp(math.inf) == math.inf and R.pinned_exp(-math.inf) == 0.0
    assert math.isnan(R.pinned_exp(math.nan))
    assert R.pinned_exp(710.0) == math.inf and R.pinned_exp(-746.0) == 0.0
    assert R.pinned_exp(709.782712893384) == math.exp(709.782712893384)
    assert R.pinned_exp(1e-9) == 1.0 + 1e-9 and R.pinned_exp(-1e-9) == 1.0 - 1e-9
    assert R.pinned_exp(-745.0) == 5e-324
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.uniform(-745, 709, 3000), rng.uniform(-1.5, 1.5, 3000),
                         rng.standard_normal(1000) * 1e-4])
    for x in xs:
        a, b = R.pinned_exp(float(x)), math.exp(float(x))
        assert abs(R._bits(a) - R._bits(b)) <= 1, x
    reached = set()
    for n in _cases:
        reached |= ref_of(n)["trace"]["exp_args"]
    fin = [R._from_bits(b) for b in reached if math.isfinite(R._from_bits(b))]
    differ = sum(R._bits(R.pinned_exp(x)) != R._bits(math.exp(x)) for x in fin)
    print(f"pinned_exp vs math.exp over the {len(fin)} finite arguments the cases reach: {differ} differ")
    assert len(fin) > 100
