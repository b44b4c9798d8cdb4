"""The directed inputs of poseopt_edge_cases.py on the CPU, on the reference
(tests/poseopt_ref.py) alone: the census of each input meets the minimum stated
next to its builder (printed, run with -s to read it); the pivot and quaternion
cases together reach all 21 (k, idx) pivot pairs and all four branches of
Quaterniond(Matrix3d); every wrong neighbour of a rule (variants=) changes the
answer of a named input, or is recorded as changing none; and the seeded list
poseopt_cases.SHARED reaches two pivot sequences and the trace branch only --
recorded in NATURAL, the reason these inputs exist.
test_gpu_poseopt_edges.py runs the same inputs through k_pose_optimization."""
import numpy as np
import pytest

import poseopt_cases as pc
import poseopt_edge_cases as E
import poseopt_ref as ref

f32 = np.float32


def _census(name):
    c, r = E.run(name)
    return E.census(c, r)


@pytest.mark.parametrize("name", list(E.CASES))
def test_census(name):
    cen = _census(name)
    print(name, {k: (sorted(v, key=str) if isinstance(v, set) else v) for k, v in cen.items()})
    E.meets(cen, E.CASES[name][1])
    assert cen["n_edges"] <= 65
    c, r = E.run(name)
    used = c["point_index"][c["point_index"] >= 0]
    assert used.max() < len(c["points"])      # no case names a point outside its array
    no_edge = c["point_index"] < 0
    assert no_edge.any() and (r["outlier"][no_edge] == pc.SENTINEL).all()


def test_pivot_and_quaternion_union():
    piv, quat = set(), set()
    for name in E.CASES:
        cen = _census(name)
        if name in E.PIVOT_CASES:
            piv |= cen["pivots"]
        if name in E.PIVOT_CASES or name.startswith("quat_"):
            quat |= cen["quat_start"] | cen["quat_step"]
    print("pivot pairs", sorted(piv), "quaternion branches", sorted(quat, key=str))
    assert piv == E.ALL_PIVOTS and len(piv) == 21
    assert quat == {"trace", 0, 1, 2}
    kinds = {(c["n_mono"] > 0, c["n_stereo"] > 0) for c in map(_census, E.PIVOT_CASES)}
    assert kinds == {(True, False), (False, True), (True, True)}   # mono, stereo and mixed
    # the first pivot is index 0 (no swap at k = 0) in solves of some, and is not in others
    first = [{i for k, i in _census(n)["pivots"] if k == 0} for n in E.PIVOT_CASES]
    assert any(0 in f for f in first) and any(0 not in f for f in first)


def test_directed_census_table():
    """The figures of DESIGN.md 4.5, printed: what all directed cases reach."""
    tot = dict(pivots=set(), quat_start=set(), quat_step=set(), flips=set(), quadrants=set(),
               ended=set(), skipped=0, not_positive=0, stale_changed_flags=0, outlier_to_inlier=0)
    for name in E.CASES:
        cen = _census(name)
        for k in ("pivots", "quat_start", "quat_step", "flips", "quadrants"):
            tot[k] |= cen[k]
        tot["ended"] |= set(cen["ended"])
        tot["skipped"] += len(cen["skipped_rounds"])
        for k in ("not_positive", "stale_changed_flags", "outlier_to_inlier"):
            tot[k] += cen[k]
    print({k: (sorted(v, key=str) if isinstance(v, set) else v) for k, v in tot.items()})
    assert len(tot["pivots"]) == 21 and tot["quadrants"] == {0, 1, 2, 3}
    assert tot["quat_step"] == {"trace", 0, 1, 2} and tot["flips"] == {"start", "exp", "mul"}
    assert tot["ended"] == {"iterations", "qmax", "rho0", "nbad"}
    assert tot["skipped"] and tot["not_positive"] and tot["stale_changed_flags"]


# What the 45 seeded problems of poseopt_cases.SHARED reach: the reason the
# directed cases exist.  Two pivot sequences, which differ in the last swap: 2 of
# the 15 swap branches of g2o_ldlt_solve, never the no-swap path at k = 0; the
# trace branch of Quaterniond(Matrix3d) only, no sign flip, quadrant 0 only.
NATURAL = dict(pivot_sequences=[(1, 1, 2, 3, 4, 5), (1, 1, 2, 3, 5, 5)],
               pivots=[(0, 1), (1, 1), (2, 2), (3, 3), (4, 4), (4, 5), (5, 5)],
               quat_start=["trace"], quat_step=["trace"], flips=[], quadrants=[0],
               skipped_rounds=0, not_positive=0)


def test_shared_list_reaches_little():
    tot = dict(pivots=set(), pivot_sequences=set(), quat_start=set(), quat_step=set(), flips=set(),
               quadrants=set())
    skipped = notpos = 0
    for _, r in pc.shared_results():
        t = r["trace"]
        for k in tot:
            tot[k] |= t[k]
        skipped += len(t["skipped_rounds"])
        notpos += t["not_positive"]
    print({k: sorted(v, key=str) for k, v in tot.items()}, skipped, notpos)
    for k in tot:
        assert sorted(tot[k], key=str) == NATURAL[k], k
    assert sum(1 for k, i in tot["pivots"] if i != k) == 2      # swap branches, of 15
    assert skipped == NATURAL["skipped_rounds"] and notpos == NATURAL["not_positive"]


# ------------------------------------------------------------ the traced rules
def test_symmetric_cases_stay_at_the_start():
    """b is exactly zero, so the step is zero, rho is 0 and the estimate stays:
    every chi2 is the chosen number, in every round."""
    for name in ("sym_thresholds", "sym_huber_exact"):
        c, r = E.run(name)
        t = r["trace"]
        assert t["ended"] == ["rho0"] * 4 and t["max_theta"] == 0.0 and t["exp_small"] == 4
        assert r["rcw"].tobytes() == c["pose"]["rcw"][0].tobytes() and not r["tcw"].any()
        assert len(set(t["round_outliers"])) == 1
        want = np.repeat([f32(d * (float(f32(s)) * d)) for _, d, s in c["pairs"]], 2)
        assert t["chi2_first"].tobytes() == want.astype(f32).tobytes()


def test_threshold_edges_sit_where_they_are_named():
    t = E.threshold_edges()
    print(t)
    up = lambda v: np.nextafter(v, f32(np.inf))
    assert f32(t["mono_at"][2]) == ref.CHI2_MONO and f32(t["mono_above"][2]) == up(ref.CHI2_MONO)
    assert f32(t["stereo_at"][2]) == ref.CHI2_STEREO
    assert f32(t["stereo_above"][2]) == up(ref.CHI2_STEREO)
    c, r = E.run("sym_thresholds")
    flags = r["outlier"][c["slots"]].reshape(-1, 2)
    # at: inlier under >; a float above: outlier; the Huber pairs lie below both thresholds
    # (mono) or above (stereo: delta^2 = 7.8150004 narrows to the float above 7.815f)
    assert flags.tolist() == [[0, 0], [1, 1], [0, 0], [1, 1], [0, 0], [0, 0], [1, 1], [1, 1]]
    for kind, delta in (("mono", ref.DELTA_MONO), ("stereo", ref.DELTA_STEREO)):
        lo, hi = t["huber_%s_le" % kind][2], t["huber_%s_gt" % kind][2]
        dsqr = delta * delta
        assert lo <= dsqr < hi
        # the closest the float32 inputs allow.  The grid holds 32,768 offsets x 7
        # weights per width, whose chi2 values fill about 7 ulp(s) d^2 = 3e-6: a mean
        # spacing of 1.3e-11, 2^-39 of delta^2.  Eight spacings is the bound.
        assert (dsqr - lo) / dsqr < 2.0 ** -36 and (hi - dsqr) / dsqr < 2.0 ** -36
        r0, r1, inl = ref.huber(np.array([lo, hi]), delta)
        assert inl.tolist() == [True, False] and r1[0] == 1.0 and r1[1] < 1.0
    # the equality itself, at principal point (0, 0)
    c, r = E.run("sym_huber_exact")
    assert r["trace"]["chi2_first"][0] == f32(ref.DELTA_MONO ** 2)
    assert float(f32(ref.DELTA_MONO)) * float(f32(ref.DELTA_MONO)) == ref.DELTA_MONO ** 2


def test_flag_cases_are_classified_as_named():
    c, r = E.run("flag_zeros")
    ur = c["u_right"][c["flag_slots"]]
    assert ur.view(np.uint32).tolist() == [0, 0x80000000, 0x80000001, 0xBF800000, 1]
    with np.errstate(invalid="ignore"):
        assert (~(ur < 0)).tolist() == [True, True, False, False, True]
    # three of the five were stereo before: the counts moved by the two monos
    base = E.synth(300, 14, "mixed", noise=0.5, outlier_frac=0.0)
    was = int((~(base["u_right"][c["flag_slots"]] < 0)).sum())
    assert r["trace"]["n_stereo"] == int((~(base["u_right"][base["slots"]] < 0)).sum()) - was + 3
    c, r = E.run("flag_nan")
    assert np.isnan(c["u_right"][c["flag_slots"][0]]) and r["trace"]["n_stereo"] == 11


def test_level_tables():
    for n in (1, 3, 16):
        c, r = E.run("levels_%d" % n)
        oct_ = c["keys"]["octave"][c["slots"]]
        assert len(c["levels"]) == n and oct_.max() == n - 1 and r["n_edges"] == 16
        if n >= 3:
            used = c["levels"][oct_]
            assert (used == 0).any() and (used == E.POS_DENORMAL).any()
        c, r = E.run("levels_%d_bad_octave" % n)
        assert (c["keys"]["octave"][c["slots"]] == n).sum() == 1
        assert r["n_edges"] == -1 and (r["outlier"] == pc.SENTINEL).all()
        assert r["rcw"].tobytes() == c["pose"]["rcw"][0].tobytes()


def test_all_outliers_counts_round_one_only():
    c, r = E.run("all_outliers_after_round1")
    t = r["trace"]
    assert t["round_outliers"][0] == tuple(range(r["n_edges"])) and t["rounds"] == 4
    assert r["lm_iterations"] == t["lm_iterations"] == 8 and len(t["ended"]) == 1
    # the estimate of the skipped rounds is the start pose again (:397)
    start = ref.pose_from_se3quat(ref.to_se3quat(c["pose"]["rcw"][0], c["pose"]["tcw"][0]))
    assert r["rcw"].tobytes() == start[0].tobytes() and r["tcw"].tobytes() == start[1].tobytes()


def test_not_positive_is_reached_only_by_a_negative_weight():
    c, r = E.run("negative_level_weight")
    assert (c["levels"] < 0).sum() == 1 and r["trace"]["not_positive"] > 0
    for name in E.CASES:
        if name != "negative_level_weight":
            assert _census(name)["not_positive"] == 0, name


# -------------------------------------------------------------- wrong neighbours
# variant -> the cases it must change (float32 outputs or info).  An empty tuple
# records a neighbour that no input of this file separates.
SENSITIVITY = {
    "classify_ge": ("sym_thresholds",),
    # e == delta^2 is reached (sym_huber_exact), but there both branches of
    # robustify give rho = (e, 1) bit for bit: sqrt(e) == delta, so
    # 2 sqrt(e) delta - delta^2 == e and delta / sqrt(e) == 1.  Off the equality
    # the two rules agree.  No input can separate them.
    "huber_lt": (),
    "stereo_le": ("flag_zeros",),
    "tie_last": ("pivots_tie_143",),
    "no_pivot": ("pivots_needed_17",),
    "three_edges": ("three_edges",),
    "ten_edges": ("term_qmax", "term_rho0", "pivots_581"),     # the ten-edge problems
    "classify_from_final": ("stale_flags_inf_observation",),
}


def _differs(a, b):
    same = all(a[k].tobytes() == b[k].tobytes() for k in ("rcw", "tcw", "ow", "outlier"))
    return not same or any(a[k] != b[k] for k in ("n_inliers", "n_edges", "lm_iterations",
                                                  "rejected_trials"))


@pytest.mark.parametrize("variant", list(SENSITIVITY))
def test_sensitivity(variant):
    names = SENSITIVITY[variant]
    changed = [n for n in E.CASES if _differs(E.run(n)[1], pc.run_ref(E.run(n)[0], variants=(variant,)))]
    print(variant, "changes", changed if changed else "no case")
    for n in names:
        assert n in changed, (variant, n)
    if not names:
        assert not changed, (variant, changed)     # recorded as separating nothing: keep it true


@pytest.mark.parametrize("k,c", [(k, c) for k in range(6) for c in range(k + 1, 6)])
def test_every_swap_branch_decides_a_result(k, c):
    """Reaching a (k, c) swap is not enough: a swap of that one pair gone wrong
    (the two diagonal entries left in place) must change the float32 outputs or
    the info of a pivot case, or a wrong index there would still pass."""
    v = "half_swap_%d%d" % (k, c)
    changed = [n for n in E.PIVOT_CASES if (k, c) in _census(n)["pivots"]
               and _differs(E.run(n)[1], pc.run_ref(E.run(n)[0], variants=(v,)))]
    print(v, "changes", changed)
    assert changed
