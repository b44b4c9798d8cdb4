"""tests/newpoints_ref.py, the restatement of LocalMapping::CreateNewMapPoints'
gate and loop body that the device batch is compared with: the census of
tests/newpoints_cases.py (every claim of a case's tags checked against the
restatement's traces), wrong neighbours of the reference's rules, libm against
the pinned functions, and the restated Jacobi SVD against numpy."""
import collections

import numpy as np
import pytest

import newpoints_cases as C
import newpoints_ref as R

f32 = np.float32


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in C.all_cases()}


def adjacent(a, b):
    return abs(R.f32_bits(a) - R.f32_bits(b)) == 1


def test_census_minimums(cases):
    status = collections.Counter()
    branch = collections.Counter()
    beta = collections.Counter()
    for c in cases.values():
        r = c.ref()
        n1 = len(c.match12)
        if not r["info"]["overflow"]:
            status.update(int(s) for s in r["status"][:n1])
        for t in c.traces():
            branch[t.get("branch")] += 1
            beta["neg"] += t.get("beta_neg", 0)
            beta["pos"] += t.get("beta_pos", 0)
    print("status census:", {R.STATUS_NAMES[k]: v for k, v in sorted(status.items())})
    print("branch census:", dict(branch), "beta signs:", dict(beta))
    for code in range(R.NSTATUS):          # every status code is reached
        assert status[code] >= 1, R.STATUS_NAMES[code]
    assert status[R.ACCEPTED] >= 500 and status[R.UNDEFINED] >= 5
    assert branch["tri"] >= 500 and branch["st1"] >= 3 and branch["st2"] >= 3   # all three branches
    assert beta["neg"] >= 100 and beta["pos"] >= 100                       # both beta signs
    nat = [c for c in cases.values() if "natural" in c.tags]
    assert sum(c.monocular for c in nat) >= 2 and sum(not c.monocular for c in nat) >= 2
    assert all(100 <= int((c.match12 >= 0).sum()) <= 300 for c in nat)


def test_directed_cases_sit_on_their_thresholds(cases):
    T = lambda name: cases[name].traces()
    S = lambda name: [int(s) for s in cases[name].ref()["status"]]
    # cosParallaxRays on both sides of 0.9998, from adjacent inputs
    t = T("low_parallax_edge")
    k2 = cases["low_parallax_edge"].kf2["keys"]["x"]
    assert adjacent(k2[0], k2[1]) and sorted(S("low_parallax_edge")) == [R.ACCEPTED, R.LOW_PARALLAX]
    lo, hi = sorted(float(x["cos_rays"]) for x in t)
    assert lo < 0.9998 <= hi and adjacent(f32(lo), f32(hi))
    # coincident rays: no parallax at all
    assert all(float(x["cos_rays"]) == 1.0 for x in T("coincident_rays"))
    assert S("coincident_rays") == [R.LOW_PARALLAX, R.ACCEPTED]
    # cosParallaxRays == 0 and the float above
    t = T("rays_zero")
    assert float(t[0]["cos_rays"]) == 0.0 < float(t[1]["cos_rays"]) < 1e-6
    assert S("rays_zero")[0] == R.LOW_PARALLAX != S("rays_zero")[1]
    k1 = cases["rays_zero"].kf1["keys"]["x"]
    assert adjacent(k1[0], k1[1])
    # z1, z2 == 0 exactly and one float above
    for z, st in (("z1", R.Z1), ("z2", R.Z2)):
        assert float(T(f"{z}_zero")[0][z]) == 0.0 and S(f"{z}_zero") == [st]
        assert 0.0 < float(T(f"{z}_above")[0][z]) < 1e-6 and S(f"{z}_above") != [st]
        ta = cases[f"{z}_zero"].kf1 if z == "z1" else cases[f"{z}_zero"].kf2
        tb = cases[f"{z}_above"].kf1 if z == "z1" else cases[f"{z}_above"].kf2
        assert adjacent(ta["pose"]["tcw"][2], tb["pose"]["tcw"][2])
    assert T("z1_zero")[0]["branch"] == "st2" and T("z2_zero")[0]["branch"] == "st1"
    # the chi-square thresholds, mono (5.991) and stereo (7.8), either keyframe
    for name, st, e, th, factor in (("reproj1_mono_edge", R.REPROJ1, "err1", "th1", 5.991),
                                    ("reproj2_mono_edge", R.REPROJ2, "err2", "th2", 5.991),
                                    ("reproj1_stereo_edge", R.REPROJ1, "err1", "th1", 7.8),
                                    ("reproj2_stereo_edge", R.REPROJ2, "err2", "th2", 7.8)):
        t = T(name)
        assert S(name) == [R.ACCEPTED, st], name
        assert float(t[0][e]) <= t[0][th] < float(t[1][e]), name
        assert t[0][th] == factor * float(C.LEVEL_SIGMA2[0]), name
        c = cases[name]
        kf = c.kf1 if st == R.REPROJ1 else c.kf2
        moved = kf["keys"]["y"] if "mono" in name else kf["u_right"]
        assert adjacent(moved[0], moved[1]), name   # the deciding input: adjacent floats
    # zero distance and one float off
    assert S("dist2_zero") == [R.ZERO_DIST] == S("dist1_zero")
    assert S("dist2_above") == [R.SCALE_RATIO] == S("dist1_below")
    # ratioDist == ratioOctave * ratioFactor exactly, and one float above
    t = T("ratio_eq")[0]
    assert t["ratio_dist"] == t["ratio_octave"] * t["ratio_factor"] and S("ratio_eq") == [R.ACCEPTED]
    assert S("ratio_above") == [R.SCALE_RATIO]
    assert adjacent(T("ratio_above")[0]["ratio_dist"], t["ratio_dist"])
    # the SVD's edges
    for name in ("svd_tie", "w_zero", "svd_eps_edge"):
        t = T(name)[0]
        assert t["skipped"] == 6 and t["rotations"] == 0 and t["sweeps"] == 1, name
    assert T("svd_tie")[0]["ties"] == 2 and T("svd_tie")[0]["W"][2] == T("svd_tie")[0]["W"][3]
    assert S("w_zero") == [R.W_ZERO]   # reached through the SVD: vt.row(3) = (0, 0, 1, 0)
    assert [float(v) for v in T("w_zero")[0]["Vt"][3]] == [0.0, 0.0, 1.0, 0.0]
    # the quirks and the parallax equality
    t = T("else_if_quirk")[0]
    assert t["branch"] == "tri" and float(t["cos_stereo2"]) > 1.0
    t = T("rays_eq_stereo")
    assert t[0]["cos_rays"] == t[0]["cos_stereo1"] and t[0]["branch"] == "st1"
    assert t[1]["cos_rays"] < t[1]["cos_stereo1"] and t[1]["branch"] == "tri"
    d = cases["rays_eq_stereo"].kf1["depth"]
    assert adjacent(d[0], d[1])
    # the gates, met exactly
    G = lambda name: int(cases[name].ref()["info"]["gated"])
    assert (G("gate_stereo_eq"), G("gate_stereo_below")) == (0, 1)
    ow = lambda name: cases[name].kf2["pose"]["ow"][0]
    assert ow("gate_stereo_eq") == f32(C.CAM_D[5]) and adjacent(ow("gate_stereo_eq"),
                                                               ow("gate_stereo_below"))
    assert (G("gate_mono_below"), G("gate_mono_above"), G("gate_mono_nan")) == (1, 0, 1)
    assert float(ow("gate_mono_below")) < 0.01 < float(ow("gate_mono_above"))
    assert adjacent(ow("gate_mono_below"), ow("gate_mono_above"))
    for name in ("gate_stereo_below", "gate_mono_below", "gate_mono_nan"):
        r = cases[name].ref()
        assert (r["status"] == R.NOT_TRIED).all() and not r["info"]["counts"].any(), name
    # undefined inputs: an index at the count, octaves outside, stereo flags without depth
    assert S("undefined_kinds") == [R.ACCEPTED] + [R.UNDEFINED] * 5


def test_counts_patterns_and_capacity(cases):
    pats = collections.defaultdict(set)
    for c in cases.values():
        if "pattern" not in c.tags:
            continue
        n = int((c.match12 >= 0).sum())
        acc = c.ref()["status"][:n] == R.ACCEPTED
        assert (acc == c.accept).all(), c.name
        pats[n].add(next(t for t in c.tags if not t.startswith(("pattern", "count"))))
    assert set(pats) == {1, 63, 64, 65, C.WG + 1}
    for n in (63, 64, 65, C.WG + 1):
        assert {"all", "none", "alt", "last"} <= pats[n], n
    assert "round2_first" in pats[C.WG + 1] and "wave2_first" in pats[65]
    assert len(cases["empty"].match12) == 0 and (cases["no_match_only"].match12 < 0).all()
    ex, ov = cases["cap_exact"].ref(), cases["cap_over"].ref()
    assert ex["cursor"] == cases["cap_exact"].capacity and not ex["info"]["overflow"]
    assert ov["info"]["overflow"] == 1 and ov["cursor"] == cases["cap_over"].cursor
    assert cases["cap_over"].cursor + int(ex["info"]["n_new"]) == cases["cap_over"].capacity + 1
    assert (ov["status"] == 0xEE).all()   # nothing but info is written


def test_w_zero_branch_by_a_direct_call(cases):
    """:395 is also reached through the SVD (case w_zero); this asserts the
    branch itself on an injected vt.row(3)."""
    c = cases["gate_stereo_eq"]
    fake = lambda A, libm, sw, tr: ([1.0, 1.0, 1.0, 0.0],
                                    [[f32(0)] * 4] * 3 + [[f32(1), f32(2), f32(3), f32(0)]], 1)
    k1, k2 = c.kf1["keys"][0], c.kf2["keys"][0]
    args = (k1, -1.0, -1.0, k2, -1.0, -1.0, c.kf1["pose"], c.kf2["pose"], C.CAM_D, C.CAM_D,
            C.SCALE_FACTORS, C.LEVEL_SIGMA2)
    assert R.triangulate_match(*args, svd=fake) == (R.W_ZERO, None)
    assert R.triangulate_match(*args)[0] == R.ACCEPTED


SWITCH_CASE = dict(gate_stereo_le="gate_stereo_eq", gate_mono_float="gate_mono_below",
                   no_else_if="else_if_quirk", kf2_own_bf="kf1_bf_quirk",
                   sort_nonstrict="svd_tie", eps_single="svd_eps_edge",
                   sweep_cap_2="nat_mono_100", descending_order="nat_stereo_200",
                   z1_lt="z1_zero", z2_lt="z2_zero", rays_le="rays_eq_stereo",
                   rays_ge0="rays_zero", ratio_le="ratio_eq")


def _answer(r):
    return tuple(r[k].tobytes() for k in ("status", "x3d", "pairs", "points", "pidx1", "pidx2",
                                          "info")) + (r["cursor"],)


@pytest.mark.parametrize("switch", R.SWITCHES)
def test_a_wrong_neighbour_of_each_rule_changes_a_named_case(cases, switch):
    assert set(SWITCH_CASE) == set(R.SWITCHES) and len(R.SWITCHES) >= 10
    c = cases[SWITCH_CASE[switch]]
    assert _answer(c.run(sw=frozenset([switch]))) != _answer(c.ref()), (switch, c.name)
    assert _answer(c.run()) == _answer(c.ref())   # the restatement itself is deterministic


def test_libm_and_pinned_modes_select_the_same_status(cases):
    n = 0
    for c in cases.values():
        r = c.run(libm=True)
        assert (r["status"] == c.ref()["status"]).all(), c.name
        assert r["info"].tobytes() == c.ref()["info"].tobytes(), c.name
        n += int((c.match12 >= 0).sum())
    assert n >= 2000


# measured over the natural cases: 4.92e-7 rad; the bound is 4 x that
SVD_ANGLE_BOUND = 2.0e-6


def test_restated_svd_against_numpy_and_sweep_counts(cases):
    worst, min_gap, max_sweeps, n = 0.0, 1.0, 0, 0
    for c in cases.values():
        if "natural" not in c.tags:
            continue
        for t in c.traces():
            if t.get("branch") != "tri":
                continue
            A = np.array(t["A"], np.float64)
            _, s, vt = np.linalg.svd(A)
            gap = (s[2] - s[3]) / s[2]
            assert gap >= 1e-3, (c.name, t["i1"], gap)   # the last vector is well defined
            v = np.array(t["Vt"][3], np.float64)
            v /= np.linalg.norm(v)
            angle = float(np.linalg.norm(v - np.sign(v @ vt[3]) * vt[3]))
            assert angle < SVD_ANGLE_BOUND, (c.name, t["i1"], angle)
            worst, min_gap = max(worst, angle), min(min_gap, gap)
            max_sweeps = max(max_sweeps, t["sweeps"])
            n += 1
    directed = max(t.get("sweeps", 0) for c in cases.values() for t in c.traces())
    print(f"SVD over {n} natural triangulations: worst angle {worst:.3e} rad, smallest relative "
          f"gap {min_gap:.3f}, most sweeps {max_sweeps} (directed cases: {directed})")
    assert n >= 500 and max_sweeps < 30
    # two directed cases (a far stereo depth against a short baseline) leave a column of
    # A at the rounding floor and run into the cap: the cap is part of the answer there
    assert directed == 30


def test_median_restatement():
    for name, idx, pose, pos, q in C.median_cases():
        med, cnt = R.scene_median_depth(idx, pose, pos, q)
        z = sorted(float(R.row_dot(pose["rcw"][6:9], pose["tcw"][2], pos[i])) for i in idx if i >= 0)
        assert cnt == len(z), name
        if not z:
            assert np.isnan(med), name
        else:
            assert float(med) == z[(len(z) - 1) // q], name
    names = [c[0] for c in C.median_cases()]
    assert {"median_0", "median_1", "median_2", "median_even6", "median_ties"} <= set(names)
