"""The Python restatement of Tracking::UpdateLocalMap (tests/local_map_ref.py)
on its own: answers worked out by hand for the tiny inputs, the conditions
every directed input must exercise, and one wrong neighbour per reference rule
that changes a named input's answer."""
import numpy as np
import pytest

import local_map_cases as C
import local_map_ref as R


def run(name, rules=(), mp_stride=None):
    i = C.get(name)
    return R.update_local_map(i["map"], i["kp_match"], i["local_kf"],
                              i["mp_stride"] if mp_stride is None else mp_stride, rules)


def fields(rec):
    return tuple(int(rec[k]) for k in R.INFO_DTYPE.names)


def test_tiny_by_hand():
    """kf -> rank 2 0 4 1 3.  Matches [p0, -, p1, p2(bad), -2, p0]: p2 is nulled;
    kf0 gets 2 votes, kf1 3.  Rank order: kf1 (pKFmax, 3), kf0.  kf1's
    covisibles [0, 2]: 0 is voted, 2 is added.  kf0: child 4 added, parent 3
    added and the pass ends.  Points: kf1 [p0, p1, p3], kf0 [p0, p3, -1] all
    taken, kf2 [p3] taken, kf4 [p4], kf3 [p2] bad."""
    r = run("tiny")
    assert r["kp_match"].tolist() == [0, -1, 1, -1, -2, 0]
    assert r["local_kf"].tolist() == [1, 0, 2, 4, 3]
    assert r["local_index"].tolist() == [0, 1, 3, 4]
    assert r["mps"]["seen"].tolist() == [1, 1, 0, 0]
    assert r["mps"]["has_obs"].tolist() == [1, 1, 1, 0]
    assert r["locked"].tolist() == [1, 0, 1, 0, 0, 1]
    #                   n_local_kf voted added ref max points nulled kept
    assert fields(r["info"]) == (5, 2, 3, 1, 3, 4, 1, 0)
    m = C.get("tiny")["map"]
    assert r["desc"].tobytes() == m["desc"][[0, 1, 3, 4]].tobytes()
    assert r["mps"]["pos"].tobytes() == m["points"]["pos"][[0, 1, 3, 4]].tobytes()


def test_tiny_empty_by_hand():
    """No matches: the stale list [3, 1] is kept and walked: kf3 [p0, p1],
    kf1 [p1] taken already."""
    r = run("tiny_empty")
    assert r["kp_match"].tolist() == [-1, -2, -1]
    assert r["local_kf"].tolist() == [3, 1]
    assert r["local_index"].tolist() == [0, 1]
    assert r["mps"]["seen"].tolist() == [0, 0]
    assert fields(r["info"]) == (2, 0, 0, -1, 0, 2, 0, 1)


def test_capacity_cuts_the_outputs_not_the_count():
    r = run("over_mp_stride")
    full = run("over_mp_stride", mp_stride=100)
    assert int(r["info"]["n_local_points"]) == 26 and len(r["local_index"]) == 5
    assert r["local_index"].tolist() == full["local_index"][:5].tolist()


MINIMUMS = {
    "tiny_empty": dict(stale_list_kept=1, minus2=1),
    "empty_stale": dict(stale_list_kept=1),
    "all_voted_bad": dict(all_voted_bad=1),
    "tie_max": dict(max_tie_rank_vs_index=1),
    "voted79": dict(n_voted_good=79, over80_break=1),
    "voted80": dict(n_voted_good=80, parent_break_unvisited=1),
    "voted81": dict(n_voted_good=81, over80_break=1),
    "voted82": dict(n_voted_good=82, over80_break=1),
    "voted100": dict(n_voted_good=100, over80_break=1),
    "neigh_11th": dict(neigh_11th_only=1, neigh_bad_skipped=2),
    "neighbours": dict(neigh_bad_skipped=1, neigh_already_added=1),
    "children5": dict(child_multi=2),
    "children16": dict(child_multi=2, children_over_16=1),
    "children17": dict(child_multi=2, children_over_16=2),
    "parent_break": dict(parent_break_unvisited=1),
    "parent_included": dict(parent_included_nobreak=1, parent_bad_added=1),
    "points_mix": dict(kf_no_points=1, neg_slots=3, dup=4, dup_within=1, bad_points_skipped=5,
                       matched_no_obs=1, matched_bad_nulled=1, minus2=2, map_seen_differs=5,
                       seen_local=3),
    "over_mp_stride": dict(over_mp_stride=1),
    "count63": dict(n_local_points=63), "count64": dict(n_local_points=64),
    "count65": dict(n_local_points=65), "count1023": dict(n_local_points=1023),
    "count1024": dict(n_local_points=1024), "count1025": dict(n_local_points=1025),
    "tier%d" % C.HASH_CAP: dict(distinct_ids=C.HASH_CAP),
    "tier%d" % (C.HASH_CAP + 1): dict(distinct_ids=C.HASH_CAP + 1),
    "tier_mix": dict(distinct_ids=C.HASH_CAP + 1, dup=100, neg_slots=2, bad_points_skipped=100,
                     matched_bad_nulled=1),
}
EXACT = ("n_voted_good", "n_local_points")


@pytest.mark.parametrize("name", sorted(MINIMUMS))
def test_census_minimums(name):
    i = C.get(name)
    ev = R.census(i, i["mp_stride"])
    for k, v in MINIMUMS[name].items():
        assert (ev[k] == v) if k in EXACT else (ev[k] >= v), (name, k, ev[k], v)
    m = i["map"]
    assert len(m["rank"]) <= 130 and sorted(m["rank"]) == list(range(len(m["rank"])))
    assert not np.array_equal(m["rank"], np.arange(len(m["rank"])))
    if name in C.SMALL and not name.startswith("count10"):
        assert max(len(x) for x in m["kf_mp"]) <= 64


def test_tier_inputs_sit_on_the_boundary():
    a, b = C.get("tier%d" % C.HASH_CAP), C.get("tier%d" % (C.HASH_CAP + 1))
    assert R.census(a)["slot_total"] == C.HASH_CAP      # all distinct: the smallest slot total
    assert R.census(b)["slot_total"] == C.HASH_CAP + 1
    assert len(b["map"]["points"]) > C.HASH_CAP         # the scratch table exists for it


def test_final_sizes_around_eighty():
    size = lambda n: fields(run("voted%d" % n)["info"])[:3]
    assert size(79) == (82, 79, 3) and size(80) == (83, 80, 3)
    assert size(81) == (81, 81, 0) and size(82) == (82, 82, 0) and size(100) == (100, 100, 0)


SWITCH = {
    "index_order": "tie_max", "max_ge": "tie_max", "neigh11": "neigh_11th",
    "limit_ge80": "voted80", "no_parent_break": "parent_break",
    "parent_bad_check": "parent_included", "neigh_continue": "neighbours",
    "child_list_order": "children5", "clear_on_empty": "empty_stale",
    "last_occurrence": "points_mix", "seen_from_map": "points_mix",
}


def test_every_rule_has_a_switch():
    assert sorted(SWITCH) == sorted(R.RULES)


@pytest.mark.parametrize("rule", R.RULES)
def test_rule_switch_changes_the_named_input(rule):
    name = SWITCH[rule]
    a, b = run(name), run(name, rules=(rule,))
    same = all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()
               for k in ("kp_match", "local_kf", "local_index", "mps", "desc", "locked", "info"))
    assert not same, (rule, name)


def test_limit_switch_also_shows_at_79():
    assert run("voted79")["local_kf"].tolist() != run("voted79", rules=("limit_ge80",))["local_kf"].tolist()


def test_combine_keeps_every_input_s_answer():
    names = ["tiny", "tie_max", "children5", "points_mix", "empty_stale"]
    m, probs = C.combine([C.get(n) for n in names], seed=3)
    ko = mo = 0
    for n, q in zip(names, probs):
        i = C.get(n)
        a = run(n)
        b = R.update_local_map(m, q["kp_match"], q["local_kf"], q["mp_stride"])
        assert (b["local_kf"] - ko).tolist() == a["local_kf"].tolist(), n
        assert (b["local_index"] - mo).tolist() == a["local_index"].tolist(), n
        assert b["mps"].tobytes() == a["mps"].tobytes() and b["locked"].tolist() == a["locked"].tolist()
        ko += len(i["map"]["rank"])
        mo += len(i["map"]["points"])


def test_merge_and_finish():
    km = np.array([5, -1, -2, 7, 9, 3], np.int32)
    out = R.merge(km, np.array([-1, 2, 0, -1, 1, -1], np.int32), np.array([40, 41, 42], np.int32))
    assert out.tolist() == [5, 42, 40, 7, 41, 3]
    pts = np.zeros(50, R.MAP_POINT_DTYPE)
    pts["has_obs"][[5, 40, 41]] = 1
    ol = np.array([0, 1, 0, 1, 0, 0], np.uint8)
    n, k = R.finish(out, ol, pts, False, False)
    assert n == 3 and k.tolist() == out.tolist()           # 5, 40, 41 have observations
    n, k = R.finish(out, ol, pts, True, False)
    assert n == 4 and k.tolist() == out.tolist()           # every non-outlier
    n, k = R.finish(out, ol, pts, False, True)
    assert n == 3 and k.tolist() == [5, -1, 40, -1, 41, 3]
