"""The directed inputs of mapping_edge_cases.py on the CPU: the oracle equals the
independent restatement (pyref.search_for_initialization /
distinctive_descriptor) on n, m12, the prev bytes and best; the census of each
input meets the minimum stated next to its builder (printed, run with -s to
read it); every wrong neighbour of a rule changes the answer of a named input;
and the natural init_pair scenes and the two random crowds of
test_gpu_mapping.py never leave the top-K path of the resolve -- what they do
reach of the directed conditions is recorded in NATURAL."""
import functools

import numpy as np
import pytest

import mapping_edge_cases as E
import scenarios as S


@functools.lru_cache(maxsize=None)
def case(name):
    return E.CASES[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name):
    import oracle as o
    o.lib()
    c = case(name)
    if c["kind"] == "init":
        return [E.run_oracle(o, p) for p in c["problems"]]
    return o.distinctive_descriptors(c["offs"], c["desc"])


def test_limits():
    """The sizes the cases are built around are the build's."""
    L = E.limits()
    assert (L["topk"], L["list"], L["stage"]) == (16, 256, 1536)
    # 16 B per padded slot + the kernel's 128 static bytes fill 160 KiB exactly
    assert L["max_stride"] == 10232 and 16 * L["max_stride"] + 128 == 160 * 1024


INIT = sorted(n for n, (b, m) in E.CASES.items() if n != "distinctive")


@pytest.mark.parametrize("name", INIT)
def test_oracle_matches_restatement_and_census(name):
    c, minimum = case(name), E.CASES[name][1]
    refs = reference(name)
    assert len(minimum) == len(c["problems"])
    for p, ref, mn in zip(c["problems"], refs, minimum):
        got = E.run_pyref(p)
        assert ref[0] == got[0], (p["name"], ref[0], got[0])
        assert np.array_equal(ref[1], got[1]), (p["name"], np.nonzero(ref[1] != got[1])[0][:10])
        assert ref[2].dtype == got[2].dtype and ref[2].tobytes() == got[2].tobytes(), p["name"]
        assert ref[0] == int((ref[1] >= 0).sum())
        cen = E.census(p)
        print(p["name"], cen)
        E.meets(cen, mn)


def test_distinctive_oracle_matches_restatement_and_census():
    c = case("distinctive")
    ref = reference("distinctive")
    got = E.distinctive_pyref(c)
    assert np.array_equal(ref, got), np.nonzero(ref != got)[0]
    cen = E.census_distinctive(c)
    print("distinctive", cen, dict(zip(c["names"], ref.tolist())))
    E.meets(cen, E.CASES["distinctive"][1])
    best = dict(zip(c["names"], ref.tolist()))
    assert best["identical"] == 0 and best["tied_rows"] == 2 and best["last_wins"] == 5
    assert best["median_255"] == 1 and best["median_256"] == 1 and best["median_256_long"] == 1
    assert best["even_median"] == 0 and best["tied_long"] == 97
    assert best["n0"] == -1 and best["empty_last"] == -1 and best["n1"] == 0


def test_shifted_bounds_is_exact():
    """The shifted problems are the equalities problems moved by an exactly
    representable amount (asserted by the builder), with the grid moved along."""
    for p, base in zip(case("shifted_bounds")["problems"], case("equalities")["problems"]):
        assert p["bounds"] == (E.SHIFT, E.W + E.SHIFT, E.SHIFT, E.H + E.SHIFT)
        assert np.array_equal(p["prev"] - np.float32(E.SHIFT), base["prev"])
        assert p["d1"].tobytes() == base["d1"].tobytes() and p["d2"].tobytes() == base["d2"].tobytes()


# Which input separates which wrong rule.  A rule that no input changes would
# not be tested by these inputs at all.
SENSITIVITY = dict(mdist_lt="equalities", th_lt="equalities", ratio_le="equalities",
                   window_le="equalities", tie_last="equalities", no_stolen_vote="steal_hist",
                   no_level_f1="batch_lanes", no_level_f2="stage_boundary")
# further inputs that separate a rule as well
ALSO = (("tie_last", "counts"), ("no_level_f1", "steal_hist"), ("no_level_f2", "counts"),
        ("window_le", "shifted_bounds"))


def _changed(name, rule):
    out = []
    for p, ref in zip(case(name)["problems"], reference(name)):
        wrong = E.run_pyref(p, rules=(rule,))
        out.append(int((wrong[1] != ref[1]).sum()) + int(wrong[0] != ref[0]))
    return out


@pytest.mark.parametrize("rule,name", sorted(SENSITIVITY.items()) + sorted(ALSO))
def test_sensitivity(rule, name):
    diff = _changed(name, rule)
    print(rule, name, "entries changed per problem", diff)
    assert sum(diff) > 0


def test_tie_rule_needs_a_ratio_above_one():
    """Equal best distances reject under nnratio 0.9 whichever of them is
    kept, so only the nnratio 1.25 problem tells the first minimum from the last."""
    assert _changed("equalities", "tie_last") == [0, 2]


def test_stolen_votes_decide_in_both_shapes():
    assert all(d > 0 for d in _changed("steal_hist", "no_stolen_vote"))


@pytest.mark.parametrize("rule,lists", [("median_upper", ("even_median",)),
                                        ("best_le", ("identical", "tied_rows", "tied_long"))])
def test_distinctive_sensitivity(rule, lists):
    c = case("distinctive")
    ref = dict(zip(c["names"], reference("distinctive").tolist()))
    wrong = dict(zip(c["names"], E.distinctive_pyref(c, rules=(rule,)).tolist()))
    print(rule, {k: (ref[k], wrong[k]) for k in ref if ref[k] != wrong[k]})
    for k in lists:
        assert ref[k] != wrong[k], (rule, k)


# ---------------------------------------------------------- the older inputs
DIRECTED = ("mdist_eq", "b1_50", "ratio_eq", "win_eq_x", "win_eq_y", "tie_accept", "si_only")
# What the inputs of test_gpu_mapping.py reach of the directed conditions.
# nc: candidate counts among 0, 1, 2, 16, 17, 256, 257; dry: the same counts
# with fewer than two survivors in the top 16; lanes: conflict lanes among
# 1 and 63, slow lanes among 0.
# None of them leaves the top-K path: no query's top 16 ever runs dry, so
# neither the wave-wide list resolve nor the lane-0 rescan has run on them,
# whatever their candidate counts (window 2000 gives every query 435 candidates
# and every one of them commits from its top 16).
NEVER = dict(dry=[], slow_lane0=False, tie_accept=0, exits=[])
# What they do reach, recorded: equalities come up by chance in the natural
# frames (integer level-0 coordinates put keypoints at |dx| == 100 exactly);
# the crowds have steal chains and stolen votes that decide the kept bins.
NATURAL = {
    "init_pair(0)": dict(nc=[], conflict_lanes=[], staged=True, chain=1, mdist_eq=1, b1_50=9,
                         ratio_eq=1, win_eq_x=219, win_eq_y=190, stolen_votes_decide=False),
    "init_pair(2)": dict(nc=[16, 17], conflict_lanes=[], staged=True, chain=1, mdist_eq=1, b1_50=5,
                         ratio_eq=0, win_eq_x=159, win_eq_y=114, stolen_votes_decide=False),
    "init_pair(6) window 2000": dict(nc=[], conflict_lanes=[1], staged=True, chain=1, mdist_eq=3,
                                     b1_50=7, win_eq_x=0, win_eq_y=0),
    "collisions(20)": dict(nc=[], conflict_lanes=[], staged=True, chain=4, mdist_eq=31, b1_50=0,
                           ratio_eq=13, win_eq_x=0, stolen_votes_decide=True),
    "collisions(40)": dict(nc=[256, 257], conflict_lanes=[], staged=True, chain=4, b1_50=0,
                           win_eq_x=0),
    "unstaged": dict(nc=[16, 17], conflict_lanes=[63], staged=False, chain=2, b1_50=0, win_eq_x=1,
                     win_eq_y=0, stolen_votes_decide=True),
}


def _natural_inputs(oracle):
    for seed, f2, w, h in ((2, 1, 1241, 376),):
        s = S.init_pair(oracle, seed, f2, w=w, h=h, nf=2000)
        yield E.as_problem(s, "init_pair(%d)" % seed, 100)
    # window 2000 covers the frame: every level-0 keypoint is a candidate
    s = S.init_pair(oracle, 6, 1, w=640, h=480, nf=2000)
    yield E.as_problem(s, "init_pair(6) window 2000", 2000, 0.9, False)
    for window, check in ((20, True), (40, False)):
        yield E.as_problem(E.crowd_collisions(), "collisions(%d)" % window, window, 0.9, check)
    yield E.as_problem(E.crowd_unstaged(), "unstaged", 30)


def summary(cen):
    counts = (0, 1, 2, 16, 17, 256, 257)
    out = dict(nc=[c for c in counts if c in cen["nc"]],
               dry=[c for c in counts[3:] if cen["dry"].get(c, 0)],
               conflict_lanes=[l for l in (1, 63) if l in cen["conflict_lanes"]],
               slow_lane0=0 in cen["slow_lanes"], full_clean=cen["full_clean"],
               paths=cen["paths"], staged=cen["staged"], steals=cen["steals"], chain=cen["chain"],
               exits=cen["exits"])
    out.update({k: int(cen[k]) for k in DIRECTED})
    if "stolen_votes_decide" in cen:
        out["stolen_votes_decide"] = cen["stolen_votes_decide"]
    return out


def test_older_inputs_do_not_reach_the_directed_conditions(oracle):
    for p in _natural_inputs(oracle):
        ref = E.run_oracle(oracle, p)
        tr = []
        got = E.run_pyref(p, trace=tr)
        assert ref[0] == got[0] and np.array_equal(ref[1], got[1]) and \
            ref[2].tobytes() == got[2].tobytes(), p["name"]
        s = summary(E.census(p, traced=(got[0], tr)))
        print(p["name"], s)
        assert s["paths"]["topk"] == sum(s["paths"].values()), (p["name"], s["paths"])
        for k, v in list(NEVER.items()) + list(NATURAL[p["name"]].items()):
            assert s[k] == v, (p["name"], k, v, s[k])
