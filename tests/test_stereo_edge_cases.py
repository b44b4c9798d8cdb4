"""The directed inputs of stereo_edge_cases.py on the CPU: the oracle equals the
independent restatement (pyref.stereo_match) bit for bit on u_right, depth and
the SAD of every accepted match, and the construction's own answer where it has
one; the census of each input meets the minimum stated next to its builder
(printed, run with -s to read it); every wrong neighbour of a rule changes the
answer of a named input; and the natural synthetic pairs reach none of it."""
import functools

import numpy as np
import pytest

import scenarios as S
import stereo_edge_cases as E


@functools.lru_cache(maxsize=None)
def case(name):
    return E.CASES[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name):
    import oracle as o
    o.lib()
    return E.run_oracle(o, case(name))


def _same(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_oracle_matches_restatement_and_census(name):
    c, minimum = case(name), E.CASES[name][1]
    ref = reference(name)
    got = E.run_pyref(c)
    for what, a, b in zip(("u_right", "depth", "sad"), ref, got):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), \
            (name, what, np.nonzero(a != b)[0][:10])
    E.check_expect(c, ref)
    # the two-output call of the older tests is the same computation
    import oracle as o
    assert _same(o.stereo_match(*E.args(c)), ref[:2])
    # SAD >= 0 exactly where a match was accepted; reset matches keep theirs
    assert ((ref[0] >= 0) <= (ref[2] >= 0)).all()
    cen = E.census(c)
    print(name, cen)
    assert cen["reset"] == int(((ref[2] >= 0) & (ref[0] < 0)).sum())
    for k, v in minimum.items():
        if isinstance(v, set):
            assert v <= set(cen[k]), (k, v, cen[k])
        elif k in E.EXACT_KEYS:
            assert cen[k] == v, (k, v, cen[k])
        else:
            assert cen[k] >= v, (k, v, cen[k])
    assert cen["fill"] <= 1.0


def test_capacity_fill():
    cen = E.census(case("capacity"))
    assert cen["NR"] == max(cen["NL"], cen["NR"])   # NR is the stride
    assert 0.9 <= cen["fill"] <= 1.0, cen["fill"]


def test_largest_sad():
    """The directed maxima DESIGN.md §4.2 records."""
    cen = E.census(case("sad_magnitudes"))
    assert cen["max_sad"] == 60180 and cen["max_sad"] <= 120 * 510


# Which input separates which wrong rule.  A rule that no input changes would
# not be tested by these inputs at all.
SENSITIVITY = dict(
    hamming_le="hamming_gates", minu_strict="u_gates", maxu_strict="u_gates",
    octave_pm2="octave_gates", tie_last="row_lists", band_round="bands", row_round="bands",
    endu_gt="border", round_even="border", sad_first_vs_last="sad_magnitudes",
    edge_inc_kept="shifts", no_zero_disp_branch="disparity", maxd_le="disparity",
    prune_le="prune_threshold", median_lower="prune_v2", sad_s16="sad_magnitudes")


@pytest.mark.parametrize("rule", sorted(SENSITIVITY))
def test_sensitivity(rule):
    name = SENSITIVITY[rule]
    ref = reference(name)
    wrong = E.run_pyref(case(name), rules=(rule,))
    diff = np.nonzero((wrong[0] != ref[0]) | (wrong[1] != ref[1]) | (wrong[2] != ref[2]))[0]
    print(rule, name, "entries changed", len(diff), diff[:10])
    assert len(diff) > 0


def test_minu_gate_with_rounding_intrinsics():
    """The uR == minU input of the KITTI intrinsics separates the strict rule too."""
    name = "u_gates_kitti"
    assert not _same(E.run_pyref(case(name), rules=("minu_strict",)), reference(name))


# what the natural pairs reach, per seed
# (the one match the disparity window of :676 rejects, seed 1, lies on its
# negative side: no natural disparity reaches maxD)
NATURAL = {1: dict(kept=401, disp_neg=1, max_sad=32846, sad_ties=0, median=2794.0),
           2: dict(kept=422, disp_neg=0, max_sad=31355, sad_ties=1, median=2046.0),
           3: dict(kept=423, disp_neg=0, max_sad=28665, sad_ties=1, median=1949.0)}


@pytest.mark.parametrize("seed", sorted(NATURAL))
def test_natural_pairs(oracle, seed):
    """Parity on the natural pairs, and their census: every column the directed
    inputs exist for is zero there."""
    sp = S.stereo_pair(oracle, seed)
    c = dict(name="stereo_pair(%d)" % seed, lk=sp["kl"], ld=sp["dl"], rk=sp["kr"], rd=sp["dr"],
             lpyr=sp["lpyr"], rpyr=sp["rpyr"], scale=sp["scale"], inv=sp["inv"], bf=S.BF, fx=S.FX,
             w=sp["w"], h=sp["h"])
    ref = E.run_oracle(oracle, c)
    got = E.run_pyref(c)
    assert _same(ref, got)
    cen = E.census(c)
    print(c["name"], cen)
    for k in ("ur_eq_minu", "border", "endu_last", "zero_branch", "band_row0", "band_last_row",
              "at_th", "disp_ge_maxd", "disp_eq_maxd", "big_low"):
        assert cen[k] == 0, (k, cen[k])
    assert cen["max_sad"] < 40000 and cen["big_high"] <= 1
    assert cen["median"] > 0 and cen["V"] >= 500
    for k, v in NATURAL[seed].items():
        assert cen[k] == v, (k, v, cen[k])
