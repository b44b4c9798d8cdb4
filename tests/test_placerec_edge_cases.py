"""CPU checks of the directed place-recognition inputs on the restatement alone
(tests/placerec_ref.py): a census that every case of placerec_edge_cases.py
does what its docstring claims, and the rule switches -- each switch states one
rule of ScoringObject.cpp / KeyFrameDatabase.cc wrongly and must change the
answer of a directed case, which shows without a GPU that a kernel wrong in that
way fails tests/test_gpu_placerec_edges.py.  No GPU needed."""
import math

import numpy as np
import pytest

import placerec_edge_cases as ec
import placerec_ref as ref

f32 = np.float32


def _bits(x):
    return int(ec.bits64(x).ravel()[0])


def _fbits(x):
    return int(ec.bits32(x).ravel()[0])


def _score_of(r, kf_id):
    return r["scores"][r["ids"].tolist().index(kf_id)]


def _chain(t):
    s = 0.0
    for x in t:
        s += x
    return s


def _pairwise(t):
    t = list(t)
    while len(t) > 1:
        t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return t[0]


# -------------------------------------------------------------- score census
def test_census_chunk_positions():
    cases = ec.score_case("chunk_positions")
    s, a, b = cases[0]
    assert len(b[0]) == 65
    assert np.flatnonzero(np.isin(b[0], a[0])).tolist() == [0, 63, 64]
    singles = [np.flatnonzero(np.isin(c[2][0], c[1][0])).tolist() for c in cases[2:5]]
    assert singles == [[0], [63], [64]] and all(len(c[1][0]) == 1 for c in cases[2:5])
    _, a, b = cases[5]
    assert a[0][-1] == b[0][-1] and np.isin(b[0], a[0]).sum() == 1
    assert int(cases[6][1][0][-1]) == 0xFFFFFFFF and int(cases[6][1][0][-2]) == 0xFFFFFFFE
    # exact L1 answers: the sum of min(vi, wi) over the common words
    want = [0.25 + 0.125 + 0.03125, 0.40625, 0.25, 0.125, 0.0625, 0.25, 0.5, 0.5]
    assert [ref.score(c[1], c[2], ec.L1) for c in cases[:8]] == want


def test_census_chain_order():
    dot, l2 = ec.score_case("chain_order")
    for case in (dot, l2):
        _, a, b = case
        assert np.flatnonzero(np.isin(b[0], a[0])).tolist() == [61, 62, 63, 64, 65, 66]
    t = ec.chain_terms(dot)
    assert t == ec.CHAIN_DOT
    chain = ref.score(dot[1], dot[2], ec.DOT)
    assert (chain, _chain(t[::-1]), _pairwise(t)) == (4.001, 4.0, 3.001)
    assert chain == _chain(t) and _bits(chain) != _bits(_chain(t[::-1])) and _bits(chain) != _bits(_pairwise(t))
    assert ref.score(dot[1], dot[2], ec.DOT, "pairwise") == 3.001
    t = ec.chain_terms(l2)
    sums = {_chain(t), _chain(t[::-1]), _pairwise(t)}
    assert len(sums) == 3 and max(sums) < 1 and min(sums) > 0   # below the clamp, all different
    assert ref.score(l2[1], l2[2], ec.L2) == 1.0 - math.sqrt(1.0 - _chain(t))
    assert _bits(ref.score(l2[1], l2[2], ec.L2)) != _bits(ref.score(l2[1], l2[2], ec.L2, "pairwise"))


def test_census_chi_guard():
    ab, ba, gh = ec.score_case("chi_guard")
    sums = [x + y for x, y in ref._common(ab[1], ab[2])]
    assert sums.count(0.0) == 3 and len(sums) == 6 and sums[0] != 0 and sums[-1] != 0
    pairs = list(ref._common(ab[1], ab[2]))
    assert (0.0, 0.0) in pairs and (0.375, -0.375) in pairs
    assert any(math.copysign(1, x) < 0 and x == 0 and y == 0 for x, y in pairs)   # (-0.0, 0.0)
    # 2 (0.25/1 + 0.0625/0.5 + 0.125/0.75), the guarded words contribute nothing
    assert ref.score(ab[1], ab[2], ec.CHI) == 2. * (0.25 + 0.125 + 0.125 / 0.75)
    allg = [x + y for x, y in ref._common(gh[1], gh[2])]
    assert len(allg) == 3 and all(v == 0.0 for v in allg)
    assert _bits(ref.score(gh[1], gh[2], ec.CHI)) == _bits(0.0)
    assert math.isnan(ref.score(gh[1], gh[2], ec.CHI, "no_chi_guard"))


def test_census_l2_clamp():
    cases = ec.score_case("l2_clamp")
    sums = [_chain(x * y for x, y in ref._common(c[1], c[2])) for c in cases]
    # the last: 1 + 2^-53 is a tie and rounds to even, exactly 1
    assert sums == [1.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, 1.0]
    got = [ref.score(c[1], c[2], ec.L2) for c in cases]
    assert got[0] == 1.0 and got[1] == 1.0 and got[3] == 1.0
    assert got[2] == 1.0 - math.sqrt(2.0 ** -53) and got[2] < 1.0
    assert math.isnan(ref.score(cases[1][1], cases[1][2], ec.L2, "no_l2_clamp"))


def test_census_signs_and_nonfinite():
    cases = ec.score_case("signs_nonfinite")
    got = [ref.score(a, b, s) for s, a, b in cases]
    # L1, neg against pos: |-.75| - .5 - .25 = 0, |-.5| - 0 - .5 = 0, |.5| - .25 - .25 = 0
    assert _bits(got[0]) == _bits(-0.0) and _bits(got[1]) == _bits(-0.0)
    assert got[2] == 0.75                         # |0| - .5 - .5, 0, |0| - .25 - .25: -1.5 / -2
    assert math.isnan(got[3])                     # sqrt(-0.125)
    assert got[4] == 1.0                          # pos against itself: every product positive
    assert math.isnan(got[5]) and got[6] == math.inf    # inf - inf; inf * .25 + ...
    assert got[7] == 1.0 and math.isnan(got[8]) and got[9] == math.inf   # clamp; inf / inf; sqrt(inf)
    assert all(_bits(g) == _bits(-0.0) for g in (got[10], got[11]))   # L1 without a common word
    assert [_bits(g) for g in got[12:]] == [_bits(0.0)] * 4


def test_census_batch_shapes():
    assert ec.PAIR_COUNTS == [1, 4, 5]
    for s in ec.SCORINGS:
        pairs, want = ec.score_pairs_by_scoring(s)
        lens = [(len(a[0]), len(b[0])) for _, a, b in pairs]
        inner = lens[1:-1]
        assert any(la == 0 and lb > 0 for la, lb in inner) and any(lb == 0 and la > 0 for la, lb in inner)
        assert len(pairs) > 5 and len(want) == len(pairs)


# ----------------------------------------------------------- database census
def test_census_loop_thresholds():
    r = ec.by_tag(ec.ref_answers("loop_thresholds"))
    eq = r["equal"]
    assert eq["seen"]["min_common"] == 6
    assert eq["ids"].tolist() == [1, 2, 3, 4] and eq["common"].tolist() == [8, 7, 7, 6]
    assert eq["scored"].tolist() == [1, 1, 1, 0]
    assert [_fbits(s) for s in eq["scores"][:3]] == [_fbits(v) for v in (1.0, 0.875, 0.75)]
    assert eq["out"] == [1, 2]                    # si == minScore kept; 0.75 scored, not retained
    assert [e[0] for e in eq["seen"]["entries"]] == [1, 2]
    assert _fbits(ec.UP) == _fbits(0.875) + 1 and r["above"]["out"] == [1]
    ae = r["all_equal"]
    assert ae["ids"].tolist() == [2, 3, 4] and ae["seen"]["min_common"] == 5
    assert [a for _, a, _ in ae["seen"]["entries"]] == [0.875] and ae["out"] == [2]
    assert r["none"]["out"] == [] and max(r["none"]["scores"]) < 2.0 and r["none"]["scored"].sum() == 3


def test_census_loop_best_init():
    r = ec.by_tag(ec.ref_answers("loop_best_init"))
    b = r["below_start"]
    assert b["scores"].tolist() == [1.0, -0.5] and b["scored"].tolist() == [1, 1]
    assert b["seen"]["entries"] == [(1, 0.5, 1)] and b["out"] == []
    assert r["kept"]["out"] == [1]


def test_census_loop_neighbour_gates():
    r = ec.by_tag(ec.ref_answers("loop_neighbour_gates"))
    p, g = r["prime"], r["gates"]
    assert set(p["scores"].tolist()) == {0.125} and len(p["ids"]) == 8
    assert g["seen"]["min_common"] == 6 and 13 not in g["ids"].tolist()
    common = dict(zip(g["ids"].tolist(), g["common"].tolist()))
    assert common[11] == 6 and common[12] == 7 and common[14] == 7
    assert _score_of(g, 11) == f32(0.125)        # stale: the gate keeps it out of the sum
    assert _score_of(g, 14) == f32(0.25) and 14 not in [e[0] for e in g["seen"]["entries"]]
    acc = {e: a for e, a, _ in g["seen"]["entries"]}
    assert acc == {10: 2.125, 12: 1.625, 15: 1.5, 16: 0.75, 17: 0.625}
    assert g["out"] == [10, 12]


def test_census_retain_thresholds():
    for tag in ("reloc", "loop"):
        r = ec.by_tag(ec.ref_answers("retain_thresholds"))[tag]
        acc = [a for _, a, _ in r["seen"]["entries"]]
        assert _fbits(acc[1]) == _fbits(f32(0.75) * f32(acc[0])) and acc[0] == 1.0
        assert _fbits(acc[2]) == _fbits(0.75) + 1
        assert r["out"] == [1, 3]


def test_census_ties():
    for tag in ("reloc", "loop"):
        r = ec.by_tag(ec.ref_answers("tie_own"))[tag]
        assert _fbits(r["scores"][0]) == _fbits(r["scores"][1]) == _fbits(0.875)
        assert r["seen"]["entries"][0] == (1, 1.75, 1) and r["out"] == [1]
    t = ec.by_tag(ec.ref_answers("tie_neighbours"))
    for tag, first in (("reloc", 2), ("loop", 2), ("reloc_swapped", 3), ("loop_swapped", 3)):
        r = t[tag]
        assert _fbits(_score_of(r, 2)) == _fbits(_score_of(r, 3)) == _fbits(1.0)
        assert r["ids"].tolist() == [1, 3, 2]      # list order is not the stored neighbour order
        assert r["seen"]["entries"][0] == (1, 2.75, first) and r["out"] == [first]


def test_census_neighbour_float_order():
    for tag in ("reloc", "loop"):
        r = ec.by_tag(ec.ref_answers("neighbour_float_order"))[tag]
        s = [f32(_score_of(r, k)) for k in (1, 3, 2)]          # entry, then stored order
        fwd = f32(f32(s[0] + s[1]) + s[2])
        rev = f32(f32(s[0] + s[2]) + s[1])
        assert (fwd, rev) == (2.0 ** 24, 2.0 ** 24 + 2) and _fbits(fwd) != _fbits(rev)
        assert r["seen"]["entries"][0] == (1, 2.0 ** 24, 3)
        assert r["seen"]["entries"][3] == (4, 12582913.0, 4)
        assert f32(0.75) * fwd < f32(12582913) <= f32(0.75) * rev
        assert r["out"] == [3, 4]


def test_census_stale_and_separate():
    r = ec.by_tag(ec.ref_answers("stale_and_separate"))
    assert _score_of(r["first"], 2) == 1.0 and _score_of(r["between"], 2) == f32(0.125)
    s = r["stale"]
    assert s["ids"].tolist() == [1, 2, 3] and s["scored"].tolist() == [1, 0, 1]
    assert _score_of(s, 2) == 1.0                 # the first reloc query's, not the loop query's
    assert _score_of(r["between"], 2) < _score_of(s, 1) < _score_of(s, 2)
    assert s["seen"]["entries"][0] == (1, 1.875, 2) and s["out"] == [2]


def test_census_list_order():
    r = ec.by_tag(ec.ref_answers("list_order"))
    assert r["first"]["ids"].tolist() == [40, 30, 20, 25] == r["first_loop"]["ids"].tolist()
    assert r["erased"]["ids"].tolist() == [40, 20, 25]
    assert r["readded"]["ids"].tolist() == [40, 20, 30, 25] == r["readded_loop"]["ids"].tolist()


def test_census_clear_reuse():
    r = ec.by_tag(ec.ref_answers("clear_reuse"))
    assert r["before"]["ids"].tolist() == [1, 2] and r["before"]["scores"].tolist() == [0.125, 1.0]
    assert r["before_loop"]["scores"].tolist() == [0.125, 1.0]
    assert r["empty"]["out"] == [] and len(r["empty"]["ids"]) == 0 and r["empty"]["seen"]["n_db"] == 0
    for tag in ("after", "after_loop"):
        a = r[tag]
        assert a["ids"].tolist() == [5, 6, 7] and a["scored"].tolist() == [1, 0, 1]
        assert _fbits(_score_of(a, 6)) == 0       # second keyframe since clear(), never scored
        assert a["seen"]["entries"][0] == (5, 0.875, 5) and a["out"] == [5, 7]


def test_census_denormal_scores():
    r = ec.by_tag(ec.ref_answers("denormal_scores"))
    tiny = float(np.finfo(np.float32).tiny)       # 2^-126: everything here lies below it
    for tag in ("reloc", "loop"):
        q = r[tag]
        assert [_fbits(s) for s in q["scores"]] == [768, 257, 1, 1, 0] and max(q["scores"]) < tiny
        acc = {e: _fbits(f32(a)) for e, a, _ in q["seen"]["entries"]}
        assert acc[1] == 768 + 257 + 1 and acc[4] == 2 and acc[2] == 257
        # 0.75f * 1026 ulps = 769.5 ulps, a tie that rounds to 770: only entry 1 is above it
        assert q["out"] == [1]
    assert 5 in [e for e, _, _ in r["reloc"]["seen"]["entries"]]
    assert 5 not in [e for e, _, _ in r["loop"]["seen"]["entries"]]    # 0 < minScore = 2^-149


def _sort_size(n_slots):
    p = 1024
    while p < n_slots:
        p *= 2
    return p


def test_census_sweep():
    r = ec.by_tag(ec.ref_answers("sweep"))
    slots = [r["reloc_%d" % n]["seen"]["n_slots"] for n in ec.SWEEP_SLOTS]
    assert slots == ec.SWEEP_SLOTS == [r["loop_%d" % n]["seen"]["n_slots"] for n in ec.SWEEP_SLOTS]
    assert sorted({_sort_size(n) for n in slots}) == [1024, 2048, 4096, 8192]
    for edge in (1024, 2048, 4096):               # each sort's last size and the next one's first
        assert edge in slots and edge + 1 in slots
    for n in ec.SWEEP_SLOTS[4:]:
        for kind in ("reloc", "loop"):
            q = r["%s_%d" % (kind, n)]
            assert len(q["ids"]) > n // 3 and q["out"], (kind, n)
        assert r["reloc_%d" % n]["seen"]["n_db"] <= n
    ops = ec.db_case("sweep")["ops"]
    added = [op[1] for op in ops if op[0] == "add"]
    erased = {op[1] for op in ops if op[0] == "erase"}
    assert added[0] in erased and added[4095] in erased and len(erased) > 4096 // 97
    assert r["reloc_4097"]["seen"]["n_db"] == 4097 - len(erased)   # erased slots stay slots
    named = {i for op in ops if op[0] == "covis" for i in op[2]}
    order = {k: i for i, k in enumerate(added)}
    far = [order[i] for i in named if i in order]
    assert min(far) < 100 and max(far) > 4000
    later = sum(1 for op in ops if op[0] == "covis" and op[1] not in ec.HEAVY
                for i in op[2] if i in order and order[i] > order[op[1]] + 1)
    assert later > 100                            # neighbours named before they are added
    for tag in ("select_reloc", "select_loop"):
        q = r[tag]
        n = len(q["ids"])
        assert n > 2 * ec.SELECT_CHUNK + 1000     # more than three chunks of the select kernel
        chunk = {}
        for (entry, acc, best), pos in zip(q["seen"]["entries"], q["seen"]["entry_pos"]):
            if acc > 2000:                        # the retained ones: every elector of a heavy keyframe
                chunk.setdefault(best, []).append(pos // ec.SELECT_CHUNK)
        assert set(chunk) == set(ec.HEAVY)
        assert 0 in chunk[ec.STAR] and max(chunk[ec.STAR][:-1]) >= 2    # below 1,024 and above 2,048
        assert chunk[ec.MOON_A][:2] == [0, 1] and chunk[ec.MOON_B][0] == 1 and chunk[ec.MOON_C][0] == 2
        elected = q["seen"]["elected"]
        assert elected.count(ec.STAR) >= 3 and len(elected) == sum(len(v) for v in chunk.values())
        assert q["out"] == list(dict.fromkeys(elected)) == [ec.MOON_A, ec.STAR, ec.MOON_B, ec.MOON_C]
        assert q["ids"].tolist()[-4:] == [ec.STAR, ec.MOON_A, ec.MOON_B, ec.MOON_C]


def test_census_query_size():
    case = ec.db_case("query_size")
    assert ec.voc_size(case) >= 9000
    q = {op[1]: op[3] for op in case["ops"] if op[0] in ("reloc", "loop")}
    assert len(q["reloc_8192"][0]) == ec.Q_LDS == len(q["loop_8192"][0])
    assert len(q["reloc_8193"][0]) == ec.Q_LDS + 1 == len(q["loop_8193"][0])
    assert len(q["reloc_9000"][0]) == 9000
    kfs = {op[1]: op[2] for op in case["ops"] if op[0] == "add"}
    assert len(kfs) == 40 and len(kfs[ec.BIG][0]) > ec.Q_LDS
    for tag in ("reloc_8192", "reloc_8193"):
        shared = np.flatnonzero(np.isin(kfs[ec.LATE][0], q[tag][0]))
        assert 128 <= shared[0] < 192             # first shared word in the third 64-word chunk
    r = ec.by_tag(ec.ref_answers("query_size"))
    for tag in q:
        assert r[tag]["out"] and r[tag]["scored"].sum() >= 1, tag
        assert len(r[tag]["ids"]) >= (20 if "small" in tag else 36)
    assert ec.LATE in r["reloc_8192"]["ids"].tolist() and ec.LATE in r["loop_8193"]["ids"].tolist()
    assert ec.BIG2 not in r["loop_8193"]["ids"].tolist()
    assert r["reloc_8192"]["scored"].sum() == 2           # the two big keyframes
    small = r["reloc_small"]
    assert small["out"][0] == 100 and not {ec.BIG, ec.BIG2} & set(small["ids"].tolist())


def test_census_growth():
    case = ec.db_case("growth")
    kfs = [op[2] for op in case["ops"] if op[0] == "add"]
    assert [len(k[0]) for k in kfs] == [1, 5000]  # 4 KiB holds 1,024 words; doubled, 2,048
    r = ec.by_tag(ec.ref_answers("growth"))
    assert r["both"]["ids"].tolist() == [1, 2] and r["both"]["scored"].tolist() == [1, 1]
    assert r["wide"]["ids"].tolist() == [1, 2] and r["wide"]["common"].tolist() == [1, 715]


# ------------------------------------------------------------------ switches
SCORE_SWITCH = {"pairwise": "chain_order", "no_chi_guard": "chi_guard", "no_l2_clamp": "l2_clamp"}
DB_SWITCH = {
    "retain_ge": "retain_thresholds",
    "minscore_gt": "loop_thresholds",
    "best_ge": "tie_own",
    "neigh_minscore": "loop_neighbour_gates",
    "connected_counted": "loop_neighbour_gates",
    "common_ge": "loop_neighbour_gates",
    "best_from_zero": "loop_best_init",
    "neigh_reverse": "neighbour_float_order",
    "order_by_slot": "list_order",
}


def test_every_switch_is_covered():
    assert set(SCORE_SWITCH) | set(DB_SWITCH) == set(ref.SWITCHES)


@pytest.mark.parametrize("switch", sorted(SCORE_SWITCH))
def test_score_switch_changes_the_answer(switch):
    cases = ec.score_case(SCORE_SWITCH[switch])
    want = [ref.score(a, b, s) for s, a, b in cases]
    got = [ref.score(a, b, s, switch) for s, a, b in cases]
    assert not ec.same_doubles(got, want)


@pytest.mark.parametrize("switch", sorted(DB_SWITCH))
def test_rule_switch_changes_the_answer(switch):
    name = DB_SWITCH[switch]
    assert ec.first_difference(ec.ref_answers(name, switch), ec.ref_answers(name)) is not None


@pytest.mark.parametrize("switch", sorted(DB_SWITCH))
def test_switch_shows_in_candidates_or_list(switch):
    """What changes is something the device comparison reads: the candidates or
    lKFsSharingWords, not an accumulator only the restatement exposes."""
    name = DB_SWITCH[switch]
    got, want = ec.ref_answers(name, switch), ec.ref_answers(name)
    assert any(g["out"] != w["out"] or g["ids"].tolist() != w["ids"].tolist()
               for g, w in zip(got, want))


def test_default_switch_is_the_reference():
    for name in ("loop_neighbour_gates", "list_order", "neighbour_float_order"):
        case = ec.db_case(name)
        plain = ec.replay(case, ref.KeyFrameDatabase(ec.voc_size(case), case["scoring"]))
        assert ec.first_difference(plain, ec.ref_answers(name)) is None


# ----------------------------------------------------------------------- cap
def test_no_case_is_left_out():
    """Every builder is a case of the GPU module and of the oracle cross-check,
    by name: neither filters the tables."""
    import test_gpu_placerec_edges as g
    import test_oracle_placerec as o
    assert g.DB_NAMES == list(ec.DB_CASES) == o.DB_NAMES and len(ec.DB_CASES) == 14
    assert g.SCORE_NAMES == list(ec.SCORE_CASES) == o.SCORE_NAMES and len(ec.SCORE_CASES) == 6
    for s in ec.SCORINGS:
        pairs, _ = ec.score_pairs_by_scoring(s)
        assert {n for n, _, _ in pairs} == {n for n in ec.SCORE_CASES
                                            if any(c[0] == s for c in ec.score_case(n))}
    census = {n[len("test_census_"):] for n in globals() if n.startswith("test_census_")}
    assert len(census) >= 19
