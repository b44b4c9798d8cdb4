"""tests/bow_batch_ref.py against hand-computable inputs and the Python
reference, and the census of the inputs tests/test_gpu_bow_batch.py runs: that
they match at all, that the gate's two sides and the rotation filter are met,
and that the node sizes straddle the 64-lane trip."""
import functools

import numpy as np

import bow_batch_ref as B
import matcher_edge_cases as E
import pyref
import scenarios as S

NATURAL = ((3, 200), (40, 200), (41, 200), (5, 60))


@functools.lru_cache(maxsize=None)
def natural(oracle, seed, nf):
    return B.from_bow(S.bow_pair(oracle, seed, nf=nf))


def test_helper_reproduces_the_edge_cases_own_expectation(oracle):
    for c in (E.bow_case("frame"), E.bow_case("frame", ties=True)) + tuple(
            E.hist_bow(s) for s in E.HIST_SHAPES):
        p = B.from_bow(c)
        km, info = B.expected(oracle, p, c["nnratio"], c["check_ori"])
        assert np.array_equal(km, c["expect"]) and info[0] == c["n_expect"]
        assert info[1] >= info[0] and info[4] == 1
        # through the packed slots (stride above the counts, junk behind them)
        stride = max(len(p["kf"]["desc"]), len(p["f"]["desc"])) + 5
        a, b = B.pack_slots([p["kf"]], stride), B.pack_slots([p["f"]], stride)
        km2, info2 = B.expected_slot(oracle, a, 0, b, 0, stride, p["points"], c["nnratio"],
                                     c["check_ori"])
        assert np.array_equal(km2, km) and info2 == info


def test_helper_agrees_with_the_python_reference(oracle):
    c = S.bow_pair(oracle, 3, nf=200)
    p = B.from_bow(c)
    for ratio, ori in ((0.7, True), (0.9, False)):
        km, info = B.expected(oracle, p, ratio, ori)
        n, fm = pyref.search_by_bow(c["kf_desc"], c["kf_angle"], c["kf_mp"], c["kf_bad"],
                                    c["kf_fv"], c["f_desc"], c["f_angle"], c["f_fv"], ratio, ori)
        assert n == info[0] and np.array_equal(fm, km)
    # the counts a few lines of numpy give
    knodes, koffs, kfeats = c["kf_fv"]
    common = [a for a in range(len(knodes)) if knodes[a] in set(c["f_fv"][0].tolist())]
    tried = sum(1 for a in common for i in kfeats[koffs[a]:koffs[a + 1]]
                if c["kf_mp"][i] >= 0 and not c["kf_bad"][i])
    assert info[2] == len(common) and info[3] == tried


def test_malformed_rule_and_clamps(oracle):
    p = natural(oracle, 5, 60)
    stride = max(len(p["kf"]["desc"]), len(p["f"]["desc"])) + 20
    a, b = B.pack_slots([p["kf"]], stride), B.pack_slots([p["f"]], stride)
    good = B.expected_slot(oracle, a, 0, b, 0, stride, p["points"], 0.7, True)
    assert good[1][0] > 0
    nf = int(b["nkeys"][0])
    for edit in ("feat", "last", "decrease"):
        bb = {k: v.copy() for k, v in b.items()}
        nn = int(bb["n_fv_nodes"][0])
        if edit == "feat":
            bb["fv_feats"][3] = nf
        elif edit == "last":
            bb["fv_offs"][nn] = nf + 1
        else:
            bb["fv_offs"][2] = bb["fv_offs"][1] - 1
        km, info = B.expected_slot(oracle, a, 0, bb, 0, stride, p["points"], 0.7, True)
        assert info == B.MALFORMED and len(km) == nf and (km == -1).all()
    bb = {k: v.copy() for k, v in b.items()}
    bb["n_fv_nodes"][0] = -3
    assert B.expected_slot(oracle, a, 0, bb, 0, stride, p["points"], 0.7, True)[1][:4] == (0, 0, 0, 0)


def test_census_of_the_gpu_inputs(oracle):
    counts = {}
    filtered = 0
    for seed, nf in NATURAL[:3]:
        _, info = B.expected(oracle, natural(oracle, seed, nf), 0.7, True)
        counts[seed] = info[0]
        filtered += info[1] - info[0]
        assert info[0] >= 30, (seed, info)           # a natural problem matches
    assert counts == {3: 52, 40: 53, 41: 44}   # bow_pair's defaults, ratio 0.7, filter on
    assert filtered > 0                               # the rotation filter removes something
    big = B.expected(oracle, B.from_bow(S.bow_pair(oracle, 3, nf=1000)), 0.7, True)[1]
    assert 250 <= big[0] <= 360 and big[1] > big[0]
    # relocalisation: one frame against keyframes of four sequences
    frame = natural(oracle, 3, 200)["f"]
    reloc = [B.expected(oracle, dict(natural(oracle, s, 200), f=frame), 0.7, True)[1][0]
             for s in (3, 40, 41, 42)]
    assert reloc == [52, 2, 3, 3]
    assert all(n < 15 for n in reloc[1:])            # the unrelated pairs fail the gate
    # the gate's two sides
    for n in (14, 15):
        q = B.thin_to(oracle, natural(oracle, 3, 200), n, 0.7, True)
        assert B.expected(oracle, q, 0.7, True, 15)[1][4] == int(n >= 15)
    # node sizes around the 64-lane trip
    sizes = np.diff(E.bow_case("frame")["f_fv"][1])
    assert set(E.NODE_SIZES) <= set(sizes.tolist()) and set(E.NODE_SIZES) == {1, 63, 64, 65, 128,
                                                                              129, 200}
