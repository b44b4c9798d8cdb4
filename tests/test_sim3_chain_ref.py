"""The reference side of the ComputeSim3 matcher batches (tests/sim3_chain_ref.py)
on the CPU: the oracle-based and the pyref-based references agree on the inputs
the GPU tests use, the helpers give hand-computed answers on a five-keypoint
case, the directed inputs hold their census, and the chain scene has what the
chain test needs (more than 40 BoW matches, more than 10 added by SearchBySim3,
a gated candidate and one without a Sim3 in the first round)."""
import numpy as np

import bow_batch_ref as B
import matcher_edge_cases as E
import pyref
import sim3_chain_cases as C
import sim3_chain_ref as R

f32 = np.float32


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return all(np.array_equal(x, y) for x, y in zip(a[:-1], b[:-1])) and a[-1] == b[-1]


def test_oracle_and_pyref_agree_on_every_bow_input(oracle):
    """Every BoW set the GPU tests run (sim3_chain_cases.all_bow_sets): directed
    nodes, ties, histogram shapes, natural pairs, empty sides, bad and NULL points,
    no point array, the gate's thinned sides, the mixed batches, malformed slots,
    both strides."""
    tags = []
    for tag, c in C.all_bow_sets(oracle):
        arr, stride = C.bow_pack(c)
        a = C.bow_refs(oracle, c, arr, stride)
        b = C.bow_refs(oracle, c, arr, stride, pyref.search_by_bow_kf)
        assert len(a) == len(c["pairs"]) and all(_same(x, y) for x, y in zip(a, b)), tag
        tags.append(tag)
    assert len(tags) == 27
    gate = C.bow_refs(oracle, C.bow_gate_set(oracle), *C.bow_pack(C.bow_gate_set(oracle)))
    assert [g[2][0] for g in gate] == [19, 20] and [g[2][4] for g in gate] == [0, 1]


def test_oracle_and_pyref_agree_on_every_sim3_input(oracle):
    """Every SearchBySim3 set the GPU tests run (sim3_chain_cases.all_search_sets):
    the crowded keyframes, 99 / 100 / 101 with the projection on max_x and the
    first-minimum tie, empty keyframes, 0 .. 257 keypoints, one cell, the borders,
    the natural similarities, the inlier filters and odd index2 entries, the
    mixed batches with skipped problems, both strides, identity slots."""
    tags = []
    for tag, c in C.all_search_sets(oracle):
        arr = C.search_pack(c)
        a = C.search_refs(oracle, c, arr)
        b = C.search_refs(oracle, c, arr, pyref.search_by_sim3)
        assert len(a) == len(c["probs"]) and all(_same(x, y) for x, y in zip(a, b)), tag
        tags.append(tag)
    assert len(tags) == 20
    thr = C.search_thresholds_set()
    got = C.search_refs(oracle, thr, C.search_pack(thr))[0][2]
    assert np.array_equal(got, E.by_sim3_thresholds()["expect"])


def test_oracle_and_pyref_agree_on_the_chain_scene(oracle):
    sides, pairs, points, mp_desc, host, draws = R.chain_scene(oracle)
    a = R.chain_reference(oracle, sides, pairs, points, mp_desc, host, draws, rounds=2,
                          optimise=False)
    b = R.chain_reference(oracle, sides, pairs, points, mp_desc, host, draws, rounds=2,
                          optimise=False, second=(pyref.search_by_bow_kf, pyref.search_by_sim3))
    for x, y in zip(a, b):
        assert _same(x["bow"], y["bow"])
        assert np.array_equal(x["match12"], y["match12"]) and np.array_equal(x["index2"], y["index2"])
        for rx, ry in zip(x["rounds"], y["rounds"]):
            assert rx["result"].tobytes() == ry["result"].tobytes()
            assert _same(rx["search"], ry["search"])


def test_helpers_on_a_five_keypoint_case():
    m12 = np.array([10, 11, -1, 12, 13], np.int32)
    ix2 = np.array([0, 7, -1, -1, 2], np.int32)       # 7: outside KF2's three keypoints
    # the filter: entries 1 and 4 are no inliers
    fm, fx = R.filter_rows(m12, ix2, np.array([1, 0, 1, 9, 0], np.uint8))
    assert fm.tolist() == [10, -1, -1, 12, -1] and fx.tolist() == [0, -1, -1, -1, -1]
    assert R.filter_rows(m12, ix2, None)[0].tolist() == m12.tolist()
    # the masks: an index2 out of range (7) or negative marks nothing in KF2
    a1, a2 = R.already_masks(m12, ix2, 3)
    assert a1.tolist() == [1, 1, 0, 1, 1] and a2.tolist() == [1, 0, 1]
    a1, a2 = R.already_masks(fm, fx, 3)
    assert a1.tolist() == [1, 0, 0, 1, 0] and a2.tolist() == [1, 0, 0]
    # the merge: this call matched keypoint 1 to KF2's 2 and keypoint 2 to KF2's 1
    pidx2 = np.array([10, 14, 13], np.int32)
    om, ox = R.merge(fm, fx, np.array([-1, 2, 1, -1, -1], np.int32), pidx2)
    assert om.tolist() == [10, 13, 14, 12, -1] and ox.tolist() == [0, 2, 1, -1, -1]
    # index2 from ids, and the gate at 19 / 20
    assert R.rows_from_ids(np.array([13, -1, 10], np.int32), pidx2).tolist() == [2, -1, 0]
    row = np.arange(5, dtype=np.int32)
    g19, g20 = R.gate(row, row, 19, 20), R.gate(row, row, 20, 20)
    assert g19[2] == 0 and (g19[0] == -1).all() and (g19[1] == -1).all()
    assert g20[2] == 1 and g20[0] is row and g20[1] is row


def test_census_of_the_directed_inputs():
    c = E.by_sim3_case()
    cen = E.census_mutual(c)
    assert cen["one_way"] >= 10 and cen["mutual"] >= 20, cen
    cen = E.census_nodes(E.bow_case("kf"))
    assert set(E.NODE_SIZES) <= set(cen["sizes"]) and cen["max_size"] == 200, cen
    assert all(cen["best_at"][d] >= 1 for d in (49, 50, 51)), cen
    assert cen["best_beyond_first_trip"] >= 1, cen
    cen = E.census_nodes(E.bow_case("kf", ties=True))
    assert cen["ties_same_trip"] >= 1 and cen["ties_cross_trip"] >= 1, cen


def test_chain_scene_has_what_the_chain_needs(oracle):
    sides, pairs, points, mp_desc, host, draws = R.chain_scene(oracle)
    ref = R.chain_reference(oracle, sides, pairs, points, mp_desc, host, draws, rounds=1)
    assert ref[0]["bow"][2][0] > 40                           # SearchByBoW
    assert ref[0]["rounds"][0]["search"][3][0] > 10           # SearchBySim3 adds
    assert any(r["bow"][2][4] == 0 for r in ref)              # a gated candidate
    assert any(r["bow"][2][4] == 1 and not int(r["rounds"][0]["result"]["has_sim3"]) for r in ref)
    gated = next(r for r in ref if r["bow"][2][4] == 0)
    assert (gated["match12"] == -1).all() and int(gated["rounds"][0]["result"]["no_more"]) == 1
