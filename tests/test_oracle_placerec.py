"""The two CPU statements of place recognition agree bit for bit: the C++ oracle
with the reference's containers (oracle/placerec_oracle.cpp) and the Python
restatement (tests/placerec_ref.py), on every directed case of
placerec_edge_cases.py and on the natural databases test_gpu_placerec.py builds.
Doubles and floats by bit pattern, any NaN equal to any NaN, lists and
candidates in order.  No GPU needed."""
import numpy as np
import pytest

import placerec_edge_cases as ec
import placerec_ref as ref
import test_gpu_placerec as nat

DB_NAMES = list(ec.DB_CASES)
SCORE_NAMES = list(ec.SCORE_CASES)


# --------------------------------------------------------------------- score
@pytest.mark.parametrize("name", SCORE_NAMES)
def test_directed_scores(oracle, name):
    cases = ec.score_case(name)
    want = [ref.score(a, b, s) for s, a, b in cases]
    got = [oracle.bow_score(a, b, s) for s, a, b in cases]
    assert ec.same_doubles(got, want)
    # the first vector is v1: swapped, the answer is the restatement's swapped answer
    got = [oracle.bow_score(b, a, s) for s, a, b in cases]
    assert ec.same_doubles(got, [ref.score(b, a, s) for s, a, b in cases])


@pytest.mark.parametrize("scoring", nat.SCORINGS)
def test_natural_score_pairs(oracle, scoring):
    _, al, bl, want = nat.score_pairs(oracle, scoring)
    got = [oracle.bow_score(a, b, scoring) for a, b in zip(al, bl)]
    assert ec.same_doubles(got, want)


def test_kl_is_not_restated(oracle):
    a = ec.bow([1], [1.0])
    with pytest.raises(ValueError):
        oracle.bow_score(a, a, ref.KL)
    with pytest.raises(ValueError):
        oracle.KeyFrameDatabase(10, ref.KL)


# ------------------------------------------------------------------ database
def _inspect_oracle(tag, db):
    return dict(min_common=db.last_min_common, elected=db.last_elected, n_db=len(db))


@pytest.mark.parametrize("name", DB_NAMES)
def test_directed_database(oracle, name):
    case = ec.db_case(name)
    want = ec.ref_answers(name)
    got = ec.replay(case, oracle.KeyFrameDatabase(ec.voc_size(case), case["scoring"]), _inspect_oracle)
    assert ec.first_difference(got, want) is None
    for g, w in zip(got, want):
        for k in ("min_common", "elected", "n_db"):
            assert g["seen"][k] == w["seen"][k], (w["tag"], k)


class Both:
    """The restatement and the oracle driven in step, with the methods of
    test_gpu_placerec.Pair."""

    def __init__(self, oracle, v, scoring=0):
        n = int(v["leaf"].sum())
        self.ref = ref.KeyFrameDatabase(n, scoring)
        self.db = oracle.KeyFrameDatabase(n, scoring)

    def add(self, kf_id, bow):
        self.ref.add(kf_id, bow)
        self.db.add(kf_id, bow)

    def erase(self, kf_id):
        self.ref.erase(kf_id)
        self.db.erase(kf_id)

    def clear(self):
        self.ref.clear()
        self.db.clear()

    def covis(self, kf_id, ids):
        self.ref.set_covisibility(kf_id, ids)
        self.db.set_covisibility(kf_id, ids)

    def _check(self, got, want):
        ids, common, scores, scored = self.db.last_query()
        rids, rcommon, rscores, rscored = self.ref.last_query()
        assert np.array_equal(ids, rids) and np.array_equal(common, rcommon)
        assert np.array_equal(scored, rscored) and ec.same_floats(scores, rscores)
        assert len(self.db) == len(self.ref.kfs)
        assert self.db.last_min_common == self.ref.last_min_common
        assert got == want
        if want:
            assert self.db.last_elected == self.ref.last_elected
        return want

    def reloc(self, qid, bow):
        return self._check(self.db.DetectRelocalizationCandidates(qid, bow),
                           self.ref.DetectRelocalizationCandidates(qid, bow))

    def loop(self, qid, bow, connected, min_score):
        return self._check(self.db.DetectLoopCandidates(qid, bow, connected, min_score),
                           self.ref.DetectLoopCandidates(qid, bow, connected, min_score))


@pytest.mark.parametrize("L", [3, 4])
def test_natural_relocalization(oracle, L):
    v, kfs, covis = nat.keyframes(oracle, L)
    p = Both(oracle, v)
    nat._fill(p, kfs, covis)
    for q in range(3):
        assert p.reloc(q + 1, nat._bow(oracle, v, [300, 40, 1000][q], 7000 + q))
    assert kfs[5][0] in p.reloc(9, kfs[5][1])


@pytest.mark.parametrize("scoring", [ref.L2_NORM, ref.CHI_SQUARE, ref.BHATTACHARYYA,
                                     ref.DOT_PRODUCT])
def test_natural_other_scoring_types(oracle, scoring):
    v = nat._tree(3, 43)
    p = Both(oracle, v, scoring)
    rng = np.random.default_rng(scoring)
    ids = list(range(1, 61))
    for i in ids:
        p.add(i, nat._bow(oracle, v, int(rng.integers(30, 200)), 50 + i, scoring))
    for i in ids:
        p.covis(i, rng.choice(ids, 4, replace=False))
    assert p.reloc(1, nat._bow(oracle, v, 150, 999, scoring))
    assert p.loop(1, nat._bow(oracle, v, 150, 998, scoring), ids[:5], 0.0)


def test_natural_loop_and_stale(oracle):
    v, kfs, covis = nat.keyframes(oracle, 3, seed=3)
    p = Both(oracle, v)
    nat._fill(p, kfs, covis)
    q = nat._bow(oracle, v, 400, 8200)
    connected = [kf_id for kf_id, _ in kfs[10:25]] + [424242]
    min_score = float(min(np.float32(1), np.float32(min(ref.score(q, b) for _, b in kfs[10:25]))))
    out = p.loop(1, q, connected, min_score)
    assert out and not set(out) & set(connected)
    assert p.loop(2, q, connected, 2.0) == []
    assert p.loop(3, q, [], 0.0)
    assert p.reloc(3, q)
    # a small query after a wide one: neighbours carry the wide query's scores
    assert p.reloc(4, kfs[17][1])


def test_natural_mutation(oracle):
    v, kfs, covis = nat.keyframes(oracle, 3, n_kf=120, seed=2)
    p = Both(oracle, v)
    nat._fill(p, kfs, covis)
    q = nat._bow(oracle, v, 300, 8100)
    p.reloc(1, q)
    with pytest.raises(ValueError):                 # already present
        p.db.add(kfs[0][0], kfs[0][1])
    gone = kfs[::3]
    for kf_id, _ in gone:
        p.erase(kf_id)
    p.erase(123456789)
    assert len(p.db) == len(kfs) - len(gone)
    p.reloc(2, q)
    for kf_id, bow in gone[::2][::-1]:
        p.add(kf_id, bow)
    p.covis(gone[0][0], [kfs[1][0], kfs[2][0]])
    p.reloc(3, q)
    p.loop(4, q, [kfs[1][0]], 0.0)
    p.clear()
    assert len(p.db) == 0 and p.reloc(5, q) == [] and len(p.db.last_query()[0]) == 0
    for kf_id, bow in kfs[:10]:
        p.add(kf_id, bow)
    assert p.reloc(6, q)


def test_natural_many_small_keyframes(oracle):
    v = nat._tree(3, 43)
    p = Both(oracle, v)
    rng = np.random.default_rng(11)
    n = 4300
    for i in range(n):
        w = np.sort(rng.choice(64, int(rng.integers(1, 4)), replace=False)).astype(np.uint32)
        p.add(i + 1, (w, np.full(len(w), 1.0 / len(w))))
    for i in range(0, n, 9):
        p.covis(i + 1, rng.integers(1, n + 1, 10))
    q = (np.arange(0, 64, 3, dtype=np.uint32), np.full(22, 1.0 / 22))
    assert p.reloc(1, q)
    assert p.loop(1, q, [5, 6, 7], 0.0)


def test_both_libraries_carry_the_oracle(oracle):
    import ctypes
    for name in ("liborb_oracle.so", "liborb_oracle_glibc.so"):
        L = ctypes.CDLL(str(oracle.HERE / name))
        for sym in ("oracle_bow_score", "oracle_kfdb_create", "oracle_kfdb_detect_loop",
                    "oracle_kfdb_detect_relocalization", "oracle_kfdb_last_elected"):
            assert hasattr(L, sym), (name, sym)
