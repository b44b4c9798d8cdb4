"""Known answers for tests/placerec_ref.py (the restatement the GPU
place-recognition tests compare against), worked out by hand, and the export /
binding check of the new C-ABI entry points.  No GPU needed."""
import math
import subprocess

import numpy as np

import placerec_ref as ref

NEW_SYMBOLS = [
    "orb_vocabulary_score", "orb_vocabulary_score_batch", "orb_kf_database_create",
    "orb_kf_database_destroy", "orb_kf_database_clear", "orb_kf_database_size",
    "orb_kf_database_add", "orb_kf_database_erase", "orb_kf_database_set_covisibility",
    "orb_kf_database_detect_relocalization", "orb_kf_database_detect_loop",
    "orb_kf_database_last_query", "orb_kf_database_profile",
]


def test_l1_identical_vectors_score_one():
    """score += |v - v| - |v| - |v| = -2v per word: -1, -0.5, -0.5 -> -2; -(-2)/2 = 1."""
    a = ([3, 8, 20], [0.5, 0.25, 0.25])
    assert ref.score(a, a) == 1.0


def test_l1_disjoint_vectors_score_zero():
    a = ([1, 4, 9], [0.5, 0.25, 0.25])
    b = ([2, 5, 10], [0.25, 0.25, 0.5])
    assert ref.score(a, b) == 0.0
    assert ref.score(a, ([], [])) == 0.0 and ref.score(([], []), ([], [])) == 0.0


def test_l1_three_word_example():
    """a = {1: .5, 3: .25, 7: .25}, b = {1: .25, 4: .5, 7: .25}.  Common words 1 and 7:
    word 1: |.5 - .25| - .5 - .25 = -.5;  word 7: |0| - .25 - .25 = -.5;
    sum -1, score = -(-1) / 2 = 0.5.  The other scoring types on the same pair:
    sum v*w = .125 + .0625 = .1875 (dot); L2 = 1 - sqrt(1 - .1875);
    chi = 2 (.125/.75 + .0625/.5); Bhattacharyya = sqrt(.125) + .25."""
    a = ([1, 3, 7], [0.5, 0.25, 0.25])
    b = ([1, 4, 7], [0.25, 0.5, 0.25])
    assert ref.score(a, b) == 0.5 and ref.score(b, a) == 0.5
    assert ref.score(a, b, ref.DOT_PRODUCT) == 0.1875
    assert ref.score(a, b, ref.L2_NORM) == 1.0 - math.sqrt(0.8125)
    assert ref.score(a, b, ref.CHI_SQUARE) == 2. * (0.125 / 0.75 + 0.0625 / 0.5)
    assert ref.score(a, b, ref.BHATTACHARYYA) == math.sqrt(0.125) + 0.25


def _three_kf_db():
    db = ref.KeyFrameDatabase(10)
    db.add(10, ([2, 5], [0.5, 0.5]))
    db.add(11, ([1, 2, 5], [0.5, 0.25, 0.25]))
    db.add(12, ([5], [1.0]))
    db.set_covisibility(10, [11])
    db.set_covisibility(11, [10, 12])
    return db


QA = ([1, 2, 5], [0.25, 0.25, 0.5])
QB = ([5], [1.0])


def test_three_keyframe_database_by_hand():
    """Keyframes added in the order 10 {2, 5}, 11 {1, 2, 5}, 12 {5}; the inverted
    file is word 1: [11], word 2: [10, 11], word 5: [10, 11, 12].
    Query QA = {1: .25, 2: .25, 5: .5}: word 1 meets 11 first, word 2 meets 10,
    word 5 meets 12, so the list is [11, 10, 12] (not the add order) with 3, 2, 1
    common words.  maxCommonWords 3, minCommonWords = (int)(3 * 0.8f) = 2, so only
    11 is scored: terms |.25-.5|-.25-.5, |0|-.25-.25, |.5-.25|-.5-.25 = -.5 each,
    score 0.75.  Its neighbours 10 and 12 share but were never scored (0): acc
    0.75, best 11; 0.75 > 0.75 * 0.75, so the result is [11]."""
    db = _three_kf_db()
    assert db.DetectRelocalizationCandidates(1, QA) == [11]
    ids, words, scores, scored = db.last_query()
    assert ids.tolist() == [11, 10, 12] and words.tolist() == [3, 2, 1]
    assert scored.tolist() == [1, 0, 0] and scores.tolist() == [0.75, 0.0, 0.0]
    assert db.last_min_common == 2


def test_three_keyframe_database_stale_scores_by_hand():
    """Query QB = {5: 1} first: the list is word 5's list [10, 11, 12], one common
    word each, minCommonWords = (int)(1 * 0.8f) = 0, all scored: 0.5, 0.25, 1.0.
    Entry 10 (neighbour 11): acc .75, best 10.  Entry 11 (neighbours 10, 12): acc
    1.75, best 12.  Entry 12: acc 1, best 12.  Retain > 0.75 * 1.75 = 1.3125:
    entry 11 only, which elects 12.
    Then QA: only 11 is scored (0.75), but its neighbours 10 and 12 share, so
    their scores from the first query are read: acc .75 + .5 + 1 = 2.25, best 12
    (1.0 > .75): the result is [12], a keyframe this query never scored."""
    db = _three_kf_db()
    assert db.DetectRelocalizationCandidates(1, QB) == [12]
    ids, words, scores, scored = db.last_query()
    assert ids.tolist() == [10, 11, 12] and words.tolist() == [1, 1, 1]
    assert scores.tolist() == [0.5, 0.25, 1.0] and scored.tolist() == [1, 1, 1]
    assert db.DetectRelocalizationCandidates(2, QA) == [12]
    ids, words, scores, scored = db.last_query()
    assert ids.tolist() == [11, 10, 12] and scored.tolist() == [1, 0, 0]
    assert scores.tolist() == [0.75, 0.5, 1.0]


def test_three_keyframe_database_loop_by_hand():
    """QB as a loop query with keyframe 12 connected and minScore 0.3: the list
    is [10, 11], both scored (0.5, 0.25); 11 falls below minScore.  Entry 10:
    neighbour 11 shares with 1 > 0 words, acc .75, best 10 -> [10].  With
    minScore 0.6 nothing is left.  Erasing 10 takes it out of every list."""
    db = _three_kf_db()
    assert db.DetectLoopCandidates(5, QB, [12], 0.3) == [10]
    assert db.last_query()[0].tolist() == [10, 11]
    assert db.DetectLoopCandidates(6, QB, [12], 0.6) == []
    db.erase(10)
    assert db.DetectLoopCandidates(7, QB, [], 0.0) == [12]
    assert db.last_query()[0].tolist() == [11, 12]


def test_threshold_is_float_multiply_then_truncation():
    f = lambda m: int(np.float32(m) * np.float32(0.8))
    assert [f(5), f(10), f(15)] == [4, 8, 12] and f(3) == 2 and f(1) == 0


def test_library_exports_and_binds_place_recognition(orb):
    L = orb.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", str(orb.LIB_PATH)], check=True,
                         capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    missing = [s for s in NEW_SYMBOLS if s not in exported]
    assert not missing, f"not exported: {missing}"
    for s in NEW_SYMBOLS:
        assert getattr(L, s).argtypes is not None, f"{s} not bound in the ctypes table"
    assert hasattr(orb, "KeyFrameDatabase") and hasattr(orb.ORBVocabulary, "score")
    assert hasattr(orb.ORBVocabulary, "score_pairs")
    blob = orb.LIB_PATH.read_bytes()
    for k in (b"k_bow_score", b"k_db_common", b"k_db_list", b"k_db_score", b"k_db_accumulate",
              b"k_db_select"):
        assert k in blob
