"""Directed inputs for place recognition (test infrastructure): BoW score pairs
and keyframe-database scripts built so that tests/placerec_ref.py reaches what
the natural inputs of test_gpu_placerec.py never do -- the 2048- and 4096-key
LDS sorts of k_db_list with every slot boundary beside them, the unstaged query
path of k_db_common and its 8192 / 8193 boundary, k_db_select over more than
two chunks with a keyframe elected on both sides of a chunk edge, every exact
comparison of src/KeyFrameDatabase.cc at equality, and the guard, the clamp and
the chain order of ScoringObject.cpp.

Values are dyadic rationals wherever a score must be exact.  Under L1 a common
word of positive values adds min(vi, wi) to the score (|vi - wi| - vi - wi =
-2 min, halved and negated), exactly; a BowVector need not be normalised for
the reference to score it.  The standard query Q8 is eight words of 0.125.

SCORE_CASES maps a name to a builder returning a list of (scoring, a, b).
DB_CASES maps a name to a builder returning dict(L, scoring, ops): a script of
    ("add", id, bow) ("erase", id) ("covis", id, ids) ("clear",)
    ("reloc", tag, query id, bow) ("loop", tag, query id, bow, connected, minScore)
on a k = 10 tree of depth L, replayed by `replay` against any database with the
interface of placerec_ref.KeyFrameDatabase (the restatement, the oracle, the
device).  Every case is built once and cached; none is ever skipped or
filtered: tests/test_placerec_edge_cases.py asserts the census of each."""
from __future__ import annotations

import functools

import numpy as np

import placerec_ref as ref

f32 = np.float32
L1, L2, CHI, BHAT, DOT = ref.L1_NORM, ref.L2_NORM, ref.CHI_SQUARE, ref.BHATTACHARYYA, ref.DOT_PRODUCT
SCORINGS = [L1, L2, CHI, BHAT, DOT]
NONE_WORD = 0xFFFFFFFF          # the kernels' "no word" sentinel; a legal WordId for score()
Q_LDS = 8192                    # PR_Q_LDS: query words k_db_common stages in LDS
SELECT_CHUNK = 1024             # threads of k_db_select
SWEEP_SLOTS = [1, 3, 4, 5, 1023, 1024, 1025, 2048, 2049, 4095, 4096, 4097]


def bow(words, values):
    w = np.asarray(words, np.uint32)
    v = np.asarray(values, np.float64)
    assert len(w) == len(v) and (len(w) < 2 or (np.diff(w.astype(np.int64)) > 0).all())
    return w, v


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def bits32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def same_doubles(got, want):
    """Bit patterns equal, any NaN equal to any NaN."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(bits64(got)[~nan], bits64(want)[~nan])


def same_floats(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(bits32(got)[~nan], bits32(want)[~nan])


# ------------------------------------------------------------- score cases
def _b65():
    return np.arange(65, dtype=np.uint32) * 10 + 10      # 10, 20, .. 650


def chunk_positions():
    """b of 65 words (one full wave chunk and one lane of the next) whose only
    common words sit at positions 0, 63 and 64; a of length 1 on each of them;
    a common word that ends both vectors; the two largest word ids."""
    bw = _b65()
    bv = np.full(65, 0.25)
    bv[[0, 63, 64]] = [0.5, 0.125, 0.0625]
    b = bow(bw, bv)
    a = bow([5, 10, 15, 25, 640, 645, 650, 655], [0.125, 0.25, 0.125, 0.125, 0.25, 0.0625, 0.03125, .03125])
    out = []
    for s in SCORINGS:
        out.append((s, a, b))
        out.append((s, b, a))
        for pos in (0, 63, 64):
            out.append((s, bow([bw[pos]], [0.25]), b))
        out.append((s, bow([1, 3, 500], [0.25, 0.25, 0.5]), bow([2, 4, 6, 500], [0.5, 0.125, 0.125, 0.25])))
        out.append((s, bow([5, NONE_WORD - 1, NONE_WORD], [0.5, 0.25, 0.25]),
                    bow([NONE_WORD - 1, NONE_WORD], [0.5, 0.5])))
        out.append((s, bow([7, NONE_WORD], [0.5, 0.5]), bow([5, 7, NONE_WORD - 1, NONE_WORD], [.25, .25, .25, .25])))
    return out


CHAIN_DOT = [1e16, 1.0, -1e16, 1.0, 3.0, 1e-3]            # chain 4.001, reversed 4.0, pairwise 3.001
_T = 3.0 * 2.0 ** 48
CHAIN_L2 = [_T, 2.0 ** -4, -_T, 2.0 ** -4, 0.25, 2.0 ** -10]   # all three below 1 and different


def chain_order():
    """Terms of very different magnitude on the common words, which sit at
    positions 61..66 of b: the chain crosses the 64-lane boundary.  b's other
    words are not in a."""
    out = []
    for s, terms in ((DOT, CHAIN_DOT), (L2, CHAIN_L2)):
        bw = np.arange(70, dtype=np.uint32) * 2 + 2
        bv = np.full(70, 1.0)
        aw = np.concatenate([[1, 3], bw[61:67], [501]]).astype(np.uint32)
        av = np.concatenate([[7.0, 9.0], terms, [11.0]])
        out.append((s, bow(aw, av), bow(bw, bv)))
    return out


def chain_terms(case):
    """vi * wi of the common words of a dot-product / L2 pair, in word order."""
    _, a, b = case
    return [x * y for x, y in ref._common(a, b)]


def chi_guard():
    """Common words whose values sum to zero -- (0, 0), (x, -x), (-0, 0) --
    between ordinary terms, and a pair in which every common word is guarded."""
    w = [2, 4, 6, 8, 10, 12]
    a = bow(w, [0.5, 0.0, 0.25, 0.375, -0.0, 0.5])
    b = bow(w, [0.5, 0.0, 0.25, -0.375, 0.0, 0.25])
    g = bow([2, 4, 6, 9], [0.0, 0.375, -0.0, 1.0])
    h = bow([2, 4, 6, 11], [0.0, -0.375, 0.0, 1.0])
    return [(CHI, a, b), (CHI, b, a), (CHI, g, h)]


def l2_clamp():
    """Sums of exactly 1, 1 + 2^-52 and 1 - 2^-53."""
    one = bow([1, 2, 3, 4], [0.5, 0.5, 0.5, 0.5])
    return [(L2, one, one),
            (L2, bow([3], [1.0 + 2.0 ** -52]), bow([3], [1.0])),
            (L2, bow([3], [1.0 - 2.0 ** -53]), bow([3], [1.0])),
            (L2, bow([3, 5], [1.0, 0.5]), bow([3, 5], [1.0, 2.0 ** -52]))]


def signs_nonfinite():
    """Negative and zero values under L1, a negative product under
    Bhattacharyya (NaN), an infinite value, and no common word under L1 (-0.0)."""
    w = [1, 5, 9]
    neg = bow(w, [-0.5, 0.0, 0.25])
    pos = bow(w, [0.25, 0.5, -0.25])
    inf = bow(w, [float("inf"), 0.5, 0.25])
    out = [(L1, neg, pos), (L1, pos, neg), (L1, neg, neg), (BHAT, neg, pos), (BHAT, pos, pos),
           (L1, inf, pos), (DOT, inf, pos), (L2, inf, pos), (CHI, inf, pos), (BHAT, inf, inf),
           (L1, bow([1, 3], [0.5, 0.5]), bow([2, 4], [0.5, 0.5]))]
    for s in SCORINGS:
        out.append((s, bow([1, 3], [0.5, 0.5]), bow([2, 4], [0.5, 0.5])))
    return out


def empties():
    """An empty a and an empty b, to sit in the middle of a batch."""
    e = bow([], [])
    x = bow([1, 2], [0.5, 0.5])
    out = []
    for s in SCORINGS:
        out += [(s, x, x), (s, e, x), (s, x, e), (s, e, e), (s, x, x)]
    return out


SCORE_CASES = {
    "chunk_positions": chunk_positions,
    "chain_order": chain_order,
    "chi_guard": chi_guard,
    "l2_clamp": l2_clamp,
    "signs_nonfinite": signs_nonfinite,
    "empties": empties,
}
PAIR_COUNTS = [1, 4, 5]   # k_bow_score takes four pairs per workgroup


@functools.lru_cache(maxsize=None)
def score_case(name):
    return SCORE_CASES[name]()


@functools.lru_cache(maxsize=None)
def score_pairs_by_scoring(scoring):
    """Every score case of one scoring type, in SCORE_CASES order (the empties
    land in the middle of the batch), with the restatement's answers."""
    pairs = [(n, a, b) for n in SCORE_CASES for s, a, b in score_case(n) if s == scoring]
    want = np.array([ref.score(a, b, scoring) for _, a, b in pairs], np.float64)
    return pairs, want


# ---------------------------------------------------------- database cases
Q8 = bow(range(8), [0.125] * 8)


def kf8(values, extra=()):
    """A keyframe on Q8's words: values[i] for word i (None: word absent), plus
    words Q8 does not hold."""
    w = [i for i, v in enumerate(values) if v is not None] + list(extra)
    x = [v for v in values if v is not None] + [0.25] * len(extra)
    return bow(w, x)


E = 0.125
FULL = kf8([E] * 8)                                   # 8 common, 1.0
S875 = kf8([E] * 7 + [None], extra=[20])              # 7 common, 0.875
S750 = kf8([E] * 6 + [0.0, None])                     # 7 common (one of value 0), 0.75
S625 = kf8([E] * 5 + [0.0, 0.0, None])                # 7 common, 0.625
S250 = kf8([E] * 2 + [0.0] * 5 + [None])              # 7 common, 0.25
C6 = kf8([E] * 6 + [None, None], extra=[21, 22])      # 6 common = minCommonWords of 8
UP = float(np.nextafter(f32(0.875), f32(1)))


def loop_thresholds():
    """maxCommonWords 8, minCommonWords 6.  si == minScore is kept, minScore one
    float above drops it; with the 1.0 keyframe connected every accScore equals
    minScore, bestAccScore stays at its start and the entry is still retained;
    minScore above every score returns nothing."""
    ops = [("add", 1, FULL), ("add", 2, S875), ("add", 3, S750), ("add", 4, C6),
           ("loop", "equal", 1, Q8, [], 0.875),
           ("loop", "above", 2, Q8, [], UP),
           ("loop", "all_equal", 3, Q8, [1], 0.875),
           ("loop", "none", 4, Q8, [], 2.0),
           ("reloc", "reloc", 1, Q8)]
    return dict(L=3, scoring=L1, ops=ops)


def loop_best_init():
    """Dot-product scores: the entry scores 1.0 = minScore and its neighbour
    -0.5, so accScore 0.5 lies below bestAccScore's start and is not retained;
    from a start of 0 it would be."""
    q = bow([1, 2], [1.0, 1.0])
    ops = [("add", 1, bow([1, 2], [0.5, 0.5])), ("add", 2, bow([1, 2], [-0.25, -0.25])),
           ("covis", 1, [2]),
           ("loop", "below_start", 1, q, [], 1.0),
           ("loop", "kept", 2, q, [], -1.0)]
    return dict(L=3, scoring=DOT, ops=ops)


def loop_neighbour_gates():
    """A priming loop query on word 0 alone gives every keyframe a loop score of
    0.125.  Then Q8 with keyframe 13 connected and minScore 0.5 (minCommonWords
    6).  Entry 10 (1.0) names 11 (6 common: gate closed at equality, its 0.125 is
    stale), 12 (7 common: 0.875 added), 13 (connected: never added) and 14 (0.25,
    below minScore, not an entry itself, still added): accScore 2.125, so the
    retain threshold is 1.59375.  Entry 12 accumulates 1.625 (kept), entry 15
    1.5 (not kept).  Adding either 0.125 lifts the threshold to 1.6875 and drops
    12; leaving 14 out lowers it to 1.40625 and keeps 15.
    A neighbour below minScore cannot be elected: its score is below minScore <=
    the entry's own."""
    ops = [("add", 10, FULL), ("add", 11, C6), ("add", 12, S875), ("add", 13, FULL),
           ("add", 14, S250), ("add", 15, S875), ("add", 16, S750), ("add", 17, S625),
           ("covis", 10, [11, 12, 13, 14]), ("covis", 12, [16]), ("covis", 15, [17]),
           ("loop", "prime", 1, bow([0], [1.0]), [], 0.0),
           ("loop", "gates", 2, Q8, [13], 0.5)]
    return dict(L=3, scoring=L1, ops=ops)


S750UP = kf8([E] * 6 + [2.0 ** -24, None])            # 0.75 + 2^-24: the float above 0.75


def retain_thresholds():
    """bestAccScore 1.0: accScore 0.75 == 0.75f * best is not retained, the next
    float is.  Reloc and loop."""
    ops = [("add", 1, FULL), ("add", 2, S750), ("add", 3, S750UP),
           ("reloc", "reloc", 1, Q8), ("loop", "loop", 1, Q8, [], 0.5)]
    return dict(L=3, scoring=L1, ops=ops)


def tie_own():
    """Entry 1 and its neighbour 2 both score 0.875: the entry stays its own
    best (1.75 elects 1); entry 2 alone (0.875) falls below 0.75 * 1.75."""
    ops = [("add", 1, S875), ("add", 2, S875), ("covis", 1, [2]),
           ("reloc", "reloc", 1, Q8), ("loop", "loop", 1, Q8, [], 0.0)]
    return dict(L=3, scoring=L1, ops=ops)


def tie_neighbours():
    """Entry 1 (0.75) names 2 and 3, both 1.0: the first stored wins."""
    ops = [("add", 1, S750), ("add", 3, FULL), ("add", 2, FULL), ("covis", 1, [2, 3]),
           ("reloc", "reloc", 1, Q8), ("loop", "loop", 1, Q8, [], 0.0),
           ("covis", 1, [3, 2]),
           ("reloc", "reloc_swapped", 2, Q8), ("loop", "loop_swapped", 2, Q8, [], 0.0)]
    return dict(L=3, scoring=L1, ops=ops)


QBIG = bow(range(8), [E] * 7 + [2.0 ** 25])


def _big(v):
    return kf8([0.0] * 7 + [v])


def neighbour_float_order():
    """accScore is a float chain in stored order: 1 + 2^24 + 1 = 2^24 (each add
    is a tie that rounds to even), reversed 1 + 1 + 2^24 = 2^24 + 2.  Keyframe 4
    accumulates 12582913 = 0.75 * 2^24 + 1: retained against best 2^24, not
    against 2^24 + 2 (threshold 12582914 after rounding)."""
    ops = [("add", 1, FULL), ("add", 2, FULL), ("add", 3, _big(2.0 ** 24)),
           ("add", 4, _big(12582913.0)), ("covis", 1, [3, 2]),
           ("reloc", "reloc", 1, QBIG), ("loop", "loop", 1, QBIG, [], 0.5)]
    return dict(L=3, scoring=L1, ops=ops)


def stale_and_separate():
    """Reloc, loop, reloc on one database.  The first reloc query (word 0 at
    1.0) scores keyframe 2 at 1.0; the loop query (word 1 at 1.0) scores it
    0.125.  In the last reloc query (Q8) keyframe 2 shares six words, is not
    scored, and is the neighbour of entry 1 (0.875): its reloc score from the
    first query (1.0) is read, so 2 is elected; its loop score would not be."""
    k2 = bow([0, 1, 2, 3, 4, 5, 30], [1.0, E, E, E, E, E, 0.25])
    ops = [("add", 1, S875), ("add", 2, k2), ("add", 3, FULL), ("covis", 1, [2]),
           ("reloc", "first", 1, bow([0], [1.0])),
           ("loop", "between", 1, bow([1], [1.0]), [], 0.0),
           ("reloc", "stale", 2, Q8)]
    return dict(L=3, scoring=L1, ops=ops)


def list_order():
    """lKFsSharingWords is ordered by (smallest shared word, position in that
    word's list).  30 and 20 both start at word 5 and were added in that order;
    40, added last, starts at word 2 and comes first; erased and added again, 30
    goes behind 20."""
    q = bow([2, 5, 9], [0.25, 0.5, 0.25])
    a = bow([5, 9], [0.5, 0.5])
    ops = [("add", 30, a), ("add", 20, bow([5], [1.0])), ("add", 25, bow([9, 11], [0.5, 0.5])),
           ("add", 40, bow([2, 9], [0.5, 0.5])),
           ("reloc", "first", 1, q), ("loop", "first_loop", 1, q, [], 0.0),
           ("erase", 30), ("reloc", "erased", 2, q),
           ("add", 30, a), ("reloc", "readded", 3, q), ("loop", "readded_loop", 3, q, [], 0.0)]
    return dict(L=3, scoring=L1, ops=ops)


def clear_reuse():
    """clear() hands slot numbers out again.  Before it, the keyframe in slot 1
    is scored 1.0; after it, a new keyframe sits in slot 1, shares six words with
    Q8 (= minCommonWords, not scored) and is the neighbour of entry 5: it reads
    as never scored, 0.0, so 5 stays its own best."""
    k2 = bow([0, 1, 2, 3, 4, 5, 30], [1.0, E, E, E, E, E, 0.25])
    ops = [("add", 1, S875), ("add", 2, k2), ("covis", 1, [2]),
           ("reloc", "before", 1, bow([0], [1.0])), ("loop", "before_loop", 1, bow([0], [1.0]), [], 0.0),
           ("clear",),
           ("reloc", "empty", 2, Q8),
           ("add", 5, S875), ("add", 6, C6), ("add", 7, FULL), ("covis", 5, [6, 2]),
           ("reloc", "after", 3, Q8), ("loop", "after_loop", 2, Q8, [], 0.5)]
    return dict(L=3, scoring=L1, ops=ops)


def denormal_scores():
    """Scores that are float denormals: 3 * 2^-141 (768 ulps of 2^-149), 2^-141 +
    2^-149, 2^-149, a double of 0.75 * 2^-149 that rounds up to 2^-149 and one of
    0.25 * 2^-149 that rounds to 0.  The loop query's minScore is 2^-149."""
    p = lambda e: 2.0 ** e
    q = bow([0, 1], [p(-130), p(-130)])           # near enough for |vi - wi| to be exact
    ops = [("add", 1, bow([0, 1], [p(-140), p(-141)])), ("add", 2, bow([0, 1], [p(-141), p(-149)])),
           ("add", 3, bow([0, 1], [p(-149), 0.0])), ("add", 4, bow([0, 1], [p(-150), p(-151)])),
           ("add", 5, bow([0, 1], [p(-151), 0.0])), ("covis", 1, [2, 3]), ("covis", 4, [5, 3]),
           ("reloc", "reloc", 1, q), ("loop", "loop", 1, q, [], p(-149))]
    return dict(L=3, scoring=L1, ops=ops)


# the growing database ------------------------------------------------------
STAR, MOON_A, MOON_B, MOON_C = 900001, 900002, 900003, 900004
HEAVY = {STAR: [1024.0, 1024.0, 1024.0], MOON_A: [1024.0, 1024.0, 512.0],
         MOON_B: [1024.0, 1024.0, 768.0], MOON_C: [1024.0, 1024.0, 640.0]}
HEAVY_AT = {700: STAR, 2100: MOON_A, 3000: MOON_B, 3500: MOON_C}   # slot -> id
QALL = bow(range(64), [1024.0] * 64)
QSWEEP = bow(range(0, 64, 3), [0.03125] * 22)
# list positions (of the final 4,097-slot queries) after which the next
# three-word keyframe is made to elect the named heavy keyframe
ELECTORS = [(100, MOON_A), (500, STAR), (1500, MOON_B), (1600, MOON_A), (2500, STAR),
            (3000, MOON_C), (3300, MOON_B)]


def sweep():
    """One database grown to 4,097 slots of one- to three-word keyframes over 64
    words (every value 0.25, so the list order is all ties and the scores are
    exact), with a reloc and a loop query at each of SWEEP_SLOTS: 1024 / 1025,
    2048 / 2049 and 4096 / 4097 are the edges of k_db_list's three LDS sorts and
    of the global one.  Slot 0, the newest slot and a sprinkle in between are
    erased before some of them; covisibility lists name ids across the whole
    range, ids not yet added included.
    At 4,097 slots QALL (all 64 words at 1024) lists every live keyframe.  Four
    heavy keyframes on words 61..63 sort to the list's end; three-word keyframes
    at chosen list positions name one of them and so elect it: STAR from below
    position 1,024 and from above 2,048, MOON_A from chunks 0 and 1, MOON_B
    first from chunk 1, MOON_C first from chunk 2."""
    rng = np.random.default_rng(20)
    n = SWEEP_SLOTS[-1]
    ops, ids, kf_words, live = [], [], {}, []
    qid = 0
    for slot in range(n):
        if slot in HEAVY_AT:
            kf_id = HEAVY_AT[slot]
            b = bow([61, 62, 63], HEAVY[kf_id])
        else:
            kf_id = 1 + 3 * slot
            w = np.sort(rng.choice(61, int(rng.integers(1, 4)), replace=False))
            b = bow(w, [0.25] * len(w))
        ops.append(("add", kf_id, b))
        ids.append(kf_id)
        live.append(kf_id)
        kf_words[kf_id] = b[0]
        if slot % 7 == 0 and kf_id not in HEAVY:
            # neighbours anywhere in the final id range, so also ids added later
            nb = 1 + 3 * rng.integers(0, n, int(rng.integers(1, 11)))
            ops.append(("covis", kf_id, [int(x) for x in nb if x != kf_id]))
        if slot + 1 in SWEEP_SLOTS:
            if slot + 1 in (5, 1025, 2049, 4096):
                gone = {ids[0], ids[-1]} | {ids[i] for i in range(2, slot, 97)}
                for g in sorted(gone & set(live) - set(HEAVY)):
                    ops.append(("erase", g))
                    live.remove(g)
            qid += 1
            connected = [int(x) for x in rng.choice(ids, min(len(ids), 5), replace=False)]
            ops.append(("reloc", "reloc_%d" % (slot + 1), qid, QSWEEP))
            ops.append(("loop", "loop_%d" % (slot + 1), qid, QSWEEP, connected, 0.03125))
    # the final list under QALL: live keyframes by (smallest word, slot)
    slot_of = {k: i for i, k in enumerate(ids)}
    order = sorted(live, key=lambda k: (int(kf_words[k][0]), slot_of[k]))
    taken = set()
    for pos, heavy in ELECTORS:
        p = next(i for i in range(pos, len(order))
                 if len(kf_words[order[i]]) == 3 and order[i] not in HEAVY and order[i] not in taken)
        taken.add(order[p])
        ops.append(("covis", order[p], [heavy]))
    ops.append(("reloc", "select_reloc", qid + 1, QALL))
    ops.append(("loop", "select_loop", qid + 1, QALL, [ids[5], ids[2000]], 0.5))
    return dict(L=3, scoring=L1, ops=ops, electors=sorted(taken))


# large queries ---------------------------------------------------------------
N_WORDS_L4 = 10 ** 4
LATE, BIG, BIG2 = 5001, 5002, 5003


def query_size():
    """Queries of 8192 (staged in LDS), 8193 (binary search in global memory)
    and 9,000 words against 40 keyframes on the k = 10, L = 4 tree.  BIG has
    8,300 words; LATE's first 130 words (0..129) are in neither of the first two
    queries, so its first shared word sits in its third 64-word chunk."""
    rng = np.random.default_rng(21)
    nw = N_WORDS_L4
    out_of_q = np.sort(np.concatenate([np.arange(200), 200 + rng.choice(nw - 200, nw - Q_LDS - 200,
                                                                       replace=False)]))
    q_words = np.setdiff1d(np.arange(nw), out_of_q)
    assert len(q_words) == Q_LDS

    def vec(words):
        words = np.sort(np.asarray(words))
        x = rng.random(len(words)) + 0.01
        return bow(words, x / x.sum())

    q0 = vec(q_words)
    q1 = vec(np.concatenate([q_words, [199]]))
    q2 = vec(np.setdiff1d(np.arange(nw), rng.choice(nw, nw - 9000, replace=False)))
    ops = []
    for i in range(36):
        ops.append(("add", 100 + i, vec(rng.choice(nw, int(rng.integers(50, 400)), replace=False))))
    ops.append(("add", LATE, vec(np.concatenate([np.arange(130), rng.choice(q_words[q_words > 300], 20,
                                                                         replace=False)]))))
    ops.append(("add", BIG, vec(rng.choice(nw, 8300, replace=False))))
    ops.append(("add", BIG2, vec(rng.choice(nw, 7900, replace=False))))
    ops.append(("add", 5004, vec([int(q_words[4000])])))
    for i in range(0, 36, 3):
        ops.append(("covis", 100 + i, [BIG, 100 + (i + 5) % 36, LATE]))
    ops.append(("covis", BIG, [BIG2, 101]))
    ops.append(("covis", BIG2, [BIG, LATE]))
    ops += [("reloc", "reloc_8192", 1, q0), ("loop", "loop_8192", 1, q0, [103], 0.0),
            ("reloc", "reloc_8193", 2, q1), ("loop", "loop_8193", 2, q1, [BIG2], 0.0),
            ("reloc", "reloc_9000", 3, q2), ("loop", "loop_9000", 3, q2, [], 0.0),
            # without the two big keyframes a small keyframe's own vector scores the small ones
            ("erase", BIG), ("erase", BIG2), ("reloc", "reloc_small", 4, ops[0][2]),
            ("loop", "loop_small", 4, ops[0][2], [], 0.0)]
    return dict(L=4, scoring=L1, ops=ops)


def growth():
    """A first keyframe of one word, then one of 5,000 words -- more than the
    device buffer's doubling -- then a query that hits both."""
    rng = np.random.default_rng(22)
    w = np.sort(rng.choice(np.arange(1, N_WORDS_L4), 5000, replace=False))
    x = rng.random(5000)
    big = bow(w, x / x.sum())
    q = bow(np.concatenate([[0], w[::7]]), np.full(1 + len(w[::7]), 2.0 ** -10))
    ops = [("add", 1, bow([0], [1.0])), ("add", 2, big), ("covis", 1, [2]),
           ("reloc", "both", 1, bow([0, int(w[0])], [0.5, 0.5])), ("reloc", "wide", 2, q),
           ("loop", "wide_loop", 1, q, [], 0.0)]
    return dict(L=4, scoring=L1, ops=ops)


DB_CASES = {
    "loop_thresholds": loop_thresholds,
    "loop_best_init": loop_best_init,
    "loop_neighbour_gates": loop_neighbour_gates,
    "retain_thresholds": retain_thresholds,
    "tie_own": tie_own,
    "tie_neighbours": tie_neighbours,
    "neighbour_float_order": neighbour_float_order,
    "stale_and_separate": stale_and_separate,
    "list_order": list_order,
    "clear_reuse": clear_reuse,
    "denormal_scores": denormal_scores,
    "sweep": sweep,
    "query_size": query_size,
    "growth": growth,
}


@functools.lru_cache(maxsize=None)
def db_case(name):
    return DB_CASES[name]()


def voc_size(case):
    return 10 ** case["L"]


def replay(case, db, inspect=None):
    """Runs the script on `db`; returns, per query, dict(tag, kind, out, ids,
    common, scores, scored).  inspect(tag, db) is called after each query."""
    res = []
    for op in case["ops"]:
        kind = op[0]
        if kind == "add":
            db.add(op[1], op[2])
        elif kind == "erase":
            db.erase(op[1])
        elif kind == "covis":
            db.set_covisibility(op[1], op[2])
        elif kind == "clear":
            db.clear()
        else:
            if kind == "reloc":
                out = db.DetectRelocalizationCandidates(op[2], op[3])
            else:
                out = db.DetectLoopCandidates(op[2], op[3], op[4], op[5])
            ids, common, scores, scored = db.last_query()
            r = dict(tag=op[1], kind=kind, out=[int(x) for x in out],
                     ids=np.array(ids, np.int64), common=np.array(common, np.int32),
                     scores=np.array(scores, np.float32), scored=np.array(scored, np.uint8))
            if inspect is not None:
                r["seen"] = inspect(op[1], db)
            res.append(r)
    return res


def same_answer(got, want):
    """Candidates and lKFsSharingWords (ids, word counts, scored flags, score
    bits) of one query, exactly."""
    return got["tag"] == want["tag"] and got["out"] == want["out"] and \
        np.array_equal(got["ids"], want["ids"]) and np.array_equal(got["common"], want["common"]) and \
        np.array_equal(got["scored"], want["scored"]) and same_floats(got["scores"], want["scores"])


def first_difference(got, want):
    if len(got) != len(want):
        return "%d queries against %d" % (len(got), len(want))
    for g, w in zip(got, want):
        if not same_answer(g, w):
            return "query %r: candidates %r against %r" % (w["tag"], g["out"][:8], w["out"][:8])
    return None


def _inspect_ref(tag, db):
    pos = {int(k.mnId): i for i, k in enumerate(db.last)}
    return dict(min_common=db.last_min_common, elected=list(db.last_elected),
                entries=[(e, float(a), b) for e, a, b in db.last_entries],
                acc_bits=[int(bits32(a).ravel()[0]) for _, a, _ in db.last_entries],
                entry_pos=[pos[e] for e, _, _ in db.last_entries],
                n_db=len(db.kfs), n_slots=db.n_added)


@functools.lru_cache(maxsize=None)
def ref_answers(name, switch=None):
    """The restatement's answers, computed once per (case, switch) and shared."""
    case = db_case(name)
    db = ref.KeyFrameDatabase(voc_size(case), case["scoring"], switch)
    return replay(case, db, _inspect_ref)


def by_tag(answers):
    return {r["tag"]: r for r in answers}
