"""GPU parity of place recognition: BoW scoring (ScoringObject.cpp:23-311) and
the keyframe database queries (src/KeyFrameDatabase.cc:79-339) against the
statement-by-statement restatement in tests/placerec_ref.py.  Everything is
compared exactly: scores as bit patterns, lists and candidates in order.
BowVectors come from the oracle's vocabulary transform on synthetic trees."""
import ctypes

import numpy as np
import pytest

import placerec_ref as ref
import scenarios

pytestmark = pytest.mark.gpu

LENS = [0, 1, 63, 64, 65, 200, 1500]
SCORINGS = [ref.L1_NORM, ref.L2_NORM, ref.CHI_SQUARE, ref.BHATTACHARYYA, ref.DOT_PRODUCT]
_cache = {}


def _voc(gpu, v, scoring=0):
    return gpu.ORBVocabulary(v["k"], v["L"], v["parent"], v["leaf"], v["desc"], v["weight"],
                             scoring, 0)


def _tree(L, seed):
    key = ("tree", L, seed)
    if key not in _cache:
        _cache[key] = scenarios.vocabulary(rng_seed=seed, k=10, L=L)
    return _cache[key]


def _bow(oracle, v, n, seed, scoring=0):
    r = oracle.vocab_transform(v, scenarios.vocab_features(v, n, rng_seed=seed), 4, scoring, 0)
    return r[0].copy(), r[1].copy()


def _pick(bow, idx):
    idx = np.sort(np.asarray(idx, np.int64))
    return bow[0][idx].copy(), bow[1][idx].copy()


def _subset(bow, n, rng):
    return _pick(bow, rng.choice(len(bow[0]), n, replace=False))


def _bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _bits32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------- score
def score_pairs(oracle, scoring):
    """Pairs over every length combination: partially overlapping (about half of
    b's words also in a), identical, and disjoint."""
    key = ("pairs", scoring)
    if key in _cache:
        return _cache[key]
    v = _tree(4, 31)
    rng = np.random.default_rng(5 + scoring)
    A = _bow(oracle, v, 12000, 1, scoring)
    B = _bow(oracle, v, 12000, 2, scoring)
    assert len(A[0]) >= 1500 and len(B[0]) >= 1500
    al, bl = [], []
    for la in LENS:
        a = _subset(A, la, rng)
        for lb in LENS:
            inb = np.isin(B[0], a[0])
            pool, rest = np.flatnonzero(inb), np.flatnonzero(~inb)
            h = min(len(pool), lb // 2)
            idx = np.concatenate([rng.choice(pool, h, replace=False),
                                  rng.choice(rest, lb - h, replace=False)])
            al.append(a)
            bl.append(_pick(B, idx))
        al.append(a)            # identical
        bl.append(a)
        rest = np.flatnonzero(~np.isin(B[0], a[0]))
        al.append(a)            # disjoint, same length
        bl.append(_pick(B, rng.choice(rest, la, replace=False)))
    want = np.array([ref.score(a, b, scoring) for a, b in zip(al, bl)], np.float64)
    ncommon = [int(np.isin(b[0], a[0]).sum()) for a, b in zip(al, bl)]
    assert max(ncommon) >= 700 and sum(1 for c in ncommon if 0 < c < 64) > 5
    _cache[key] = (v, al, bl, want)
    return _cache[key]


@pytest.mark.parametrize("scoring", SCORINGS)
def test_score_host(gpu, oracle, scoring):
    v, al, bl, want = score_pairs(oracle, scoring)
    voc = _voc(gpu, v, scoring)
    got = voc.score_pairs(al, bl)
    assert np.array_equal(_bits64(got), _bits64(want))
    # one pair at a time, both argument orders
    for i in (len(al) // 2, len(al) - 3):
        assert _bits64(voc.score(al[i], bl[i])) == _bits64(want[i])
        assert _bits64(voc.score(bl[i], al[i])) == _bits64(ref.score(bl[i], al[i], scoring))


@pytest.mark.parametrize("scoring", SCORINGS)
def test_score_device_batch(gpu, oracle, scoring):
    torch = pytest.importorskip("torch")
    v, al, bl, want = score_pairs(oracle, scoring)
    voc = _voc(gpu, v, scoring)
    dev = torch.device("cuda:0")

    def csr(vs):
        offs = np.zeros(len(vs) + 1, np.int32)
        offs[1:] = np.cumsum([len(x[0]) for x in vs])
        w = np.concatenate([x[0] for x in vs]).astype(np.uint32).view(np.int32)
        x = np.concatenate([x[1] for x in vs]).astype(np.float64)
        return [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (offs, w, x)]

    ao, aw, av = csr(al)
    bo, bw, bv = csr(bl)
    out = torch.full((len(al),), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    voc.score_batch(len(al), ao.data_ptr(), aw.data_ptr(), av.data_ptr(), bo.data_ptr(),
                    bw.data_ptr(), bv.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits64(out.cpu().numpy()), _bits64(want))


def test_score_kl_is_refused(gpu, oracle):
    v = _tree(3, 32)
    voc = _voc(gpu, v, ref.KL)
    a = _bow(oracle, v, 50, 1)
    with pytest.raises(gpu.OrbError) as e:
        voc.score(a, a)
    assert e.value.status == gpu.ORB_EINVAL
    with pytest.raises(gpu.OrbError) as e:
        gpu.KeyFrameDatabase(voc)
    assert e.value.status == gpu.ORB_EINVAL
    good = _voc(gpu, v)
    with pytest.raises(gpu.OrbError) as e:   # words not strictly ascending
        good.score((np.array([3, 3], np.uint32), np.ones(2)), a)
    assert e.value.status == gpu.ORB_EINVAL


# ---------------------------------------------------------------- database
class Pair:
    """A device database and the restatement, driven in step."""

    def __init__(self, gpu, v, scoring=0):
        self.voc = _voc(gpu, v, scoring)
        self.db = gpu.KeyFrameDatabase(self.voc)
        self.ref = ref.KeyFrameDatabase(int(v["leaf"].sum()), scoring)

    def add(self, kf_id, bow):
        self.db.add(kf_id, bow)
        self.ref.add(kf_id, bow)

    def erase(self, kf_id):
        self.db.erase(kf_id)
        self.ref.erase(kf_id)

    def clear(self):
        self.db.clear()
        self.ref.clear()

    def covis(self, kf_id, ids):
        self.db.set_covisibility(kf_id, ids)
        self.ref.set_covisibility(kf_id, ids)

    def _check_last(self):
        ids, common, scores, scored = self.db.last_query()
        rids, rcommon, rscores, rscored = self.ref.last_query()
        assert np.array_equal(ids, rids)
        assert np.array_equal(common, rcommon)
        assert np.array_equal(scored, rscored)
        assert np.array_equal(_bits32(scores), _bits32(rscores))
        assert len(self.db) == len(self.ref.kfs)

    def reloc(self, qid, bow):
        got = self.db.DetectRelocalizationCandidates(qid, bow)
        want = self.ref.DetectRelocalizationCandidates(qid, bow)
        self._check_last()
        assert got.tolist() == want
        return want

    def loop(self, qid, bow, connected, min_score):
        got = self.db.DetectLoopCandidates(qid, bow, connected, min_score)
        want = self.ref.DetectLoopCandidates(qid, bow, connected, min_score)
        self._check_last()
        assert got.tolist() == want
        return want


def keyframes(oracle, L, n_kf=300, seed=0):
    """n_kf keyframes (ids in an order unrelated to the add order) on a k = 10
    tree of depth L, with up-to-10 neighbour snapshots that also name ids that
    are not in the database."""
    key = ("kfs", L, n_kf, seed)
    if key in _cache:
        return _cache[key]
    v = _tree(L, 40 + L)
    rng = np.random.default_rng(seed)
    ids = (1000 + 7 * rng.permutation(n_kf)).tolist()
    big = _bow(oracle, v, 600, 9000 + seed)
    kfs = []
    for i, kf_id in enumerate(ids):
        if i % 40 in (3, 11, 19, 27):   # exact sizes around the wave width
            bow = _subset(big, [1, 63, 64, 65][(i % 40 - 3) // 8], rng)
        else:
            bow = _bow(oracle, v, int(rng.integers(20, 400)), 100 * seed + i)
        kfs.append((kf_id, bow))
    sizes = {len(b[0]) for _, b in kfs}
    assert {1, 63, 64, 65} <= sizes
    covis = {}
    for kf_id in ids:
        nb = rng.choice(ids + [5, 6], int(rng.integers(0, 11)), replace=False)
        covis[kf_id] = [int(x) for x in nb if x != kf_id]
    _cache[key] = (v, kfs, covis)
    return _cache[key]


def _fill(p, kfs, covis):
    for kf_id, bow in kfs:
        p.add(kf_id, bow)
    for kf_id, nb in covis.items():
        p.covis(kf_id, nb)


@pytest.mark.parametrize("L", [3, 4])
def test_relocalization_query(gpu, oracle, L):
    v, kfs, covis = keyframes(oracle, L)
    p = Pair(gpu, v)
    _fill(p, kfs, covis)
    for q in range(3):
        out = p.reloc(q + 1, _bow(oracle, v, [300, 40, 1000][q], 7000 + q))
        assert len(out) > 0
        nlist = len(p.ref.last)
        if L == 3:
            assert nlist > 200          # dense sharing
        elif q == 1:
            assert 0 < nlist < len(kfs)  # some keyframes share nothing
    # a keyframe's own BowVector as the query finds that keyframe
    kf_id, bow = kfs[5]
    assert kf_id in p.reloc(9, bow)


@pytest.mark.parametrize("scoring", [ref.L2_NORM, ref.CHI_SQUARE, ref.BHATTACHARYYA,
                                     ref.DOT_PRODUCT])
def test_relocalization_other_scoring_types(gpu, oracle, scoring):
    v = _tree(3, 43)
    p = Pair(gpu, v, scoring)
    rng = np.random.default_rng(scoring)
    ids = list(range(1, 61))
    for i in ids:
        p.add(i, _bow(oracle, v, int(rng.integers(30, 200)), 50 + i, scoring))
    for i in ids:
        p.covis(i, rng.choice(ids, 4, replace=False))
    assert p.reloc(1, _bow(oracle, v, 150, 999, scoring))


@pytest.mark.parametrize("m", [5, 10, 15])
def test_threshold_truncation(gpu, m):
    """maxCommonWords = m with m * 0.8f an integer (4, 8, 12): keyframes with
    exactly that many common words are not scored, one more is."""
    v = _tree(3, 43)
    p = Pair(gpu, v)
    rng = np.random.default_rng(m)
    q = (np.arange(0, 40, 2, dtype=np.uint32), np.full(20, 0.05))
    cut = int(np.float32(m) * np.float32(0.8))
    counts = [m, cut, cut + 1, cut - 1, 1, m, cut, 0]
    for i, c in enumerate(counts):
        shared = rng.choice(q[0], c, replace=False)
        other = rng.choice(np.arange(101, 900, 2), 7, replace=False)
        w = np.sort(np.concatenate([shared, other])).astype(np.uint32)
        val = rng.random(len(w))
        p.add(i + 1, (w, val / val.sum()))
    for i in range(len(counts)):
        p.covis(i + 1, [(i + 1) % len(counts) + 1, (i + 3) % len(counts) + 1])
    p.reloc(77, q)
    assert p.ref.last_min_common == cut == m * 4 // 5
    _, words, _, scored = p.ref.last_query()
    assert sorted(words.tolist()) == sorted(c for c in counts if c)
    assert scored.tolist() == [int(c > cut) for c in words]


def test_stale_scores(gpu, oracle):
    """The second query scores few keyframes, but their neighbours share a word
    with it and carry the first query's score."""
    v, kfs, covis = keyframes(oracle, 3, seed=1)
    # q2 is one keyframe's own vector, so hardly anything but that keyframe is
    # scored; q1 is a single word of one of its neighbours: maxCommonWords 1,
    # minCommonWords 0, and every keyframe holding the word is scored
    q2 = kfs[17][1]
    bows = dict(kfs)
    nb = next(n for n in covis[kfs[17][0]] if n in bows and len(bows[n][0]) > 100)
    q1 = (bows[nb][0][:1].copy(), np.ones(1))
    # CPU: the condition holds in the restatement alone
    r = ref.KeyFrameDatabase(int(v["leaf"].sum()))
    for kf_id, bow in kfs:
        r.add(kf_id, bow)
    for kf_id, nb in covis.items():
        r.set_covisibility(kf_id, nb)
    r.DetectRelocalizationCandidates(1, q1)
    ids1, _, _, scored1 = r.last_query()
    first = set(ids1[scored1 == 1].tolist())
    r.DetectRelocalizationCandidates(2, q2)
    ids2, _, _, scored2 = r.last_query()
    shares2 = set(ids2.tolist())
    second = set(ids2[scored2 == 1].tolist())
    stale = [n for k in second for n in r.kfs[k].neighbours
             if n in shares2 and n not in second and n in first]
    assert stale, "no neighbour reads an earlier query's score"
    # GPU parity for both
    p = Pair(gpu, v)
    _fill(p, kfs, covis)
    p.reloc(1, q1)
    p.reloc(2, q2)


def test_mutation(gpu, oracle):
    v, kfs, covis = keyframes(oracle, 3, n_kf=120, seed=2)
    p = Pair(gpu, v)
    _fill(p, kfs, covis)
    q = _bow(oracle, v, 300, 8100)
    p.reloc(1, q)
    with pytest.raises(gpu.OrbError) as e:      # already present
        p.db.add(kfs[0][0], kfs[0][1])
    assert e.value.status == gpu.ORB_EINVAL
    gone = kfs[::3]
    for kf_id, _ in gone:
        p.erase(kf_id)
    p.erase(123456789)                          # not present: no-op
    assert len(p.db) == len(kfs) - len(gone)
    p.reloc(2, q)
    for kf_id, bow in gone[::2][::-1]:          # back in, in another order: new sequence numbers
        p.add(kf_id, bow)
    p.covis(gone[0][0], [kfs[1][0], kfs[2][0]])
    p.reloc(3, q)
    p.loop(4, q, [kfs[1][0]], 0.0)
    p.clear()
    assert len(p.db) == 0
    assert p.reloc(5, q) == []
    assert len(p.db.last_query()[0]) == 0
    for kf_id, bow in kfs[:10]:
        p.add(kf_id, bow)
    assert p.reloc(6, q)


def test_loop_query(gpu, oracle):
    v, kfs, covis = keyframes(oracle, 3, seed=3)
    p = Pair(gpu, v)
    _fill(p, kfs, covis)
    q = _bow(oracle, v, 400, 8200)
    connected = [kf_id for kf_id, _ in kfs[10:25]] + [424242]   # one id not in the database
    # minScore as LoopClosing::DetectLoop computes it (src/LoopClosing.cc:135-150)
    scores = p.voc.score_pairs([q] * 15, [b for _, b in kfs[10:25]])
    want = [ref.score(q, b) for _, b in kfs[10:25]]
    assert np.array_equal(_bits64(scores), _bits64(want))
    min_score = float(min(np.float32(1), np.float32(scores.min())))   # float minScore = 1
    out = p.loop(1, q, connected, min_score)
    assert out and not set(out) & set(connected)
    assert not set(p.ref.last_query()[0].tolist()) & set(connected)
    assert p.loop(2, q, connected, 2.0) == []       # minScore removes every entry
    assert p.loop(3, q, [], 0.0)
    assert p.reloc(3, q)                            # reloc ids are a sequence of their own


def test_loop_same_best_keyframe_emitted_once(gpu, oracle):
    v, kfs, _ = keyframes(oracle, 3, n_kf=60, seed=4)
    q = _bow(oracle, v, 60, 8300)
    # the best-scoring keyframe of this query, from the restatement alone
    r = ref.KeyFrameDatabase(int(v["leaf"].sum()))
    for kf_id, bow in kfs:
        r.add(kf_id, bow)
    r.DetectLoopCandidates(1, q, [], 0.0)
    ids, _, scores, scored = r.last_query()
    star_id = int(ids[np.argmax(np.where(scored == 1, scores, -1))])
    p = Pair(gpu, v)
    for kf_id, bow in kfs:
        p.add(kf_id, bow)
    for kf_id, _ in kfs:
        if kf_id != star_id:
            p.covis(kf_id, [star_id])              # every entry elects the same keyframe
    out = p.loop(1, q, [], 0.0)
    elected = p.ref.last_elected
    assert elected.count(star_id) > 1
    first = list(dict.fromkeys(elected))            # each at its first occurrence
    assert out == first and out.count(star_id) == 1


def test_empties_and_errors(gpu, oracle):
    v = _tree(3, 43)
    p = Pair(gpu, v)
    q = _bow(oracle, v, 100, 1)
    empty = (np.zeros(0, np.uint32), np.zeros(0))
    assert p.reloc(1, q) == []                      # empty database
    assert p.loop(1, q, [], 0.0) == []
    a = (np.array([1, 3, 5], np.uint32), np.array([0.5, 0.25, 0.25]))
    b = (np.array([2, 4], np.uint32), np.array([0.5, 0.5]))
    p.add(1, a)
    p.add(2, a)
    p.add(3, empty)                                 # a keyframe without words never shares
    assert p.reloc(2, empty) == []                  # empty query
    assert p.reloc(3, b) == []                      # shares nothing
    assert p.reloc(4, a) == [1, 2]
    L = gpu.lib()
    w, x = np.ascontiguousarray(a[0]), np.ascontiguousarray(a[1])
    out = np.zeros(4, np.int64)
    n = ctypes.c_int(-1)
    args = (len(w), w.ctypes.data, x.ctypes.data, out.ctypes.data)
    assert L.orb_kf_database_detect_relocalization(p.db._h, 5, *args, 1, ctypes.byref(n)) \
        == gpu.ORB_ECAPACITY and n.value == 2
    assert L.orb_kf_database_detect_relocalization(p.db._h, 0, *args, 4, ctypes.byref(n)) \
        == gpu.ORB_EINVAL                           # id 0
    assert L.orb_kf_database_detect_relocalization(p.db._h, 5, *args, 4, ctypes.byref(n)) \
        == gpu.ORB_EINVAL                           # repeated id
    assert L.orb_kf_database_detect_relocalization(p.db._h, 6, *args, 4, ctypes.byref(n)) \
        == gpu.ORB_OK and n.value == 2 and out[:2].tolist() == [1, 2]
    assert L.orb_kf_database_last_query(p.db._h, None, None, None, None, 0, ctypes.byref(n)) \
        == gpu.ORB_ECAPACITY and n.value == 2
    for bad in [(np.array([5, 3], np.uint32), np.ones(2)),                 # not ascending
                (np.array([10 ** 6], np.uint32), np.ones(1))]:             # beyond the vocabulary
        with pytest.raises(gpu.OrbError) as e:
            p.db.add(50, bad)
        assert e.value.status == gpu.ORB_EINVAL
        with pytest.raises(gpu.OrbError) as e:
            p.db.DetectRelocalizationCandidates(60, bad)
        assert e.value.status == gpu.ORB_EINVAL
    with pytest.raises(gpu.OrbError):
        p.db.set_covisibility(1, list(range(11)))   # more than 10
    with pytest.raises(gpu.OrbError):
        p.db.set_covisibility(99, [1])              # not in the database


def test_many_small_keyframes(gpu):
    """More keyframes than the list sort holds in LDS (4096): the sort runs in
    global memory.  One to three words each, so the list order is all ties."""
    v = _tree(3, 43)
    p = Pair(gpu, v)
    rng = np.random.default_rng(11)
    n = 4300
    for i in range(n):
        w = np.sort(rng.choice(64, int(rng.integers(1, 4)), replace=False)).astype(np.uint32)
        p.add(i + 1, (w, np.full(len(w), 1.0 / len(w))))
    for i in range(0, n, 9):
        p.covis(i + 1, rng.integers(1, n + 1, 10))
    q = (np.arange(0, 64, 3, dtype=np.uint32), np.full(22, 1.0 / 22))
    assert p.reloc(1, q)
    assert len(p.ref.kfs) > 4096 and len(p.ref.last) > 1000


def test_end_to_end(gpu, oracle):
    """extract -> transform -> add, then query with the next frame of the sequence."""
    v = _tree(4, 44)
    p = Pair(gpu, v)
    ext = gpu.ORBextractor(500, 1.2, 8, 20, 7)
    bows = []
    for frame in range(3):
        _, d = ext(gpu.synth_image(3, frame, 640, 480))
        bw, bv, _ = p.voc.transform(d, 4)
        rw, rv = oracle.vocab_transform(v, d, 4)[:2]
        assert np.array_equal(bw, rw) and np.array_equal(_bits64(bv), _bits64(rv))
        bows.append((bw, bv))
    p.add(1, bows[0])
    p.add(2, bows[1])
    p.covis(1, [2])
    p.covis(2, [1])
    out = p.reloc(1, bows[2])
    assert out
    want = ref.score(bows[2], bows[1])
    assert _bits64(p.voc.score(bows[2], bows[1])) == _bits64(want)
