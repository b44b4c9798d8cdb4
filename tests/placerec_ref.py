"""Pure-Python restatement of DBoW2 scoring and of ORB-SLAM2's KeyFrameDatabase,
the checker of the place-recognition kernels.  Paths are relative to the
reference tree; SO = Thirdparty/DBoW2/DBoW2/ScoringObject.cpp, DB =
src/KeyFrameDatabase.cc.

Python floats are IEEE doubles, so the score chains round as the reference's
`double score` does; every quantity the reference holds in `float` goes through
numpy.float32.  The inverted file is a real list per word, walked as the
reference walks it: nothing here sorts keyframes.

A BowVector is (words, values): ascending word ids and their values, the
layout ORBVocabulary.transform / oracle.vocab_transform produce.

`switch` (score, KeyFrameDatabase) names one rule to state wrongly, one of
SWITCHES; tests/test_placerec_edge_cases.py uses it to show that each directed
case of placerec_edge_cases.py would catch a kernel wrong in that way.  None,
the default, is the reference."""
import bisect
import math

import numpy as np

L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)  # BowVector.h:45-53
f32 = np.float32
NAN = float("nan")

SWITCHES = (
    "retain_ge",          # it->first >= minScoreToRetain            (DB:189, :324)
    "minscore_gt",        # si > minScore                            (DB:140)
    "best_ge",            # pKF2 score >= bestScore                  (DB:167, :301)
    "neigh_minscore",     # loop neighbours also tested against minScore   (DB:164)
    "connected_counted",  # connected keyframes marked and counted, only not listed   (DB:99-103)
    "common_ge",          # loop neighbour gate mnLoopWords >= minCommonWords   (DB:164)
    "best_from_zero",     # loop bestAccScore starts at 0            (DB:149)
    "neigh_reverse",      # neighbours accumulated last to first     (DB:160, :292)
    "pairwise",           # the score's terms added as a pairwise tree, not a chain
    "no_chi_guard",       # chi-square without `vi + wi != 0.0`      (SO:148)
    "no_l2_clamp",        # L2 without `score >= 1`                  (SO:114)
    "order_by_slot",      # lKFsSharingWords in add order alone
)


def _sqrt(x):
    """sqrt of <math.h>: NaN for a negative argument, where math.sqrt raises."""
    return math.sqrt(x) if not x < 0 else NAN


def _div(x, y):
    """IEEE x / y, where Python raises on y == 0."""
    if y != 0:
        return x / y
    if x != x or x == 0:
        return NAN
    return math.copysign(math.inf, x) * math.copysign(1.0, y)


class _Sum:
    """`score += term`: the reference's chain; or, switched, an adjacent-pair tree."""

    def __init__(self, pairwise):
        self.s = 0.0
        self.terms = [] if pairwise else None

    def add(self, t):
        if self.terms is None:
            self.s += t
        else:
            self.terms.append(t)

    def value(self):
        if self.terms is None:
            return self.s
        t = self.terms or [0.0]
        while len(t) > 1:
            t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
        return t[0]


def _common(v1, v2):
    """The iteration every *Scoring::score shares (SO:29-59 and its copies):
    (vi, wi) for each word in both maps, ascending; lower_bound skips."""
    w1, x1 = [int(w) for w in v1[0]], [float(x) for x in v1[1]]
    w2, x2 = [int(w) for w in v2[0]], [float(x) for x in v2[1]]
    i = j = 0
    while i < len(w1) and j < len(w2):          # SO:34
        if w1[i] == w2[j]:                       # SO:39
            yield x1[i], x2[j]
            i += 1                               # SO:44-45
            j += 1
        elif w1[i] < w2[j]:                      # SO:47
            i = bisect.bisect_left(w1, w2[j])    # SO:50 v1.lower_bound
        else:
            j = bisect.bisect_left(w2, w1[i])    # SO:56 v2.lower_bound


def score(v1, v2, scoring=L1_NORM, switch=None):
    """TemplatedVocabulary::score -> m_scoring_object->score(v1, v2)."""
    acc = _Sum(switch == "pairwise")
    if scoring == L1_NORM:                       # SO:23-68
        for vi, wi in _common(v1, v2):
            acc.add(math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi))   # SO:41
        return -acc.value() / 2.0                # SO:65
    if scoring == L2_NORM:                       # SO:73-120
        for vi, wi in _common(v1, v2):
            acc.add(vi * wi)                     # SO:91
        s = acc.value()
        if s >= 1 and switch != "no_l2_clamp":   # SO:114-115
            return 1.0
        return 1.0 - _sqrt(1.0 - s)              # SO:117
    if scoring == CHI_SQUARE:                    # SO:125-170
        for vi, wi in _common(v1, v2):
            if vi + wi != 0.0 or switch == "no_chi_guard":   # SO:148
                acc.add(_div(vi * wi, vi + wi))
        return 2. * acc.value()                  # SO:167
    if scoring == BHATTACHARYYA:                 # SO:226-266
        for vi, wi in _common(v1, v2):
            acc.add(_sqrt(vi * wi))              # SO:245
        return acc.value()
    if scoring == DOT_PRODUCT:                   # SO:271-311
        for vi, wi in _common(v1, v2):
            acc.add(vi * wi)                     # SO:290
        return acc.value()
    raise ValueError("KL calls log(): not restated")


class KeyFrame:
    """The KeyFrame members KeyFrameDatabase touches (include/KeyFrame.h).  The
    reference leaves the two scores uninitialised; a score never written reads
    0.0f here, the value the library documents."""

    def __init__(self, mnId, bow):
        self.mnId = mnId
        self.mBowVec = ([int(w) for w in bow[0]], [float(x) for x in bow[1]])
        self.mnLoopQuery = 0
        self.mnLoopWords = 0
        self.mLoopScore = f32(0)
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = f32(0)
        self.neighbours = []   # ids: snapshot of GetBestCovisibilityKeyFrames(10)
        self.seq = 0           # add sequence number (read by the order_by_slot switch only)


class KeyFrameDatabase:
    def __init__(self, voc_size, scoring=L1_NORM, switch=None):
        assert switch is None or switch in SWITCHES
        self.scoring = scoring
        self.switch = switch
        self.n_added = 0
        self.last_entries = []   # (entry id, accScore, pBestKF id) of lAccScoreAndMatch
        self.voc_size = voc_size
        self.mvInvertedFile = [[] for _ in range(voc_size)]   # DB:38
        self.kfs = {}          # keyframes in the database, by id
        self.last = []         # lKFsSharingWords of the last query
        self.last_min_common = 0
        self.last_kind = None
        self.last_elected = []

    def add(self, kf_id, bow):                   # DB:42-49
        assert kf_id not in self.kfs
        pKF = KeyFrame(kf_id, bow)               # a keyframe added again is a new one
        self.kfs[kf_id] = pKF
        pKF.seq = self.n_added
        self.n_added += 1
        for w in pKF.mBowVec[0]:
            self.mvInvertedFile[w].append(pKF)   # DB:48

    def erase(self, kf_id):                      # DB:51-70
        pKF = self.kfs.pop(kf_id, None)
        if pKF is None:
            return
        for w in pKF.mBowVec[0]:
            lKFs = self.mvInvertedFile[w]
            for i, k in enumerate(lKFs):
                if k is pKF:                     # DB:63-67
                    del lKFs[i]
                    break

    def clear(self):                             # DB:72-76
        self.mvInvertedFile = [[] for _ in range(self.voc_size)]
        self.kfs = {}
        self.last = []
        self.last_kind = None

    def set_covisibility(self, kf_id, neighbour_ids):
        self.kfs[kf_id].neighbours = [int(i) for i in neighbour_ids][:10]

    def _neighbours(self, pKF):
        # an id that is not in the database is never reached by the walk, so its
        # mn*Query cannot equal the query's id: leaving it out changes nothing
        nb = [self.kfs[i] for i in pKF.neighbours if i in self.kfs]
        return nb[::-1] if self.switch == "neigh_reverse" else nb

    def _score(self, bow, pKFi):
        return f32(score(bow, pKFi.mBowVec, self.scoring, self.switch))

    def _listed(self, lKFsSharingWords):
        if self.switch == "order_by_slot":
            lKFsSharingWords.sort(key=lambda k: k.seq)
        return lKFsSharingWords

    def _better(self, s2, bestScore):            # DB:167, :301
        return s2 >= bestScore if self.switch == "best_ge" else s2 > bestScore

    def last_query(self):
        """(ids, word counts, scores, scored flags) of lKFsSharingWords."""
        loop = self.last_kind == "loop"
        ids = [k.mnId for k in self.last]
        words = [k.mnLoopWords if loop else k.mnRelocWords for k in self.last]
        scores = [k.mLoopScore if loop else k.mRelocScore for k in self.last]
        scored = [int(w > self.last_min_common) for w in words]
        return (np.array(ids, np.int64), np.array(words, np.int32), np.array(scores, np.float32),
                np.array(scored, np.uint8))

    def DetectLoopCandidates(self, mnId, bow, connected_ids, minScore):   # DB:79-202
        minScore = f32(minScore)
        sw = self.switch
        spConnectedKeyFrames = {self.kfs[i] for i in connected_ids if i in self.kfs}   # DB:81
        lKFsSharingWords = []
        for w in [int(x) for x in bow[0]]:       # DB:89
            for pKFi in self.mvInvertedFile[w]:  # DB:91-93
                if pKFi.mnLoopQuery != mnId:     # DB:96
                    pKFi.mnLoopWords = 0
                    if pKFi not in spConnectedKeyFrames:   # DB:99
                        pKFi.mnLoopQuery = mnId
                        lKFsSharingWords.append(pKFi)
                    elif sw == "connected_counted":
                        pKFi.mnLoopQuery = mnId
                pKFi.mnLoopWords += 1            # DB:106
        lKFsSharingWords = self._listed(lKFsSharingWords)
        self.last, self.last_kind, self.last_min_common = lKFsSharingWords, "loop", 0
        self.last_entries, self.last_elected = [], []
        if not lKFsSharingWords:                 # DB:111
            return []
        maxCommonWords = 0
        for k in lKFsSharingWords:               # DB:117-122
            if k.mnLoopWords > maxCommonWords:
                maxCommonWords = k.mnLoopWords
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))   # DB:124
        self.last_min_common = minCommonWords
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:            # DB:129
            if pKFi.mnLoopWords > minCommonWords:              # DB:133
                si = self._score(bow, pKFi)      # DB:137
                pKFi.mLoopScore = si             # DB:139
                if si > minScore if sw == "minscore_gt" else si >= minScore:   # DB:140
                    lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:                   # DB:145
            return []
        lAccScoreAndMatch = []
        bestAccScore = f32(0) if sw == "best_from_zero" else minScore   # DB:149
        for si, pKFi in lScoreAndMatch:          # DB:152
            bestScore = si                       # DB:157-159
            accScore = si
            pBestKF = pKFi
            for pKF2 in self._neighbours(pKFi):  # DB:160
                enough = pKF2.mnLoopWords >= minCommonWords if sw == "common_ge" \
                    else pKF2.mnLoopWords > minCommonWords
                if sw == "neigh_minscore" and not pKF2.mLoopScore >= minScore:
                    continue
                if pKF2.mnLoopQuery == mnId and enough:          # DB:164
                    accScore = f32(accScore + pKF2.mLoopScore)   # DB:166
                    if self._better(pKF2.mLoopScore, bestScore):   # DB:167
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))        # DB:175
            self.last_entries.append((pKFi.mnId, accScore, pBestKF.mnId))
            if accScore > bestAccScore:          # DB:176
                bestAccScore = accScore
        return self._retain(lAccScoreAndMatch, bestAccScore)

    def DetectRelocalizationCandidates(self, mnId, bow):       # DB:205-339
        lKFsSharingWords = []
        for w in [int(x) for x in bow[0]]:       # DB:214
            for pKFi in self.mvInvertedFile[w]:  # DB:218-220
                if pKFi.mnRelocQuery != mnId:    # DB:225
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1           # DB:234
        lKFsSharingWords = self._listed(lKFsSharingWords)
        self.last, self.last_kind, self.last_min_common = lKFsSharingWords, "reloc", 0
        self.last_entries, self.last_elected = [], []
        if not lKFsSharingWords:                 # DB:238
            return []
        maxCommonWords = 0
        for k in lKFsSharingWords:               # DB:243-249
            if k.mnRelocWords > maxCommonWords:
                maxCommonWords = k.mnRelocWords
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))   # DB:251
        self.last_min_common = minCommonWords
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:            # DB:258
            if pKFi.mnRelocWords > minCommonWords:             # DB:262
                si = self._score(bow, pKFi)      # DB:267
                pKFi.mRelocScore = si            # DB:268
                lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:                   # DB:274
            return []
        lAccScoreAndMatch = []
        bestAccScore = f32(0)                    # DB:278
        for si, pKFi in lScoreAndMatch:          # DB:281
            bestScore = si                       # DB:288-290
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in self._neighbours(pKFi):  # DB:292
                if pKF2.mnRelocQuery != mnId:    # DB:296
                    continue
                accScore = f32(accScore + pKF2.mRelocScore)    # DB:299
                if self._better(pKF2.mRelocScore, bestScore):    # DB:301
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))      # DB:309
            self.last_entries.append((pKFi.mnId, accScore, pBestKF.mnId))
            if accScore > bestAccScore:          # DB:310
                bestAccScore = accScore
        return self._retain(lAccScoreAndMatch, bestAccScore)

    def _retain(self, lAccScoreAndMatch, bestAccScore):        # DB:181-201, :316-338
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        out = []
        self.last_elected = []   # pBestKF of every retained entry, before the duplicate filter
        for acc, pKFi in lAccScoreAndMatch:
            if acc >= minScoreToRetain if self.switch == "retain_ge" else acc > minScoreToRetain:
                self.last_elected.append(pKFi.mnId)
                if pKFi not in spAlreadyAddedKF:
                    out.append(pKFi.mnId)
                    spAlreadyAddedKF.add(pKFi)
        return out
