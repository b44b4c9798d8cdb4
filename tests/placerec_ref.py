"""Pure-Python restatement of DBoW2 scoring and of ORB-SLAM2's KeyFrameDatabase,
the checker of the place-recognition kernels.  Paths are relative to the
reference tree; SO = Thirdparty/DBoW2/DBoW2/ScoringObject.cpp, DB =
src/KeyFrameDatabase.cc.

Python floats are IEEE doubles, so the score chains round as the reference's
`double score` does; every quantity the reference holds in `float` goes through
numpy.float32.  The inverted file is a real list per word, walked as the
reference walks it: nothing here sorts keyframes.

A BowVector is (words, values): ascending word ids and their values, the
layout ORBVocabulary.transform / oracle.vocab_transform produce."""
import bisect
import math

import numpy as np

L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)  # BowVector.h:45-53
f32 = np.float32


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


def score(v1, v2, scoring=L1_NORM):
    """TemplatedVocabulary::score -> m_scoring_object->score(v1, v2)."""
    s = 0.0
    if scoring == L1_NORM:                       # SO:23-68
        for vi, wi in _common(v1, v2):
            s += math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi)   # SO:41
        return -s / 2.0                          # SO:65
    if scoring == L2_NORM:                       # SO:73-120
        for vi, wi in _common(v1, v2):
            s += vi * wi                         # SO:91
        return 1.0 if s >= 1 else 1.0 - math.sqrt(1.0 - s)            # SO:114-117
    if scoring == CHI_SQUARE:                    # SO:125-170
        for vi, wi in _common(v1, v2):
            if vi + wi != 0.0:                   # SO:148
                s += vi * wi / (vi + wi)
        return 2. * s                            # SO:167
    if scoring == BHATTACHARYYA:                 # SO:226-266
        for vi, wi in _common(v1, v2):
            s += math.sqrt(vi * wi)              # SO:245
        return s
    if scoring == DOT_PRODUCT:                   # SO:271-311
        for vi, wi in _common(v1, v2):
            s += vi * wi                         # SO:290
        return s
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


class KeyFrameDatabase:
    def __init__(self, voc_size, scoring=L1_NORM):
        self.scoring = scoring
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
        return [self.kfs[i] for i in pKF.neighbours if i in self.kfs]

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
        spConnectedKeyFrames = {self.kfs[i] for i in connected_ids if i in self.kfs}   # DB:81
        lKFsSharingWords = []
        for w in [int(x) for x in bow[0]]:       # DB:89
            for pKFi in self.mvInvertedFile[w]:  # DB:91-93
                if pKFi.mnLoopQuery != mnId:     # DB:96
                    pKFi.mnLoopWords = 0
                    if pKFi not in spConnectedKeyFrames:   # DB:99
                        pKFi.mnLoopQuery = mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1            # DB:106
        self.last, self.last_kind, self.last_min_common = lKFsSharingWords, "loop", 0
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
                si = f32(score(bow, pKFi.mBowVec, self.scoring))   # DB:137
                pKFi.mLoopScore = si             # DB:139
                if si >= minScore:               # DB:140
                    lScoreAndMatch.append((si, pKFi))
        if not lScoreAndMatch:                   # DB:145
            return []
        lAccScoreAndMatch = []
        bestAccScore = minScore                  # DB:149
        for si, pKFi in lScoreAndMatch:          # DB:152
            bestScore = si                       # DB:157-159
            accScore = si
            pBestKF = pKFi
            for pKF2 in self._neighbours(pKFi):  # DB:160
                if pKF2.mnLoopQuery == mnId and pKF2.mnLoopWords > minCommonWords:   # DB:164
                    accScore = f32(accScore + pKF2.mLoopScore)   # DB:166
                    if pKF2.mLoopScore > bestScore:              # DB:167
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))        # DB:175
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
        self.last, self.last_kind, self.last_min_common = lKFsSharingWords, "reloc", 0
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
                si = f32(score(bow, pKFi.mBowVec, self.scoring))   # DB:267
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
                if pKF2.mRelocScore > bestScore:               # DB:301
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))      # DB:309
            if accScore > bestAccScore:          # DB:310
                bestAccScore = accScore
        return self._retain(lAccScoreAndMatch, bestAccScore)

    def _retain(self, lAccScoreAndMatch, bestAccScore):        # DB:181-201, :316-338
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        out = []
        self.last_elected = []   # pBestKF of every retained entry, before the duplicate filter
        for acc, pKFi in lAccScoreAndMatch:
            if acc > minScoreToRetain:
                self.last_elected.append(pKFi.mnId)
                if pKFi not in spAlreadyAddedKF:
                    out.append(pKFi.mnId)
                    spAlreadyAddedKF.add(pKFi)
        return out
