// placerec_oracle.cpp -- CPU ORACLE for place recognition: DBoW2 BoW scoring
// and ORB-SLAM2's KeyFrameDatabase.  TEST INFRASTRUCTURE ONLY: linked into
// liborb_oracle.so next to orb_oracle.cpp, loaded by tests/ only.
//
// A second statement of what tests/placerec_ref.py restates in Python, written
// from the reference text and with the reference's own containers, so that a
// misreading in either one shows as a disagreement (tests/test_oracle_placerec.py):
//   * L1Scoring::score             Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68
//   * L2Scoring::score                                                   :73-120
//   * ChiSquareScoring::score                                            :125-170
//   * BhattacharyyaScoring::score                                        :226-266
//   * DotProductScoring::score                                           :271-311
//     (KLScoring::score :175-221 calls log() and is not restated)
//   * KeyFrameDatabase::add / erase / clear        src/KeyFrameDatabase.cc:42-76
//   * KeyFrameDatabase::DetectLoopCandidates                             :79-202
//   * KeyFrameDatabase::DetectRelocalizationCandidates                   :205-339
// BowVector is std::map<WordId, WordValue> (BowVector.h:56-58) walked with
// lower_bound; the inverted file is std::vector<std::list<KF*>>
// (KeyFrameDatabase.h:74); the queries use std::list and std::set as the
// reference does.
//
// The keyframe record holds what KeyFrameDatabase touches of a KeyFrame
// (include/KeyFrame.h:144-149): mnId, mBowVec, mnLoopQuery, mnLoopWords,
// mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore, and a snapshot of
// GetBestCovisibilityKeyFrames(10) as ids.  The reference leaves the two scores
// uninitialised; they start at 0.0f here, the value the library documents.
//
// PARITY STATUS: unpinned against a reference binary.  The reference itself
// cannot be built here: OpenCV is absent, ScoringObject.cpp includes
// TemplatedVocabulary.h (which needs it), and KeyFrameDatabase.cc needs the
// whole KeyFrame.  Pinned against the independent Python restatement instead.
#include <math.h>
#include <stdint.h>

#include <list>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace placerec_oracle {

typedef uint32_t WordId;                          // BowVector.h:20
typedef double WordValue;                         // BowVector.h:23
typedef std::map<WordId, WordValue> BowVector;    // BowVector.h:56-58

enum { L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT };  // BowVector.h:45-53

static BowVector make_bow(int n, const uint32_t* words, const double* values) {
  BowVector v;
  for (int i = 0; i < n; ++i) v.insert(v.end(), std::make_pair(words[i], values[i]));
  return v;
}

// The walk all five score() bodies share (SO:34-59 and its four copies): both
// iterators advance on an equal key, otherwise the one behind jumps with
// lower_bound to the other's key.  `term(vi, wi)` is called once per common
// word, in ascending word order, vi from v1 and wi from v2.
template <class Term>
static void for_common_words(const BowVector& v1, const BowVector& v2, Term term) {
  BowVector::const_iterator a = v1.begin(), b = v2.begin();
  while (a != v1.end() && b != v2.end()) {
    if (a->first == b->first) {
      term(a->second, b->second);
      ++a;
      ++b;
    } else if (a->first < b->first) {
      a = v1.lower_bound(b->first);
    } else {
      b = v2.lower_bound(a->first);
    }
  }
}

static double score_l1(const BowVector& v1, const BowVector& v2) {    // SO:23-68
  double score = 0;
  for_common_words(v1, v2, [&](double vi, double wi) {
    score += fabs(vi - wi) - fabs(vi) - fabs(wi);                     // SO:41
  });
  return -score / 2.0;                                                // SO:65
}

static double score_l2(const BowVector& v1, const BowVector& v2) {    // SO:73-120
  double score = 0;
  for_common_words(v1, v2, [&](double vi, double wi) { score += vi * wi; });   // SO:91
  if (score >= 1) return 1.0;                                         // SO:114-115
  return 1.0 - sqrt(1.0 - score);                                     // SO:117
}

static double score_chi(const BowVector& v1, const BowVector& v2) {   // SO:125-170
  double score = 0;
  for_common_words(v1, v2, [&](double vi, double wi) {
    if (vi + wi != 0.0) score += vi * wi / (vi + wi);                 // SO:148
  });
  return 2. * score;                                                  // SO:167
}

static double score_bhat(const BowVector& v1, const BowVector& v2) {  // SO:226-266
  double score = 0;
  for_common_words(v1, v2, [&](double vi, double wi) { score += sqrt(vi * wi); });   // SO:245
  return score;
}

static double score_dot(const BowVector& v1, const BowVector& v2) {   // SO:271-311
  double score = 0;
  for_common_words(v1, v2, [&](double vi, double wi) { score += vi * wi; });   // SO:290
  return score;
}

// TemplatedVocabulary::score -> m_scoring_object->score (TemplatedVocabulary.h:1217).
static bool score(int scoring, const BowVector& v1, const BowVector& v2, double& out) {
  switch (scoring) {
    case L1_NORM: out = score_l1(v1, v2); return true;
    case L2_NORM: out = score_l2(v1, v2); return true;
    case CHI_SQUARE: out = score_chi(v1, v2); return true;
    case BHATTACHARYYA: out = score_bhat(v1, v2); return true;
    case DOT_PRODUCT: out = score_dot(v1, v2); return true;
    default: return false;
  }
}

struct KF {
  int64_t mnId = 0;
  BowVector mBowVec;
  uint64_t mnLoopQuery = 0;     // KeyFrame.cc:35
  int mnLoopWords = 0;
  float mLoopScore = 0.0f;
  uint64_t mnRelocQuery = 0;
  int mnRelocWords = 0;
  float mRelocScore = 0.0f;
  std::vector<int64_t> neighbours;  // ids, best first
};

struct Database {
  int scoring = L1_NORM;
  size_t vocSize = 0;
  std::vector<std::list<KF*> > mvInvertedFile;   // KeyFrameDatabase.h:74
  std::map<int64_t, KF*> inDb;                   // keyframes add() was called for and erase() not
  std::map<int64_t, KF*> known;                  // the latest record made for each id
  std::vector<KF*> owned;                        // every record (the reference never frees one here)
  // the last query, for inspection
  std::list<KF*> lastSharing;
  int lastKind = -1, lastMinCommon = 0;
  std::vector<int64_t> lastElected;

  ~Database() {
    for (KF* k : owned) delete k;
  }

  void add(KF* pKF) {                                                 // DB:42-49
    for (BowVector::const_iterator vit = pKF->mBowVec.begin(); vit != pKF->mBowVec.end(); ++vit)
      mvInvertedFile[vit->first].push_back(pKF);                      // DB:48
  }

  void erase(KF* pKF) {                                               // DB:51-70
    for (BowVector::const_iterator vit = pKF->mBowVec.begin(); vit != pKF->mBowVec.end(); ++vit) {
      std::list<KF*>& lKFs = mvInvertedFile[vit->first];
      for (std::list<KF*>::iterator lit = lKFs.begin(); lit != lKFs.end(); ++lit)
        if (*lit == pKF) {                                            // DB:63-67
          lKFs.erase(lit);
          break;
        }
    }
  }

  void clear() {                                                      // DB:72-76
    mvInvertedFile.clear();
    mvInvertedFile.resize(vocSize);
  }

  // GetBestCovisibilityKeyFrames(10) of pKF: the records its snapshot names.
  // An id no record was ever made for has no keyframe; an erased keyframe
  // still exists in the reference and is returned like any other.
  std::vector<KF*> neighbours(const KF* pKF) const {
    std::vector<KF*> v;
    for (int64_t id : pKF->neighbours) {
      std::map<int64_t, KF*>::const_iterator f = known.find(id);
      if (f != known.end()) v.push_back(f->second);
    }
    return v;
  }

  // DB:181-201 and DB:316-338, the same text twice.
  std::vector<KF*> retain(const std::list<std::pair<float, KF*> >& lAccScoreAndMatch,
                          float bestAccScore) {
    const float minScoreToRetain = 0.75f * bestAccScore;              // DB:181, :316
    std::set<KF*> spAlreadyAddedKF;
    std::vector<KF*> out;
    lastElected.clear();
    for (std::list<std::pair<float, KF*> >::const_iterator it = lAccScoreAndMatch.begin();
         it != lAccScoreAndMatch.end(); ++it) {
      if (it->first > minScoreToRetain) {                             // DB:189, :324
        KF* pKFi = it->second;
        lastElected.push_back(pKFi->mnId);
        if (!spAlreadyAddedKF.count(pKFi)) {                          // DB:192, :329
          out.push_back(pKFi);
          spAlreadyAddedKF.insert(pKFi);
        }
      }
    }
    return out;
  }

  std::vector<KF*> DetectLoopCandidates(uint64_t mnId, const BowVector& bow,
                                        const std::set<KF*>& spConnectedKeyFrames,
                                        float minScore) {             // DB:79-202
    std::list<KF*> lKFsSharingWords;
    for (BowVector::const_iterator vit = bow.begin(); vit != bow.end(); ++vit) {   // DB:89
      std::list<KF*>& lKFs = mvInvertedFile[vit->first];
      for (std::list<KF*>::iterator lit = lKFs.begin(); lit != lKFs.end(); ++lit) {
        KF* pKFi = *lit;
        if (pKFi->mnLoopQuery != mnId) {                              // DB:96
          pKFi->mnLoopWords = 0;
          if (!spConnectedKeyFrames.count(pKFi)) {                    // DB:99
            pKFi->mnLoopQuery = mnId;
            lKFsSharingWords.push_back(pKFi);
          }
        }
        pKFi->mnLoopWords++;                                          // DB:106
      }
    }
    lastSharing = lKFsSharingWords;
    lastKind = 1;
    lastMinCommon = 0;
    lastElected.clear();
    if (lKFsSharingWords.empty()) return std::vector<KF*>();          // DB:111

    std::list<std::pair<float, KF*> > lScoreAndMatch;
    int maxCommonWords = 0;
    for (KF* k : lKFsSharingWords)                                    // DB:118-122
      if (k->mnLoopWords > maxCommonWords) maxCommonWords = k->mnLoopWords;
    int minCommonWords = maxCommonWords * 0.8f;                       // DB:124
    lastMinCommon = minCommonWords;

    for (KF* pKFi : lKFsSharingWords) {                               // DB:129
      if (pKFi->mnLoopWords > minCommonWords) {                       // DB:133
        double s = 0;
        score(scoring, bow, pKFi->mBowVec, s);
        float si = s;                                                 // DB:137
        pKFi->mLoopScore = si;                                        // DB:139
        if (si >= minScore) lScoreAndMatch.push_back(std::make_pair(si, pKFi));   // DB:140
      }
    }
    if (lScoreAndMatch.empty()) return std::vector<KF*>();            // DB:145

    std::list<std::pair<float, KF*> > lAccScoreAndMatch;
    float bestAccScore = minScore;                                    // DB:149
    for (std::list<std::pair<float, KF*> >::iterator it = lScoreAndMatch.begin();
         it != lScoreAndMatch.end(); ++it) {                          // DB:152
      KF* pKFi = it->second;
      std::vector<KF*> vpNeighs = neighbours(pKFi);                   // DB:155
      float bestScore = it->first;                                    // DB:157
      float accScore = it->first;
      KF* pBestKF = pKFi;
      for (KF* pKF2 : vpNeighs) {                                     // DB:160
        if (pKF2->mnLoopQuery == mnId && pKF2->mnLoopWords > minCommonWords) {   // DB:164
          accScore += pKF2->mLoopScore;                               // DB:166
          if (pKF2->mLoopScore > bestScore) {                         // DB:167
            pBestKF = pKF2;
            bestScore = pKF2->mLoopScore;
          }
        }
      }
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));   // DB:175
      if (accScore > bestAccScore) bestAccScore = accScore;           // DB:176
    }
    return retain(lAccScoreAndMatch, bestAccScore);
  }

  std::vector<KF*> DetectRelocalizationCandidates(uint64_t mnId, const BowVector& bow) {   // DB:205-339
    std::list<KF*> lKFsSharingWords;
    for (BowVector::const_iterator vit = bow.begin(); vit != bow.end(); ++vit) {   // DB:214
      std::list<KF*>& lKFs = mvInvertedFile[vit->first];
      for (std::list<KF*>::iterator lit = lKFs.begin(); lit != lKFs.end(); ++lit) {
        KF* pKFi = *lit;
        if (pKFi->mnRelocQuery != mnId) {                             // DB:225
          pKFi->mnRelocWords = 0;
          pKFi->mnRelocQuery = mnId;
          lKFsSharingWords.push_back(pKFi);
        }
        pKFi->mnRelocWords++;                                         // DB:234
      }
    }
    lastSharing = lKFsSharingWords;
    lastKind = 0;
    lastMinCommon = 0;
    lastElected.clear();
    if (lKFsSharingWords.empty()) return std::vector<KF*>();          // DB:238

    int maxCommonWords = 0;
    for (KF* k : lKFsSharingWords)                                    // DB:244-249
      if (k->mnRelocWords > maxCommonWords) maxCommonWords = k->mnRelocWords;
    int minCommonWords = maxCommonWords * 0.8f;                       // DB:251
    lastMinCommon = minCommonWords;

    std::list<std::pair<float, KF*> > lScoreAndMatch;
    for (KF* pKFi : lKFsSharingWords) {                               // DB:258
      if (pKFi->mnRelocWords > minCommonWords) {                      // DB:262
        double s = 0;
        score(scoring, bow, pKFi->mBowVec, s);
        float si = s;                                                 // DB:267
        pKFi->mRelocScore = si;                                       // DB:268
        lScoreAndMatch.push_back(std::make_pair(si, pKFi));           // DB:270
      }
    }
    if (lScoreAndMatch.empty()) return std::vector<KF*>();            // DB:274

    std::list<std::pair<float, KF*> > lAccScoreAndMatch;
    float bestAccScore = 0;                                           // DB:278
    for (std::list<std::pair<float, KF*> >::iterator it = lScoreAndMatch.begin();
         it != lScoreAndMatch.end(); ++it) {                          // DB:281
      KF* pKFi = it->second;
      std::vector<KF*> vpNeighs = neighbours(pKFi);                   // DB:286
      float bestScore = it->first;                                    // DB:288
      float accScore = bestScore;
      KF* pBestKF = pKFi;
      for (KF* pKF2 : vpNeighs) {                                     // DB:292
        if (pKF2->mnRelocQuery != mnId) continue;                     // DB:296
        accScore += pKF2->mRelocScore;                                // DB:299
        if (pKF2->mRelocScore > bestScore) {                          // DB:301
          pBestKF = pKF2;
          bestScore = pKF2->mRelocScore;
        }
      }
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));   // DB:309
      if (accScore > bestAccScore) bestAccScore = accScore;           // DB:310
    }
    return retain(lAccScoreAndMatch, bestAccScore);
  }
};

static bool words_fit(const Database* D, int n, const uint32_t* words) {
  for (int i = 0; i < n; ++i)
    if (words[i] >= D->vocSize || (i > 0 && words[i] <= words[i - 1])) return false;
  return true;
}

static int give(const std::vector<KF*>& v, int64_t* out, int cap) {
  for (size_t i = 0; i < v.size() && (int)i < cap; ++i) out[i] = v[i]->mnId;
  return (int)v.size();
}

}  // namespace placerec_oracle

using namespace placerec_oracle;

// score(a, b) with the given ScoringType; returns 0, or -1 for KL / unknown.
extern "C" int oracle_bow_score(int scoring, int na, const uint32_t* a_words,
                                const double* a_values, int nb, const uint32_t* b_words,
                                const double* b_values, double* out) {
  const BowVector a = make_bow(na, a_words, a_values), b = make_bow(nb, b_words, b_values);
  return score(scoring, a, b, *out) ? 0 : -1;
}

extern "C" void* oracle_kfdb_create(int voc_size, int scoring) {
  if (voc_size < 0 || scoring == KL || scoring < 0 || scoring > DOT_PRODUCT) return nullptr;
  Database* D = new Database();
  D->scoring = scoring;
  D->vocSize = (size_t)voc_size;
  D->mvInvertedFile.resize(D->vocSize);                               // DB:38
  return D;
}

extern "C" void oracle_kfdb_destroy(void* h) { delete (Database*)h; }

extern "C" int oracle_kfdb_size(void* h) { return (int)((Database*)h)->inDb.size(); }

// A keyframe added again after erase is a new KeyFrame: new counters and scores.
extern "C" int oracle_kfdb_add(void* h, int64_t id, int n, const uint32_t* words,
                               const double* values) {
  Database* D = (Database*)h;
  if (D->inDb.count(id) || !words_fit(D, n, words)) return -1;
  KF* k = new KF();
  k->mnId = id;
  k->mBowVec = make_bow(n, words, values);
  D->owned.push_back(k);
  D->inDb[id] = k;
  D->known[id] = k;
  D->add(k);
  return 0;
}

extern "C" void oracle_kfdb_erase(void* h, int64_t id) {
  Database* D = (Database*)h;
  std::map<int64_t, KF*>::iterator f = D->inDb.find(id);
  if (f == D->inDb.end()) return;
  D->erase(f->second);
  D->inDb.erase(f);
}

extern "C" void oracle_kfdb_clear(void* h) {
  Database* D = (Database*)h;
  D->clear();
  D->inDb.clear();
  D->known.clear();
  D->lastSharing.clear();
  D->lastKind = -1;
  D->lastElected.clear();
}

extern "C" int oracle_kfdb_set_covisibility(void* h, int64_t id, int n, const int64_t* ids) {
  Database* D = (Database*)h;
  std::map<int64_t, KF*>::iterator f = D->inDb.find(id);
  if (f == D->inDb.end() || n < 0 || n > 10) return -1;
  f->second->neighbours.assign(ids, ids + n);
  return 0;
}

// Both queries return the number of candidates (written up to cap), -1 on bad words.
extern "C" int oracle_kfdb_detect_loop(void* h, uint64_t query_id, int n, const uint32_t* words,
                                       const double* values, int n_connected,
                                       const int64_t* connected, float min_score, int64_t* out,
                                       int cap) {
  Database* D = (Database*)h;
  if (!words_fit(D, n, words)) return -1;
  std::set<KF*> spConnectedKeyFrames;                                 // DB:81
  for (int i = 0; i < n_connected; ++i) {
    std::map<int64_t, KF*>::iterator f = D->known.find(connected[i]);
    if (f != D->known.end()) spConnectedKeyFrames.insert(f->second);
  }
  return give(D->DetectLoopCandidates(query_id, make_bow(n, words, values), spConnectedKeyFrames,
                                      min_score), out, cap);
}

extern "C" int oracle_kfdb_detect_relocalization(void* h, uint64_t query_id, int n,
                                                 const uint32_t* words, const double* values,
                                                 int64_t* out, int cap) {
  Database* D = (Database*)h;
  if (!words_fit(D, n, words)) return -1;
  return give(D->DetectRelocalizationCandidates(query_id, make_bow(n, words, values)), out, cap);
}

// lKFsSharingWords of the last query: ids, mn*Words, m*Score; returns its length.
extern "C" int oracle_kfdb_last_query(void* h, int64_t* ids, int32_t* words, float* scores,
                                      int cap) {
  Database* D = (Database*)h;
  int i = 0;
  for (KF* k : D->lastSharing) {
    if (i < cap) {
      ids[i] = k->mnId;
      words[i] = D->lastKind == 1 ? k->mnLoopWords : k->mnRelocWords;
      scores[i] = D->lastKind == 1 ? k->mLoopScore : k->mRelocScore;
    }
    ++i;
  }
  return i;
}

extern "C" int oracle_kfdb_last_min_common(void* h) { return ((Database*)h)->lastMinCommon; }

// pBestKF of every retained entry before the duplicate filter; returns the count.
extern "C" int oracle_kfdb_last_elected(void* h, int64_t* ids, int cap) {
  Database* D = (Database*)h;
  for (size_t i = 0; i < D->lastElected.size() && (int)i < cap; ++i) ids[i] = D->lastElected[i];
  return (int)D->lastElected.size();
}
