// The C++ host mirror's place-recognition classes on the hand-worked cases of
// tests/test_placerec_ref.py: ORBVocabulary::score and KeyFrameDatabase
// (add / erase / DetectRelocalizationCandidates / DetectLoopCandidates).
#include <cstdio>
#include <vector>

#include "../../orb_slam2-chinese-annotation_amd/host/orb_amd.hpp"

using namespace orb_amd;

static int fails = 0;
#define EXPECT(c)                                          \
  do {                                                     \
    if (!(c)) {                                            \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                             \
    }                                                      \
  } while (0)

int main() {
  // a one-level tree with ten words (word i = node i + 1); L1, TF-IDF
  const int n = 11;
  std::vector<int32_t> parent(n, 0);
  std::vector<uint8_t> leaf(n, 1), desc((size_t)n * 32, 0);
  std::vector<double> weight(n, 1.0);
  leaf[0] = 0;
  for (int i = 1; i < n; ++i) desc[(size_t)i * 32] = (uint8_t)i;
  ORBVocabulary voc;
  voc.create(10, 1, ORB_VOC_L1_NORM, ORB_VOC_TF_IDF, parent, leaf, desc, weight);
  EXPECT(voc.size() == 10);

  const BowVector a{{1, 0.5}, {3, 0.25}, {7, 0.25}}, b{{1, 0.25}, {4, 0.5}, {7, 0.25}};
  EXPECT(voc.score(a, b) == 0.5);
  EXPECT(voc.score(a, a) == 1.0);
  EXPECT(voc.score(a, BowVector{{2, 1.0}}) == 0.0);

  KeyFrameDatabase db(voc);
  db.add(10, BowVector{{2, 0.5}, {5, 0.5}});
  db.add(11, BowVector{{1, 0.5}, {2, 0.25}, {5, 0.25}});
  db.add(12, BowVector{{5, 1.0}});
  db.SetBestCovisibilityKeyFrames(10, {11});
  db.SetBestCovisibilityKeyFrames(11, {10, 12});
  EXPECT(db.size() == 3);
  const BowVector qa{{1, 0.25}, {2, 0.25}, {5, 0.5}}, qb{{5, 1.0}};
  typedef std::vector<int64_t> Ids;
  EXPECT(db.DetectRelocalizationCandidates(1, qb) == Ids{12});
  EXPECT(db.DetectRelocalizationCandidates(2, qa) == Ids{12});  // through the first query's scores
  EXPECT(db.DetectLoopCandidates(5, qb, {12}, 0.3f) == Ids{10});
  EXPECT(db.DetectLoopCandidates(6, qb, {12}, 0.6f).empty());
  db.erase(10);
  EXPECT(db.size() == 2);
  EXPECT(db.DetectLoopCandidates(7, qb, {}, 0.0f) == Ids{12});
  db.clear();
  EXPECT(db.size() == 0 && db.DetectRelocalizationCandidates(3, qa).empty());
  if (fails == 0) std::printf("OK\n");
  return fails != 0;
}
