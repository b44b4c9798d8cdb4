// The C++ host mirror's device-batched SearchByProjection(CurrentFrame,
// LastFrame) and the discard / marking call on hand-checkable problems: n
// keypoints 40 px apart at octave 0, each with a map point that carries its
// exact descriptor and projects 1 px (or 5 px) beside it at the identity pose.
//   problem 0: 20 points at 1 px, th 3               -> 20 matches, no retry
//   problem 1: 19 at 1 px and 5 at 5 px              -> 19, retried at 6: 24
//   problem 2: 19 at 1 px, stereo, tlw.z = 1 > mb    -> 19, retried: 19, forward
// Plain g++: the four HIP runtime calls it needs are declared by hand.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../orb_slam2-chinese-annotation_amd/host/orb_amd.hpp"

extern "C" {
int hipMalloc(void** p, size_t n);
int hipFree(void* p);
int hipMemcpy(void* dst, const void* src, size_t n, int kind);  // 1: to device, 2: to host
int hipDeviceSynchronize(void);
}

using namespace orb_amd;

static int fails = 0;
#define EXPECT(c)                                          \
  do {                                                     \
    if (!(c)) {                                            \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                             \
    }                                                      \
  } while (0)

template <typename T>
struct Dev {
  T* p = nullptr;
  size_t n = 0;
  explicit Dev(const std::vector<T>& h) : n(h.size()) {
    if (hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)) != 0) std::abort();
    if (n) hipMemcpy(p, h.data(), n * sizeof(T), 1);
  }
  ~Dev() { hipFree(p); }
  std::vector<T> host() const {
    std::vector<T> h(n);
    hipDeviceSynchronize();
    if (n) hipMemcpy(h.data(), p, n * sizeof(T), 2);
    return h;
  }
};

int main() {
  const int P = 3, S = 32, NEAR[P] = {20, 19, 19}, FAR[P] = {0, 5, 0};
  const orb_camera_t cam{512.0f, 512.0f, 320.0f, 240.0f, 64.0f, 0.125f};
  const float Z = 8.0f;
  std::vector<float> scale(8, 1.0f);
  for (int l = 1; l < 8; ++l) scale[l] = scale[l - 1] * 1.2f;

  std::vector<KeyPoint> keys(P * S), lastKeys(P * S);
  std::vector<uint8_t> desc(P * S * 32), mpDesc(P * S * 32), outlier(P * S, 0);
  std::vector<float> ur(P * S, -1.0f);
  std::vector<int32_t> nkeys(P), lastN(P), lastIdx(P * S, -1), kpMatch(P * S, 77);
  std::vector<orb_map_point_t> pts(P * S);
  std::vector<orb_pose_t> cur(P), last(P);
  std::memset(pts.data(), 0, pts.size() * sizeof(orb_map_point_t));
  for (int p = 0; p < P; ++p) {
    std::memset(&cur[p], 0, sizeof(orb_pose_t));
    cur[p].rcw[0] = cur[p].rcw[4] = cur[p].rcw[8] = 1.0f;
    last[p] = cur[p];
    if (p == 2) last[p].tcw[2] = 1.0f;
    const int n = NEAR[p] + FAR[p];
    nkeys[p] = lastN[p] = n;
    for (int i = 0; i < n; ++i) {
      const int k = p * S + i;
      const float x = 40.0f + 40.0f * (i % 8), y = 40.0f + 40.0f * (i / 8);
      std::memset(&keys[k], 0, sizeof(KeyPoint));
      keys[k].x = x;
      keys[k].y = y;
      keys[k].size = 31.0f;
      keys[k].class_id = -1;
      lastKeys[k] = keys[k];
      for (int b = 0; b < 32; ++b) desc[k * 32 + b] = mpDesc[k * 32 + b] = (uint8_t)(37 * i + 11 * b + p);
      const float u = x + (i < NEAR[p] ? 1.0f : 5.0f);
      pts[k].pos[0] = (u - cam.cx) / cam.fx * Z;
      pts[k].pos[1] = (y - cam.cy) / cam.fy * Z;
      pts[k].pos[2] = Z;
      pts[k].has_obs = (uint8_t)(i % 2);
      pts[k].bad = (uint8_t)(p == 0 && i == 4);
      lastIdx[k] = i;
      if (p == 2) ur[k] = u - cam.bf / Z;  // the projection's own right coordinate
    }
  }
  std::vector<orb_frame_match_info_t> info(P);
  std::vector<orb_track_discard_info_t> out(P);
  Dev<KeyPoint> dKeys(keys), dLast(lastKeys);
  Dev<uint8_t> dDesc(desc), dMpDesc(mpDesc), dOutlier(outlier);
  Dev<float> dUr(ur);
  Dev<int32_t> dN(nkeys), dLastN(lastN), dLastIdx(lastIdx), dMatch(kpMatch);
  Dev<orb_map_point_t> dPts(pts);
  Dev<orb_pose_t> dCur(cur), dLastPose(last);
  Dev<orb_frame_match_info_t> dInfo(info);
  Dev<orb_track_discard_info_t> dOut(out);

  ORBmatcher m(0.9f, false);
  EXPECT(ORBmatcher::search_by_projection_frame_batch_max_stride() >= 4096);
  m.search_by_projection_frame_batch(P, dKeys.p, dDesc.p, dUr.p, nullptr, dN.p, S, dCur.p,
                                     dLastPose.p, dLast.p, dLastN.p, dLastIdx.p, nullptr, dPts.p,
                                     dMpDesc.p, S, cam, 0.0f, 640.0f, 0.0f, 480.0f, scale, 3.0f,
                                     false, 20, dMatch.p, dInfo.p);
  info = dInfo.host();
  kpMatch = dMatch.host();
  const int WANT[P][5] = {{20, 20, 0, 0, 0}, {24, 19, 1, 0, 0}, {19, 19, 1, 1, 0}};
  for (int p = 0; p < P; ++p) {
    EXPECT(info[p].n_matches == WANT[p][0] && info[p].n_matches_first_pass == WANT[p][1]);
    EXPECT(info[p].retried == WANT[p][2] && info[p].forward == WANT[p][3] &&
           info[p].backward == WANT[p][4]);
    for (int i = 0; i < S; ++i)
      EXPECT(kpMatch[p * S + i] == (i < nkeys[p] ? i : 77));
  }

  // discard: keypoints 1 and 2 of every problem flagged; problem 0's point 4 is bad
  for (int p = 0; p < P; ++p) outlier[p * S + 1] = outlier[p * S + 2] = 1;
  outlier[0 * S + 31] = 1;  // past the count: stays
  hipMemcpy(dOutlier.p, outlier.data(), outlier.size(), 1);
  m.track_discard_outliers_batch(P, dN.p, S, dMatch.p, dOutlier.p, dPts.p, S, true, dInfo.p,
                                 dOut.p);
  out = dOut.host();
  kpMatch = dMatch.host();
  outlier = dOutlier.host();
  pts = dPts.host();
  for (int p = 0; p < P; ++p) {
    const int n = nkeys[p];
    EXPECT(out[p].n_discarded == 2 && out[p].n_matches == WANT[p][0] - 2);
    EXPECT(out[p].n_matches_map == n / 2 - 1);  // odd keypoints have has_obs; keypoint 1 went
    for (int i = 0; i < n; ++i) {
      const bool gone = i == 1 || i == 2 || (p == 0 && i == 4);
      EXPECT(kpMatch[p * S + i] == (gone ? -1 : i));
      EXPECT(outlier[p * S + i] == 0);
      EXPECT(pts[p * S + i].seen == ((p == 0 && i == 4) ? 0 : 1));
    }
  }
  EXPECT(outlier[31] == 1);
  bool threw = false;
  try {
    m.track_discard_outliers_batch(P, dN.p, S, dMatch.p, dOutlier.p, dPts.p, 0, true, dInfo.p,
                                   dOut.p);
  } catch (const Error& e) {
    threw = e.status == ORB_EINVAL;
  }
  EXPECT(threw);
  if (fails == 0) std::printf("OK\n");
  return fails != 0;
}
