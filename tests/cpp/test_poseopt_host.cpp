// The C++ host mirror's Optimizer::PoseOptimization on hand-checkable frames:
// exact observations with one planted 40-pixel outlier, the start pose that is
// already the optimum with every error exactly zero (rho == 0 ends each
// round), the fewer-than-three rule and an octave out of range.
#include <cmath>
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

static KeyPoint kp(float x, float y, int octave) {
  KeyPoint k{};
  k.x = x;
  k.y = y;
  k.size = 31.0f;
  k.octave = octave;
  k.class_id = -1;
  return k;
}

static orb_pose_t identity() {
  orb_pose_t p{};
  p.rcw[0] = p.rcw[4] = p.rcw[8] = 1.0f;
  return p;
}

int main() {
  ORBmatcher m;
  const orb_camera_t cam{718.856f, 718.856f, 607.1928f, 185.2157f, 386.1448f, 0.5371657f};
  std::vector<float> inv(8);
  for (int l = 0; l < 8; ++l) inv[l] = 1.0f / (float)std::pow(1.44, l);

  // 1. 24 points seen from the identity pose, stereo and mono mixed, keypoint 0
  //    without a MapPoint and keypoint 7 displaced by 40 px: it alone is flagged
  {
    const int n = 25;
    std::vector<KeyPoint> keys(n, kp(9.0f, 9.0f, 0));
    std::vector<float> ur(n, -1.0f), pts;
    std::vector<int32_t> mp(n, -1);
    for (int i = 1; i < n; ++i) {
      const double z = 5.0 + 1.3 * i, x = (i % 5 - 2) * 0.21 * z, y = (i % 3 - 1) * 0.15 * z;
      pts.push_back((float)x);
      pts.push_back((float)y);
      pts.push_back((float)z);
      const double X = pts[pts.size() - 3], Y = pts[pts.size() - 2], Z = pts[pts.size() - 1];
      const double u = X / Z * cam.fx + cam.cx, v = Y / Z * cam.fy + cam.cy;
      keys[i] = kp((float)u, (float)v, i % 8);
      if (i % 2) ur[i] = (float)(u - cam.bf / Z);
      mp[i] = i - 1;
    }
    keys[7].x += 40.0f;
    PoseFrame F;
    F.mvKeysUn = &keys;
    F.mvuRight = &ur;
    F.mvpMapPoints = &mp;
    F.points = pts.data();
    F.mvInvLevelSigma2 = &inv;
    F.cam = cam;
    F.mTcw = identity();
    F.mvbOutlier.assign(n, 0xA5);
    const int nin = Optimizer::PoseOptimization(m, &F);
    EXPECT(nin == 23 && F.info.n_edges == 24 && F.info.lm_iterations >= 4);
    for (int i = 0; i < n; ++i) EXPECT(F.mvbOutlier[i] == (i == 0 ? 0xA5 : (i == 7 ? 1 : 0)));
    for (int i = 0; i < 9; ++i) EXPECT(std::fabs(F.mTcw.rcw[i] - (i % 4 == 0 ? 1.0f : 0.0f)) < 1e-4f);
    for (int i = 0; i < 3; ++i) EXPECT(std::fabs(F.mTcw.tcw[i]) < 1e-3f && std::fabs(F.mTcw.ow[i]) < 1e-3f);
  }

  // 2. points on the optical axis observed at (cx, cy): every error is exactly
  //    zero, the step is zero, rho == 0 ends each of the four rounds
  {
    const int n = 12;
    std::vector<KeyPoint> keys(n, kp(cam.cx, cam.cy, 1));
    std::vector<int32_t> mp(n);
    std::vector<float> pts;
    for (int i = 0; i < n; ++i) {
      mp[i] = i;
      pts.insert(pts.end(), {0.0f, 0.0f, 4.0f + 3.0f * i});
    }
    PoseFrame F;
    F.mvKeysUn = &keys;
    F.mvpMapPoints = &mp;
    F.points = pts.data();
    F.mvInvLevelSigma2 = &inv;
    F.cam = cam;
    F.mTcw = identity();
    const int nin = Optimizer::PoseOptimization(m, &F);
    EXPECT(nin == n && F.info.n_edges == n && F.info.lm_iterations == 4 && F.info.rejected_trials == 4);
    for (int i = 0; i < 9; ++i) EXPECT(F.mTcw.rcw[i] == (i % 4 == 0 ? 1.0f : 0.0f));
    for (int i = 0; i < 3; ++i) EXPECT(F.mTcw.tcw[i] == 0.0f);
    for (int i = 0; i < n; ++i) EXPECT(F.mvbOutlier[i] == 0);

    // 3. two correspondences: 0, the pose untouched, their flags cleared
    std::vector<int32_t> two(n, -1);
    two[3] = 3;
    two[9] = 9;
    F.mvpMapPoints = &two;
    F.mTcw.tcw[0] = 0.25f;
    F.mvbOutlier.assign(n, 0xA5);
    EXPECT(Optimizer::PoseOptimization(m, &F) == 0 && F.info.n_edges == 2);
    EXPECT(F.mTcw.tcw[0] == 0.25f && F.mTcw.rcw[0] == 1.0f);
    for (int i = 0; i < n; ++i) EXPECT(F.mvbOutlier[i] == ((i == 3 || i == 9) ? 0 : 0xA5));

    // 4. an octave outside mvInvLevelSigma2 on a keypoint that has a MapPoint
    F.mvpMapPoints = &mp;
    keys[5].octave = 8;
    F.mvbOutlier.assign(n, 0xA5);
    EXPECT(Optimizer::PoseOptimization(m, &F) == 0 && F.info.n_edges == -1);
    EXPECT(F.mTcw.tcw[0] == 0.25f && F.mvbOutlier[5] == 0xA5 && F.mvbOutlier[0] == 0xA5);
  }
  if (fails == 0) std::printf("OK\n");
  return fails != 0;
}
