// The C++ host mirror's ComputeSceneMedianDepth / CreateNewMapPoints on one
// (current keyframe, neighbour) pair packed by tests/test_cpp_newpoints.py:
//   test_newpoints_host <in> <out>
// <in>:  int32 header {n1, n2, n_levels, monocular, stereo, cursor, capacity,
//        n_exist}, then per keyframe keys, (u_right, depth when stereo),
//        point_index, pose; match12; cam1, cam2 (six floats each);
//        scale_factors, level_sigma2; the n_exist points of the map; the
//        neighbour's median depth (used when not monocular: it is not read).
// <out>: info, cursor, status, x3d, new_pairs, both point_index rows, the
//        points array (capacity records), the median used and its depth count.
// Plain g++ against the C ABI.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../orb_slam2-chinese-annotation_amd/host/orb_amd.hpp"

using namespace orb_amd;

template <typename T>
static std::vector<T> take(std::FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
    std::printf("FAIL short input\n");
    std::exit(2);
  }
  return v;
}
template <typename T>
static void put(std::FILE* f, const std::vector<T>& v) {
  if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  const std::vector<int32_t> hdr = take<int32_t>(in, 8);
  const size_t n1 = hdr[0], n2 = hdr[1], nLevels = hdr[2], capacity = hdr[6], nExist = hdr[7];
  const bool monocular = hdr[3] != 0, stereo = hdr[4] != 0;
  static_assert(sizeof(orb_new_point_info_t) == 64 && sizeof(orb_map_point_t) == 36, "ABI records");
  ORBmatcher::KeyFrameView kf[2];
  for (int k = 0; k < 2; ++k) {
    const size_t n = k == 0 ? n1 : n2;
    kf[k].mvKeysUn = take<KeyPoint>(in, n);
    if (stereo) {
      kf[k].mvuRight = take<float>(in, n);
      kf[k].mvDepth = take<float>(in, n);
    }
    kf[k].mvpMapPoints = take<int32_t>(in, n);
    kf[k].pose = take<orb_pose_t>(in, 1)[0];
  }
  const std::vector<int32_t> match12 = take<int32_t>(in, n1);
  const orb_camera_t cam1 = take<orb_camera_t>(in, 1)[0], cam2 = take<orb_camera_t>(in, 1)[0];
  const std::vector<float> sf = take<float>(in, nLevels), sigma2 = take<float>(in, nLevels);
  const std::vector<orb_map_point_t> exist = take<orb_map_point_t>(in, nExist);
  float median = take<float>(in, 1)[0];
  std::fclose(in);
  if (ORBmatcher::create_new_map_points_max_stride() < 2048 ||
      ORBmatcher::scene_median_depth_max_stride() < 2048)
    return 3;

  ORBmatcher m(0.6f, false);
  int nDepths = -1;
  if (monocular) median = m.ComputeSceneMedianDepth(kf[1], exist, 2, &nDepths);
  std::vector<orb_map_point_t> points(capacity);
  if (capacity) std::memset(points.data(), 0xA5, capacity * sizeof(orb_map_point_t));
  std::copy(exist.begin(), exist.end(), points.begin());
  int cursor = hdr[5];
  std::vector<uint8_t> status;
  std::vector<float> x3D;
  std::vector<int32_t> pairs;
  const orb_new_point_info_t info = m.CreateNewMapPoints(
      kf[0], kf[1], match12, cam1, cam2, sf, sigma2, monocular, median, points, cursor, status,
      x3D, pairs);

  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  std::fwrite(&info, sizeof(info), 1, o);
  const int32_t cur = cursor, cnt = nDepths;
  std::fwrite(&cur, 4, 1, o);
  put(o, status);
  put(o, x3D);
  put(o, pairs);
  put(o, kf[0].mvpMapPoints);
  put(o, kf[1].mvpMapPoints);
  put(o, points);
  std::fwrite(&median, 4, 1, o);
  std::fwrite(&cnt, 4, 1, o);
  std::fclose(o);
  std::printf("OK %d %d\n", info.n_new, info.gated);
  return 0;
}
