// The C++ host mirror's device-batched SearchForTriangulation on problems packed
// by tests/test_cpp_tri_batch.py:
//   test_tri_batch_host <in> <out>
// <in>:  int32 header {P, K, stride, n_levels, only_stereo, check_ori}, the
//        camera (6 floats), scale factors and sigma2 (n_levels floats each),
//        then the K keyframe slots: keys, desc, nkeys, fv_nodes, fv_offs,
//        fv_feats, n_fv_nodes, point_index, u_right, poses; then kf1_slot,
//        kf2_slot (P int32 each) and F12 (9 floats per problem).
// <out>: match12 (P * stride int32), info (P records).
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
  const std::vector<int32_t> hdr = take<int32_t>(in, 6);
  const size_t P = hdr[0], K = hdr[1], S = hdr[2], L = hdr[3];
  const std::vector<float> camv = take<float>(in, 6);
  const orb_camera_t cam{camv[0], camv[1], camv[2], camv[3], camv[4], camv[5]};
  const std::vector<float> scale = take<float>(in, L), sigma2 = take<float>(in, L);
  Dev<KeyPoint> keys(take<KeyPoint>(in, K * S));
  Dev<uint8_t> desc(take<uint8_t>(in, K * S * 32));
  Dev<int32_t> nkeys(take<int32_t>(in, K));
  Dev<uint32_t> nodes(take<uint32_t>(in, K * S));
  Dev<int32_t> offs(take<int32_t>(in, K * (S + 1)));
  Dev<uint32_t> feats(take<uint32_t>(in, K * S));
  Dev<int32_t> nnodes(take<int32_t>(in, K));
  Dev<int32_t> pidx(take<int32_t>(in, K * S));
  Dev<float> uright(take<float>(in, K * S));
  Dev<orb_pose_t> pose(take<orb_pose_t>(in, K));
  Dev<int32_t> slot1(take<int32_t>(in, P)), slot2(take<int32_t>(in, P));
  Dev<float> f12(take<float>(in, 9 * P));
  std::fclose(in);
  const std::vector<int32_t> junk(P * S, 77);
  const std::vector<orb_tri_match_info_t> noInfo(P);
  Dev<int32_t> match(junk);
  Dev<orb_tri_match_info_t> info(noInfo);
  static_assert(sizeof(orb_tri_match_info_t) == 24, "six int32 fields");

  ORBmatcher m(0.6f, hdr[5] != 0);
  if (ORBmatcher::search_for_triangulation_batch_max_stride() <
      ORBmatcher::create_new_map_points_max_stride())
    return 3;
  const ORBmatcher::BowSlots kf{keys.p, desc.p, nkeys.p, nodes.p, offs.p, feats.p, nnodes.p};
  m.search_for_triangulation_batch((int)P, slot1.p, slot2.p, kf, pidx.p, uright.p, pose.p, (int)S,
                                   f12.p, cam, scale, sigma2, hdr[4] != 0, match.p, info.p);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  put(o, match.host());
  put(o, info.host());
  std::fclose(o);
  std::printf("OK\n");
  return 0;
}
