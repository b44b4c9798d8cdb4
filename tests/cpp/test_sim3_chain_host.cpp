// The C++ host mirror's two ComputeSim3 matcher batches:
//   test_sim3_chain_host caps
//       prints the two capacity functions (no device needed);
//   test_sim3_chain_host <in> <out>
//       runs search_by_bow_kf_batch, then search_by_sim3_batch on its rows, on
//       problems packed by tests/test_cpp_sim3_chain.py.
// <in>:  int32 header {P, K, stride, n_levels, n_points, check_ori, min_matches},
//        nnratio, the camera (6 floats), width, height, log scale, th (floats),
//        scale factors (n_levels floats), then the K keyframe slots: keys, desc,
//        nkeys, fv_nodes, fv_offs, fv_feats, n_fv_nodes, point_index, poses;
//        then kf1_slot, kf2_slot (P int32 each), the points and their
//        descriptors (n_points each) and P Sim3 records.
// <out>: match12 and index2 after the BoW batch, bow info, match12 and index2
//        after the search, new12 (P * stride int32 each), search info.
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
  static_assert(sizeof(orb_sim3_search_info_t) == 20, "five int32 fields");
  if (argc == 2 && std::strcmp(argv[1], "caps") == 0) {
    std::printf("%d %d %d\n", ORBmatcher::search_by_bow_kf_batch_max_stride(),
                ORBmatcher::search_by_sim3_batch_max_stride(),
                ORBmatcher::optimize_sim3_max_stride());
    return 0;
  }
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  const std::vector<int32_t> hdr = take<int32_t>(in, 7);
  const size_t P = hdr[0], K = hdr[1], S = hdr[2], L = hdr[3], NP = hdr[4];
  const float nnratio = take<float>(in, 1)[0];
  const std::vector<float> camv = take<float>(in, 6);
  const orb_camera_t cam{camv[0], camv[1], camv[2], camv[3], camv[4], camv[5]};
  const std::vector<float> hv = take<float>(in, 4);  // width, height, log scale, th
  const std::vector<float> scale = take<float>(in, L);
  Dev<KeyPoint> keys(take<KeyPoint>(in, K * S));
  Dev<uint8_t> desc(take<uint8_t>(in, K * S * 32));
  Dev<int32_t> nkeys(take<int32_t>(in, K));
  Dev<uint32_t> nodes(take<uint32_t>(in, K * S));
  Dev<int32_t> offs(take<int32_t>(in, K * (S + 1)));
  Dev<uint32_t> feats(take<uint32_t>(in, K * S));
  Dev<int32_t> nnodes(take<int32_t>(in, K));
  Dev<int32_t> pidx(take<int32_t>(in, K * S));
  Dev<orb_pose_t> pose(take<orb_pose_t>(in, K));
  Dev<int32_t> slot1(take<int32_t>(in, P)), slot2(take<int32_t>(in, P));
  Dev<orb_map_point_t> points(take<orb_map_point_t>(in, NP));
  Dev<uint8_t> mpDesc(take<uint8_t>(in, NP * 32));
  Dev<orb_sim3_result_t> sim3(take<orb_sim3_result_t>(in, P));
  std::fclose(in);
  const std::vector<int32_t> junk(P * S, 0x5A5A5A5A);
  Dev<int32_t> match(junk), index2(junk), new12(junk);
  const std::vector<orb_bow_match_info_t> noBow(P);
  const std::vector<orb_sim3_search_info_t> noSearch(P);
  Dev<orb_bow_match_info_t> bowInfo(noBow);
  Dev<orb_sim3_search_info_t> searchInfo(noSearch);

  ORBmatcher m(nnratio, hdr[5] != 0);
  const ORBmatcher::BowSlots kf{keys.p, desc.p, nkeys.p, nodes.p, offs.p, feats.p, nnodes.p};
  m.search_by_bow_kf_batch((int)P, slot1.p, slot2.p, kf, pidx.p, (int)S, points.p, hdr[6],
                           match.p, index2.p, bowInfo.p);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  put(o, match.host());
  put(o, index2.host());
  put(o, bowInfo.host());
  m.search_by_sim3_batch((int)P, slot1.p, slot2.p, keys.p, desc.p, nkeys.p, pidx.p, pose.p,
                         (int)S, points.p, mpDesc.p, match.p, index2.p, nullptr, sim3.p, nullptr,
                         cam, 0.f, hv[0], 0.f, hv[1], scale, hv[2], hv[3], new12.p, searchInfo.p);
  put(o, match.host());
  put(o, index2.host());
  put(o, new12.host());
  put(o, searchInfo.host());
  std::fclose(o);
  std::printf("OK\n");
  return 0;
}
