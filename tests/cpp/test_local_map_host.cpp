// The C++ host mirror's UpdateLocalMap batch and the two tails of TrackLocalMap
// on problems packed by tests/test_cpp_local_map.py:
//   test_local_map_host <in> <out>
// <in>:  int32 header {P, n_kf, n_mp, kp_stride, kf_stride, mp_stride, then the
//        lengths of kf_cov, kf_child, kf_mp, mp_obs}, the view's arrays in the
//        order of orb_map_view_t, then nkeys, kp_match, local_kf, n_local_kf,
//        and for the tails km_local and outlier.
// <out>: kp_match, local_kf, n_local_kf, local_index, mps, mp_desc, nmps, locked,
//        info; then kp_match after the merge, after the finish, and n_inliers.
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
  const std::vector<int32_t> hdr = take<int32_t>(in, 10);
  const size_t P = hdr[0], NK = hdr[1], NM = hdr[2], S = hdr[3], KS = hdr[4], MS = hdr[5];
  Dev<int32_t> rank(take<int32_t>(in, NK)), byRank(take<int32_t>(in, NK));
  Dev<uint8_t> kfBad(take<uint8_t>(in, NK));
  Dev<int32_t> parent(take<int32_t>(in, NK));
  Dev<int32_t> covOffs(take<int32_t>(in, NK + 1)), cov(take<int32_t>(in, hdr[6]));
  Dev<int32_t> childOffs(take<int32_t>(in, NK + 1)), child(take<int32_t>(in, hdr[7]));
  Dev<int32_t> mpOffs(take<int32_t>(in, NK + 1)), kfMp(take<int32_t>(in, hdr[8]));
  Dev<int32_t> obsOffs(take<int32_t>(in, NM + 1)), obs(take<int32_t>(in, hdr[9]));
  Dev<orb_map_point_t> points(take<orb_map_point_t>(in, NM));
  Dev<uint8_t> desc(take<uint8_t>(in, NM * 32));
  Dev<int32_t> nkeys(take<int32_t>(in, P)), match(take<int32_t>(in, P * S));
  Dev<int32_t> localKf(take<int32_t>(in, P * KS)), nLocalKf(take<int32_t>(in, P));
  Dev<int32_t> kmLocal(take<int32_t>(in, P * S));
  Dev<uint8_t> outlier(take<uint8_t>(in, P * S));
  std::fclose(in);
  static_assert(sizeof(orb_local_map_info_t) == 32, "eight int32 fields");
  static_assert(sizeof(orb_map_point_t) == 36, "the gathered record");

  orb_map_view_t view;
  std::memset(&view, 0, sizeof(view));
  view.n_kf = (int32_t)NK;
  view.n_mp = (int32_t)NM;
  view.kf_rank = rank.p; view.kf_by_rank = byRank.p; view.kf_bad = kfBad.p;
  view.kf_parent = parent.p;
  view.kf_cov_offs = covOffs.p; view.kf_cov = cov.p;
  view.kf_child_offs = childOffs.p; view.kf_child = child.p;
  view.kf_mp_offs = mpOffs.p; view.kf_mp = kfMp.p;
  view.mp_obs_offs = obsOffs.p; view.mp_obs = obs.p;
  view.points = points.p; view.mp_desc = desc.p;

  const std::vector<int32_t> junkIdx(P * MS, 77), junkP(P, 77);
  const std::vector<orb_map_point_t> noPts(P * MS);
  const std::vector<uint8_t> junkDesc(P * MS * 32, 77), junkLocked(P * S, 77);
  const std::vector<orb_local_map_info_t> noInfo(P);
  Dev<int32_t> localIndex(junkIdx), nmps(junkP), nInliers(junkP);
  Dev<orb_map_point_t> mps(noPts);
  Dev<uint8_t> mpDesc(junkDesc), locked(junkLocked);
  Dev<orb_local_map_info_t> info(noInfo);

  ORBmatcher m(0.8f, true);
  if (ORBmatcher::update_local_map_max_keyframes() < 1024) return 3;
  m.update_local_map_batch((int)P, view, nkeys.p, match.p, (int)S, localKf.p, nLocalKf.p, (int)KS,
                           localIndex.p, mps.p, mpDesc.p, nmps.p, (int)MS, locked.p, info.p);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  put(o, match.host());
  put(o, localKf.host());
  put(o, nLocalKf.host());
  put(o, localIndex.host());
  put(o, mps.host());
  put(o, mpDesc.host());
  put(o, nmps.host());
  put(o, locked.host());
  put(o, info.host());
  m.track_local_merge_batch((int)P, nkeys.p, (int)S, kmLocal.p, localIndex.p, (int)MS, match.p);
  put(o, match.host());
  m.track_local_map_finish_batch((int)P, nkeys.p, (int)S, match.p, outlier.p, points.p, 0, false,
                                 true, nInliers.p);
  put(o, match.host());
  put(o, nInliers.host());
  std::fclose(o);
  std::printf("OK\n");
  return 0;
}
