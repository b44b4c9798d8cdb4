// The C++ host mirror's Sim3Solver on one problem packed by
// tests/test_cpp_sim3.py:
//   test_sim3_host <in> <out>
// <in>:  int32 header {stride, n_slots, n_points, n_levels, fix_scale,
//        draw_stride, has_index1, rounds_of}, then kf1_slot, kf2_slot, keys,
//        nkeys, point_index, pose, points, match12, index2, index1 (when
//        present), draws, level_sigma2, cam1, cam2 (six floats each).
// <out>: after setup: state, corr; then rounds of iterate(rounds_of) until a
//        Sim3 or bNoMore: state, corr, result, inliers12; then find() on a
//        solver set up again: state, result, and the three getters.
// Plain g++: the HIP runtime calls it needs are declared by hand.
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
  const std::vector<int32_t> hdr = take<int32_t>(in, 8);
  const size_t S = hdr[0], NS = hdr[1], NP = hdr[2];
  Dev<int32_t> slot1(take<int32_t>(in, 1)), slot2(take<int32_t>(in, 1));
  Dev<KeyPoint> keys(take<KeyPoint>(in, NS * S));
  Dev<int32_t> nkeys(take<int32_t>(in, NS)), pidx(take<int32_t>(in, NS * S));
  Dev<orb_pose_t> pose(take<orb_pose_t>(in, NS));
  Dev<orb_map_point_t> pts(take<orb_map_point_t>(in, NP));
  Dev<int32_t> match12(take<int32_t>(in, S)), index2(take<int32_t>(in, S));
  Dev<int32_t> index1(take<int32_t>(in, hdr[6] ? S : 0));
  Dev<uint32_t> draws(take<uint32_t>(in, hdr[5]));
  const std::vector<float> sigma2 = take<float>(in, hdr[3]);
  const orb_camera_t cam1 = take<orb_camera_t>(in, 1)[0], cam2 = take<orb_camera_t>(in, 1)[0];
  std::fclose(in);
  static_assert(sizeof(orb_sim3_corr_t) == 56 && sizeof(orb_sim3_state_t) == 184 &&
                    sizeof(orb_sim3_result_t) == 132,
                "ABI records");
  if (ORBmatcher::sim3_solver_max_stride() < 2048) return 3;

  Dev<orb_sim3_state_t> state(std::vector<orb_sim3_state_t>(1));
  std::vector<uint8_t> junk(S * sizeof(orb_sim3_corr_t), 0x5A);
  Dev<uint8_t> corr(junk);
  Dev<uint8_t> inl(std::vector<uint8_t>(S, 0x5A));
  Dev<orb_sim3_result_t> res(std::vector<orb_sim3_result_t>(1));

  ORBmatcher m(0.75f, true);
  Sim3Solver::Problem pr{slot1.p, slot2.p, keys.p, nkeys.p, pidx.p, pose.p, (int)S, pts.p,
                         match12.p, hdr[6] ? index1.p : nullptr, index2.p, draws.p, hdr[5],
                         2147483647u, state.p, (orb_sim3_corr_t*)corr.p, inl.p, res.p};
  auto toHost = [](void* dst, const void* src, size_t n) {
    hipDeviceSynchronize();
    hipMemcpy(dst, src, n, 2);
  };
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  Sim3Solver solver(m, pr, sigma2, cam1, cam2, hdr[4] != 0, toHost);
  solver.SetRansacParameters(0.99, 20, 300);
  put(o, state.host());
  put(o, corr.host());
  bool bNoMore = false, ok = false;
  std::vector<bool> vbInliers;
  int nInliers = 0;
  float T12[16] = {0};
  for (int round = 0; round < 61 && !ok && !bNoMore; ++round)
    ok = solver.iterate(hdr[7], bNoMore, vbInliers, nInliers, T12);
  put(o, state.host());
  put(o, corr.host());
  put(o, res.host());
  put(o, inl.host());
  if (ok && (std::count(vbInliers.begin(), vbInliers.end(), true) != nInliers ||
             std::memcmp(T12, solver.result().T12, sizeof(T12)) != 0)) {
    std::printf("FAIL inliers\n");
    return 1;
  }

  Sim3Solver again(m, pr, sigma2, cam1, cam2, hdr[4] != 0, toHost);
  float T[16] = {0};
  const bool found = again.find(vbInliers, nInliers, T);
  put(o, state.host());
  put(o, res.host());
  std::vector<float> g(13);
  again.GetEstimatedRotation(g.data());
  again.GetEstimatedTranslation(g.data() + 9);
  g[12] = again.GetEstimatedScale();
  put(o, g);
  std::fclose(o);
  std::printf("OK %d %d\n", ok ? 1 : 0, found ? 1 : 0);
  return 0;
}
