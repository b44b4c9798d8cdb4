// The C++ host mirror's device-batched SearchByBoW(KF, F) and the strided-count
// discard call on problems packed by tests/test_cpp_bow_batch.py:
//   test_bow_batch_host <in> <out>
// <in>:  int32 header {P, stride, mp_stride, min_matches, check_ori}, float
//        nnratio, then per side (keyframes, frames) keys, desc, nkeys, fv_nodes,
//        fv_offs, fv_feats, n_fv_nodes, then point_index and the points.
// <out>: kp_match (P * stride int32), info (P records), then the discard call's
//        records on those matches with every third keypoint flagged.
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

struct Side {
  Dev<KeyPoint> keys;
  Dev<uint8_t> desc;
  Dev<int32_t> nkeys;
  Dev<uint32_t> nodes;
  Dev<int32_t> offs;
  Dev<uint32_t> feats;
  Dev<int32_t> nnodes;
  Side(std::FILE* f, size_t P, size_t S)
      : keys(take<KeyPoint>(f, P * S)), desc(take<uint8_t>(f, P * S * 32)),
        nkeys(take<int32_t>(f, P)), nodes(take<uint32_t>(f, P * S)),
        offs(take<int32_t>(f, P * (S + 1))), feats(take<uint32_t>(f, P * S)),
        nnodes(take<int32_t>(f, P)) {}
  ORBmatcher::BowSlots slots() const {
    return ORBmatcher::BowSlots{keys.p, desc.p, nkeys.p, nodes.p, offs.p, feats.p, nnodes.p};
  }
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  const std::vector<int32_t> hdr = take<int32_t>(in, 5);
  const float nnratio = take<float>(in, 1)[0];
  const int P = hdr[0], S = hdr[1], MS = hdr[2], minMatches = hdr[3];
  Side kf(in, P, S), fr(in, P, S);
  Dev<int32_t> pidx(take<int32_t>(in, (size_t)P * S));
  Dev<orb_map_point_t> pts(take<orb_map_point_t>(in, (size_t)P * MS));
  std::fclose(in);
  const std::vector<int32_t> junk((size_t)P * S, 77);
  const std::vector<orb_bow_match_info_t> noInfo(P);
  const std::vector<orb_track_discard_info_t> noOut(P);
  Dev<int32_t> match(junk);
  Dev<orb_bow_match_info_t> info(noInfo);
  static_assert(sizeof(orb_bow_match_info_t) == 20, "five int32 fields");

  ORBmatcher m(nnratio, hdr[4] != 0);
  if (ORBmatcher::search_by_bow_batch_max_stride() < 8192) return 3;
  m.search_by_bow_batch(P, nullptr, nullptr, kf.slots(), pidx.p, fr.slots(), S, pts.p, MS,
                        minMatches, match.p, info.p);
  const std::vector<int32_t> km = match.host();
  const std::vector<orb_bow_match_info_t> hinfo = info.host();

  // the discard loop on those matches, its count read from the BoW records
  std::vector<uint8_t> flagged((size_t)P * S, 0);
  for (size_t i = 0; i < flagged.size(); i += 3) flagged[i] = 1;
  Dev<uint8_t> outlier(flagged);
  Dev<orb_track_discard_info_t> out(noOut);
  m.track_discard_outliers_batch_n(P, fr.nkeys.p, S, match.p, outlier.p, pts.p, MS, true,
                                   &info.p->n_matches, 5, out.p);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  put(o, km);
  put(o, hinfo);
  put(o, out.host());
  put(o, match.host());
  std::fclose(o);
  std::printf("OK\n");
  return 0;
}
