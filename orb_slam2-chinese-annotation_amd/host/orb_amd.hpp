// orb_amd.hpp -- C++ host mirror of ORB_SLAM2::ORBextractor / ORB_SLAM2::ORBmatcher
// over the C ABI (include/orb_abi.h).  Header-only, C++17, no OpenCV.
//
// Same member names, argument meaning and error behaviour as the reference
// classes (include/ORBextractor.h:45-114, include/ORBmatcher.h:37-102), with
// cv::Mat / cv::KeyPoint replaced by plain views:
//   cv::KeyPoint            -> orb_keypoint_t  (identical 28-byte layout)
//   cv::Mat N x 32 CV_8U    -> Descriptors      (row-major N x 32 bytes)
//   cv::Mat 8UC1 image      -> ImageView        (pointer, width, height, stride)
// The OpenCV-typed drop-in a maintainer compiles into the reference tree is in
// INTEGRATION.md; it forwards to these calls.
#pragma once

#include <algorithm>
#include <cassert>
#include <cstdint>
#include <functional>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/orb_abi.h"

namespace orb_amd {

struct Error : std::runtime_error {
  orb_status_t status;
  Error(orb_status_t s, const std::string& what)
      : std::runtime_error(what + ": " + orb_status_string(s)), status(s) {}
};

inline void check(orb_status_t s, const char* what) {
  if (s != ORB_OK) throw Error(s, what);
}

using KeyPoint = orb_keypoint_t;

struct ImageView {
  const uint8_t* data = nullptr;
  int width = 0, height = 0;
  size_t stride = 0;  // bytes between rows
  bool empty() const { return !data || width <= 0 || height <= 0; }
};

struct Descriptors {
  int rows = 0;
  std::vector<uint8_t> data;  // rows x 32
  const uint8_t* row(int i) const { return data.data() + (size_t)i * ORB_DESC_BYTES; }
  bool empty() const { return rows == 0; }
};

struct Image {
  int width = 0, height = 0;
  std::vector<uint8_t> data;
  ImageView view() const { return {data.data(), width, height, (size_t)width}; }
};

// ---------------------------------------------------------------- extractor
class ORBextractor {
 public:
  enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

  ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST,
               int device = 0) {
    check(orb_extractor_create(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device,
                               &h_),
          "ORBextractor");
  }
  ~ORBextractor() { orb_extractor_destroy(h_); }
  ORBextractor(const ORBextractor&) = delete;
  ORBextractor& operator=(const ORBextractor&) = delete;

  // operator()(image, mask, keypoints, descriptors) -- src/ORBextractor.cc:1091-1169.
  // Empty image: returns with the outputs untouched (:1095-1096).  The mask is
  // ignored, as in the reference (include/ORBextractor.h:58).
  void operator()(const ImageView& image, const ImageView& /*mask*/,
                  std::vector<KeyPoint>& keypoints, Descriptors& descriptors) {
    if (image.empty()) return;
    const int cap = orb_extractor_capacity(h_, image.width, image.height);
    assert(cap >= 0 && "image too small/large for this pyramid");  // reference: assert (:1100)
    if (cap < 0) throw Error(ORB_EINVAL, "ORBextractor::operator()");
    keypoints.resize(cap);
    descriptors.data.resize((size_t)cap * ORB_DESC_BYTES);
    int n = 0;
    check(orb_extractor_extract(h_, image.data, image.width, image.height, image.stride,
                                keypoints.data(), descriptors.data.data(), cap, &n),
          "ORBextractor::operator()");
    keypoints.resize(n);
    descriptors.data.resize((size_t)n * ORB_DESC_BYTES);
    descriptors.rows = n;
  }

  int GetLevels() { return orb_extractor_get_levels(h_); }
  float GetScaleFactor() { return orb_extractor_get_scale_factor(h_); }
  std::vector<float> GetScaleFactors() { return floats(orb_extractor_get_scale_factors); }
  std::vector<float> GetInverseScaleFactors() {
    return floats(orb_extractor_get_inverse_scale_factors);
  }
  std::vector<float> GetScaleSigmaSquares() { return floats(orb_extractor_get_scale_sigma_squares); }
  std::vector<float> GetInverseScaleSigmaSquares() {
    return floats(orb_extractor_get_inverse_scale_sigma_squares);
  }

  // mvImagePyramid (include/ORBextractor.h:85): host copies of the last image's levels.
  std::vector<Image> ImagePyramid() {
    std::vector<Image> out(GetLevels());
    for (int l = 0; l < (int)out.size(); ++l) {
      check(orb_extractor_pyramid_level(h_, l, nullptr, 0, &out[l].width, &out[l].height),
            "mvImagePyramid");
      out[l].data.resize((size_t)out[l].width * out[l].height);
      check(orb_extractor_pyramid_level(h_, l, out[l].data.data(), out[l].width, nullptr, nullptr),
            "mvImagePyramid");
    }
    return out;
  }

  orb_extractor_t* handle() { return h_; }

 private:
  std::vector<float> floats(void (*fn)(const orb_extractor_t*, float*)) {
    std::vector<float> v(GetLevels());
    fn(h_, v.data());
    return v;
  }
  orb_extractor_t* h_ = nullptr;
};

// --------------------------------------------------------------- DBoW2 types
// DBoW2::BowVector (std::map<WordId, WordValue>, Thirdparty/DBoW2/DBoW2/BowVector.h)
// and DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned int>>,
// FeatureVector.h): the same containers, so Frame::mBowVec / mFeatVec keep their
// types.  CsrFeatureVector is the flat form the C ABI takes.
using WordId = uint32_t;
using NodeId = uint32_t;
using BowVector = std::map<WordId, double>;
using FeatureVector = std::map<NodeId, std::vector<unsigned int>>;

struct CsrFeatureVector {
  std::vector<uint32_t> nodes;
  std::vector<int32_t> offs{0};
  std::vector<uint32_t> feats;
  int size() const { return (int)nodes.size(); }
};

inline CsrFeatureVector flatten(const FeatureVector& fv) {
  CsrFeatureVector c;
  c.nodes.reserve(fv.size());
  c.offs.reserve(fv.size() + 1);
  for (const auto& it : fv) {
    c.nodes.push_back(it.first);
    c.feats.insert(c.feats.end(), it.second.begin(), it.second.end());
    c.offs.push_back((int32_t)c.feats.size());
  }
  return c;
}

// ORBVocabulary = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>
// (include/ORBVocabulary.h), device-resident.  loadFromTextFile as
// TemplatedVocabulary.h:1362-1448 (returns false on a malformed header);
// transform as Frame::ComputeBoW calls it (src/Frame.cc:439-449:
// transform(vCurrentDesc, mBowVec, mFeatVec, 4)).
class ORBVocabulary {
 public:
  explicit ORBVocabulary(int device = 0) : device_(device) {}
  ~ORBVocabulary() { orb_vocabulary_destroy(h_); }
  ORBVocabulary(const ORBVocabulary&) = delete;
  ORBVocabulary& operator=(const ORBVocabulary&) = delete;

  bool loadFromTextFile(const std::string& filename) {
    orb_vocabulary_t* h = nullptr;
    if (orb_vocabulary_load_text(device_, filename.c_str(), &h) != ORB_OK) return false;
    orb_vocabulary_destroy(h_);
    h_ = h;
    return true;
  }
  // Node table form (node 0 = root; parent[i] < i; entry 0 ignored).
  void create(int k, int L, int scoring, int weighting, const std::vector<int32_t>& parent,
              const std::vector<uint8_t>& leaf, const std::vector<uint8_t>& descriptors,
              const std::vector<double>& weights) {
    orb_vocabulary_t* h = nullptr;
    check(orb_vocabulary_create(device_, k, L, scoring, weighting, (int)parent.size(),
                                parent.data(), leaf.data(), descriptors.data(), weights.data(),
                                &h),
          "ORBVocabulary::create");
    orb_vocabulary_destroy(h_);
    h_ = h;
  }
  unsigned int size() const { return (unsigned)info()[5]; }
  bool empty() const { return size() == 0; }
  unsigned int getBranchingFactor() const { return (unsigned)info()[0]; }
  unsigned int getDepthLevels() const { return (unsigned)info()[1]; }

  // transform(const vector<cv::Mat>& features, BowVector&, FeatureVector&, levelsup),
  // TemplatedVocabulary.h:1128-1210; desc rows are the features in order.
  void transform(const Descriptors& desc, BowVector& v, FeatureVector& fv, int levelsup) const {
    v.clear();
    fv.clear();
    if (!h_ || desc.rows == 0) return;
    const int n = desc.rows;
    std::vector<uint32_t> bw(n), fvn(n), fvf(n);
    std::vector<double> bv(n);
    std::vector<int32_t> fvo(n + 1);
    int32_t nw = 0, nf = 0;
    check(orb_vocabulary_transform(h_, n, desc.data.data(), levelsup, bw.data(), bv.data(), &nw,
                                   fvn.data(), fvo.data(), fvf.data(), &nf, nullptr, nullptr),
          "ORBVocabulary::transform");
    for (int i = 0; i < nw; ++i) v.emplace_hint(v.end(), bw[i], bv[i]);
    for (int j = 0; j < nf; ++j)
      fv.emplace_hint(fv.end(), fvn[j],
                      std::vector<unsigned int>(fvf.begin() + fvo[j], fvf.begin() + fvo[j + 1]));
  }
  // score(const BowVector& a, const BowVector& b), TemplatedVocabulary.h ->
  // ScoringObject.cpp:23-311 with the vocabulary's scoring type (KL: assert).
  double score(const BowVector& a, const BowVector& b) const {
    std::vector<uint32_t> aw, bw;
    std::vector<double> av, bv;
    flatten(a, aw, av);
    flatten(b, bw, bv);
    const int32_t ao[2] = {0, (int32_t)aw.size()}, bo[2] = {0, (int32_t)bw.size()};
    double out = 0.0;
    check(orb_vocabulary_score(h_, 1, ao, aw.data(), av.data(), bo, bw.data(), bv.data(), &out),
          "ORBVocabulary::score");
    return out;
  }
  static void flatten(const BowVector& v, std::vector<uint32_t>& words,
                      std::vector<double>& values) {
    words.reserve(v.size());
    values.reserve(v.size());
    for (const auto& it : v) {
      words.push_back(it.first);
      values.push_back(it.second);
    }
  }
  orb_vocabulary_t* handle() { return h_; }

 private:
  std::vector<int32_t> info() const {
    std::vector<int32_t> i(6, 0);
    if (h_) orb_vocabulary_info(h_, i.data());
    return i;
  }
  int device_;
  orb_vocabulary_t* h_ = nullptr;
};

// KeyFrameDatabase (src/KeyFrameDatabase.cc) over keyframe ids (KeyFrame::mnId),
// device-resident.  A keyframe is its id, its mBowVec and, once known, the ids
// of GetBestCovisibilityKeyFrames(10); the queries return candidate ids in the
// reference's order.  The vocabulary must outlive the database.
class KeyFrameDatabase {
 public:
  explicit KeyFrameDatabase(ORBVocabulary& voc) {
    check(orb_kf_database_create(voc.handle(), &h_), "KeyFrameDatabase");
  }
  ~KeyFrameDatabase() { orb_kf_database_destroy(h_); }
  KeyFrameDatabase(const KeyFrameDatabase&) = delete;
  KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

  void add(int64_t kfId, const BowVector& bow) {  // :42-49
    std::vector<uint32_t> w;
    std::vector<double> v;
    ORBVocabulary::flatten(bow, w, v);
    check(orb_kf_database_add(h_, kfId, (int)w.size(), w.data(), v.data()),
          "KeyFrameDatabase::add");
  }
  void erase(int64_t kfId) { check(orb_kf_database_erase(h_, kfId), "KeyFrameDatabase::erase"); }
  void clear() { check(orb_kf_database_clear(h_), "KeyFrameDatabase::clear"); }
  int size() const { return orb_kf_database_size(h_); }
  // snapshot of pKF->GetBestCovisibilityKeyFrames(10), read at :155 and :286
  void SetBestCovisibilityKeyFrames(int64_t kfId, const std::vector<int64_t>& ids) {
    check(orb_kf_database_set_covisibility(h_, kfId, (int)ids.size(), ids.data()),
          "KeyFrameDatabase::SetBestCovisibilityKeyFrames");
  }
  // DetectLoopCandidates(pKF, minScore) (:79-202): kfId = pKF->mnId, connected =
  // the ids of pKF->GetConnectedKeyFrames().
  std::vector<int64_t> DetectLoopCandidates(uint64_t kfId, const BowVector& bow,
                                            const std::vector<int64_t>& connected,
                                            float minScore) {
    std::vector<uint32_t> w;
    std::vector<double> v;
    ORBVocabulary::flatten(bow, w, v);
    std::vector<int64_t> out((size_t)std::max(size(), 1));
    int n = 0;
    check(orb_kf_database_detect_loop(h_, kfId, (int)w.size(), w.data(), v.data(),
                                      (int)connected.size(), connected.data(), minScore,
                                      out.data(), (int)out.size(), &n),
          "KeyFrameDatabase::DetectLoopCandidates");
    out.resize((size_t)n);
    return out;
  }
  // DetectRelocalizationCandidates(F) (:205-339): frameId = F->mnId.
  std::vector<int64_t> DetectRelocalizationCandidates(uint64_t frameId, const BowVector& bow) {
    std::vector<uint32_t> w;
    std::vector<double> v;
    ORBVocabulary::flatten(bow, w, v);
    std::vector<int64_t> out((size_t)std::max(size(), 1));
    int n = 0;
    check(orb_kf_database_detect_relocalization(h_, frameId, (int)w.size(), w.data(), v.data(),
                                                out.data(), (int)out.size(), &n),
          "KeyFrameDatabase::DetectRelocalizationCandidates");
    out.resize((size_t)n);
    return out;
  }
  orb_kf_database_t* handle() { return h_; }

 private:
  orb_kf_database_t* h_ = nullptr;
};

// ------------------------------------------------------------------ matcher
// The matcher-side Frame / MapPoint state, flattened (what ORBmatcher reads).
struct FrameView {
  std::vector<KeyPoint> mvKeysUn;
  Descriptors mDescriptors;
  std::vector<float> mvuRight;  // empty = monocular
  float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
  std::vector<float> mvScaleFactors;
  int N() const { return (int)mvKeysUn.size(); }
  orb_frame_t c() const {
    orb_frame_t f;
    f.n = N();
    f.keys = mvKeysUn.data();
    f.descriptors = mDescriptors.data.data();
    f.u_right = mvuRight.empty() ? nullptr : mvuRight.data();
    f.min_x = mnMinX;
    f.max_x = mnMaxX;
    f.min_y = mnMinY;
    f.max_y = mnMaxY;
    f.n_levels = (int)mvScaleFactors.size();
    f.scale_factors = mvScaleFactors.data();
    return f;
  }
};

class ORBmatcher {
 public:
  static const int TH_LOW = 50;
  static const int TH_HIGH = 100;
  static const int HISTO_LENGTH = 30;

  explicit ORBmatcher(float nnratio = 0.6f, bool checkOri = true, int device = 0)
      : mfNNratio(nnratio), mbCheckOrientation(checkOri) {
    check(orb_matcher_create(device, &h_), "ORBmatcher");
  }
  ~ORBmatcher() { orb_matcher_destroy(h_); }
  ORBmatcher(const ORBmatcher&) = delete;
  ORBmatcher& operator=(const ORBmatcher&) = delete;

  // static int DescriptorDistance(const cv::Mat&, const cv::Mat&) -- src/ORBmatcher.cc:1814-1830
  static int DescriptorDistance(const uint8_t* a, const uint8_t* b) {
    return orb_descriptor_distance(a, b);
  }

  // SearchByProjection(Frame&, const vector<MapPoint*>&, th) -- src/ORBmatcher.cc:47-133.
  // mvpMapPoints[i] is the map-point index assigned to keypoint i (-1 = NULL);
  // on entry locked[i] = (mvpMapPoints[i] && Observations() > 0).  Returns nmatches.
  int SearchByProjection(const FrameView& F, const std::vector<orb_mp_track_t>& mps,
                         const std::vector<uint8_t>& mpDescriptors, float th,
                         std::vector<int32_t>& mvpMapPoints,
                         const std::vector<uint8_t>& locked = {}) {
    const orb_frame_t f = F.c();
    std::vector<int32_t> km(F.N(), -1);
    int32_t n = 0;
    check(orb_match_projection_local(h_, &f, locked.empty() ? nullptr : locked.data(),
                                     (int)mps.size(), mps.data(), mpDescriptors.data(), th,
                                     mfNNratio, km.data(), &n),
          "SearchByProjection");
    if ((int)mvpMapPoints.size() != F.N()) mvpMapPoints.assign(F.N(), -1);
    for (int i = 0; i < F.N(); ++i)
      if (km[i] >= 0) mvpMapPoints[i] = km[i];
    return n;
  }

  // SearchByProjection(CurrentFrame, LastFrame, th, bMono) -- src/ORBmatcher.cc:1460-1619.
  // Limit (ORB_ECAPACITY, nothing launched): with N = current.N() and
  // W = ceil(N / 32), both rounded up to 4,
  // 4 * (W + 2 * N + max(last.size(), 1)) + 128 bytes must fit 160 KiB.
  int SearchByProjection(const FrameView& current, const std::vector<orb_last_mp_t>& last,
                         const std::vector<uint8_t>& lastDescriptors, const orb_camera_t& cam,
                         float tlc_z, float th, bool bMono, std::vector<int32_t>& mvpMapPoints,
                         const std::vector<uint8_t>& locked = {}) {
    const orb_frame_t f = current.c();
    std::vector<int32_t> km(current.N(), -1);
    int32_t n = 0;
    check(orb_match_projection_frame(h_, &f, locked.empty() ? nullptr : locked.data(),
                                     (int)last.size(), last.data(), lastDescriptors.data(), &cam,
                                     tlc_z, th, bMono ? 1 : 0, mbCheckOrientation ? 1 : 0,
                                     km.data(), &n),
          "SearchByProjection(F, LastFrame)");
    if ((int)mvpMapPoints.size() != current.N()) mvpMapPoints.assign(current.N(), -1);
    for (int i = 0; i < current.N(); ++i) {
      if (km[i] >= 0) mvpMapPoints[i] = km[i];
      else if (km[i] == -2) mvpMapPoints[i] = -1;  // rotation filter reset
    }
    return n;
  }

  // Frame::ComputeStereoMatches -- src/Frame.cc:516-704 (mvuRight, mvDepth).
  void ComputeStereoMatches(const FrameView& left, const std::vector<KeyPoint>& rightKeys,
                            const Descriptors& rightDesc, const std::vector<Image>& leftPyr,
                            const std::vector<Image>& rightPyr,
                            const std::vector<float>& invScale, float bf, float fx,
                            std::vector<float>& mvuRight, std::vector<float>& mvDepth) {
    const int L = (int)leftPyr.size();
    std::vector<const uint8_t*> lp(L), rp(L);
    std::vector<int32_t> w(L), hh(L);
    std::vector<int64_t> st(L);
    for (int l = 0; l < L; ++l) {
      lp[l] = leftPyr[l].data.data();
      rp[l] = rightPyr[l].data.data();
      w[l] = leftPyr[l].width;
      hh[l] = leftPyr[l].height;
      st[l] = leftPyr[l].width;
    }
    const orb_frame_t f = left.c();
    orb_stereo_input_t in;
    in.left = &f;
    in.n_right = (int)rightKeys.size();
    in.right_keys = rightKeys.data();
    in.right_desc = rightDesc.data.data();
    in.n_levels = L;
    in.left_levels = lp.data();
    in.right_levels = rp.data();
    in.level_width = w.data();
    in.level_height = hh.data();
    in.level_stride = st.data();
    in.inv_scale_factors = invScale.data();
    in.bf = bf;
    in.fx = fx;
    mvuRight.assign(left.N(), -1.0f);
    mvDepth.assign(left.N(), -1.0f);
    check(orb_stereo_match(h_, &in, mvuRight.data(), mvDepth.data()), "ComputeStereoMatches");
  }

  // SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches),
  // src/ORBmatcher.cc:164-306.  kfMapPoints[i] = MapPoint id of KF keypoint i or
  // -1; kfBad[i] = isBad().  vpMapPointMatches (out) = MapPoint id per F keypoint.
  int SearchByBoW(const FrameView& KF, const std::vector<int32_t>& kfMapPoints,
                  const std::vector<uint8_t>& kfBad, const FeatureVector& kfFeatVec,
                  const FrameView& F, const FeatureVector& fFeatVec,
                  std::vector<int32_t>& vpMapPointMatches) {
    const CsrFeatureVector a = flatten(kfFeatVec), b = flatten(fFeatVec);
    const std::vector<float> ka = angles(KF), fa = angles(F);
    vpMapPointMatches.assign(F.N(), -1);
    int32_t n = 0;
    check(orb_match_bow(h_, KF.N(), KF.mDescriptors.data.data(), ka.data(), kfMapPoints.data(),
                        kfBad.empty() ? nullptr : kfBad.data(), a.size(), a.nodes.data(),
                        a.offs.data(), a.feats.data(), F.N(), F.mDescriptors.data.data(),
                        fa.data(), b.size(), b.nodes.data(), b.offs.data(), b.feats.data(),
                        mfNNratio, mbCheckOrientation ? 1 : 0, vpMapPointMatches.data(), &n),
          "SearchByBoW(KF, F)");
    return n;
  }

  // SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12),
  // src/ORBmatcher.cc:581-716.  vpMatches12 (out) = KF2 MapPoint id per KF1 keypoint.
  int SearchByBoW(const FrameView& KF1, const std::vector<int32_t>& mp1,
                  const std::vector<uint8_t>& bad1, const FeatureVector& fv1,
                  const FrameView& KF2, const std::vector<int32_t>& mp2,
                  const std::vector<uint8_t>& bad2, const FeatureVector& fv2,
                  std::vector<int32_t>& vpMatches12) {
    const CsrFeatureVector a = flatten(fv1), b = flatten(fv2);
    const std::vector<float> a1 = angles(KF1), a2 = angles(KF2);
    vpMatches12.assign(KF1.N(), -1);
    int32_t n = 0;
    check(orb_match_bow_kf(h_, KF1.N(), KF1.mDescriptors.data.data(), a1.data(), mp1.data(),
                           bad1.empty() ? nullptr : bad1.data(), a.size(), a.nodes.data(),
                           a.offs.data(), a.feats.data(), KF2.N(), KF2.mDescriptors.data.data(),
                           a2.data(), mp2.data(), bad2.empty() ? nullptr : bad2.data(), b.size(),
                           b.nodes.data(), b.offs.data(), b.feats.data(), mfNNratio,
                           mbCheckOrientation ? 1 : 0, vpMatches12.data(), &n),
          "SearchByBoW(KF, KF)");
    return n;
  }

  // SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize),
  // src/ORBmatcher.cc:429-577.  vbPrevMatched as (x, y) pairs, updated in place.
  int SearchForInitialization(const FrameView& F1, const FrameView& F2,
                              std::vector<float>& vbPrevMatched, std::vector<int>& vnMatches12,
                              int windowSize = 10) {
    const orb_frame_t f1 = F1.c(), f2 = F2.c();
    std::vector<int32_t> m(F1.N(), -1);
    int32_t n = 0;
    check(orb_search_for_initialization(h_, &f1, &f2, vbPrevMatched.data(), windowSize,
                                        mfNNratio, mbCheckOrientation ? 1 : 0, m.data(), &n),
          "SearchForInitialization");
    vnMatches12.assign(m.begin(), m.end());
    return n;
  }

  // Tracking::SearchLocalPoints' isInFrustum pass (src/Tracking.cc:1360-1377,
  // src/Frame.cc:303-366); returns nToMatch, tracks feed SearchByProjection.
  int isInFrustum(const std::vector<orb_map_point_t>& mps, const orb_pose_t& pose,
                  const orb_camera_t& cam, const FrameView& F, float viewingCosLimit,
                  float logScaleFactor, std::vector<orb_mp_track_t>& tracks) {
    tracks.assign(mps.size(), orb_mp_track_t{});
    int32_t n = 0;
    check(orb_frustum(h_, (int)mps.size(), mps.data(), &pose, &cam, F.mnMinX, F.mnMaxX, F.mnMinY,
                      F.mnMaxY, viewingCosLimit, logScaleFactor, (int)F.mvScaleFactors.size(),
                      tracks.data(), &n),
          "isInFrustum");
    return n;
  }

  // MapPoint::ComputeDistinctiveDescriptors for many points (src/MapPoint.cc:250-326):
  // observation descriptors in CSR (obsOffs.size() = points + 1).  Returns BestIdx
  // per point (-1 for an empty list, whose descriptor row is left untouched).
  std::vector<int32_t> ComputeDistinctiveDescriptors(const std::vector<int32_t>& obsOffs,
                                                     const std::vector<uint8_t>& obsDesc,
                                                     std::vector<uint8_t>& descriptors) {
    const int n = (int)obsOffs.size() - 1;
    std::vector<int32_t> best(n > 0 ? n : 0, -1);
    if (n <= 0) return best;
    descriptors.resize((size_t)n * ORB_DESC_BYTES);
    check(orb_distinctive_descriptors(h_, n, obsOffs.data(),
                                      obsDesc.empty() ? nullptr : obsDesc.data(), best.data(),
                                      descriptors.data()),
          "ComputeDistinctiveDescriptors");
    return best;
  }

  // Fuse(KeyFrame* pKF, vpMapPoints, th), src/ORBmatcher.cc:903-1077 (match half):
  // fuseIdx[i] = keypoint point i fuses into, or -1.
  int Fuse(const FrameView& KF, const std::vector<float>& invLevelSigma2, const orb_pose_t& pose,
           const orb_camera_t& cam, float logScaleFactor,
           const std::vector<orb_map_point_t>& mps, const std::vector<uint8_t>& mpDesc, float th,
           std::vector<int32_t>& fuseIdx) {
    const orb_frame_t f = KF.c();
    fuseIdx.assign(mps.size(), -1);
    int32_t n = 0;
    check(orb_fuse(h_, &f, invLevelSigma2.data(), &pose, &cam, logScaleFactor, (int)mps.size(),
                   mps.data(), mpDesc.data(), th, fuseIdx.data(), &n),
          "Fuse");
    return n;
  }

  // Fuse(KeyFrame* pKF, Scw, vpPoints, th, vpReplacePoint), src/ORBmatcher.cc:1079-1210.
  int Fuse(const FrameView& KF, const float scw[12], const orb_camera_t& cam,
           float logScaleFactor, const std::vector<orb_map_point_t>& mps,
           const std::vector<uint8_t>& mpDesc, float th, std::vector<int32_t>& fuseIdx) {
    const orb_frame_t f = KF.c();
    fuseIdx.assign(mps.size(), -1);
    int32_t n = 0;
    check(orb_fuse_sim3(h_, &f, scw, &cam, logScaleFactor, (int)mps.size(), mps.data(),
                        mpDesc.data(), th, fuseIdx.data(), &n),
          "Fuse(KF, Scw)");
    return n;
  }

  // SearchByProjection(Frame& F, KeyFrame* pKF, sAlreadyFound, th, ORBdist),
  // src/ORBmatcher.cc:1622-1759: kpMatch[j] = point assigned, -1 none, -2 reset.
  // Limit of this overload and the Scw one below (ORB_ECAPACITY, nothing
  // launched): with N = F.N() and W = ceil(N / 32), both rounded up to 4,
  // 4 * (W + N + max(mps.size(), 1)) + 128 bytes must fit 160 KiB.
  int SearchByProjection(const FrameView& F, const std::vector<uint8_t>& locked,
                         const orb_pose_t& pose, const orb_camera_t& cam, float logScaleFactor,
                         const std::vector<orb_map_point_t>& mps,
                         const std::vector<uint8_t>& mpDesc, const std::vector<float>& kfAngle,
                         float th, int ORBdist, std::vector<int32_t>& kpMatch) {
    const orb_frame_t f = F.c();
    kpMatch.assign(F.N(), -1);
    int32_t n = 0;
    check(orb_search_by_projection_reloc(h_, &f, locked.empty() ? nullptr : locked.data(), &pose,
                                         &cam, logScaleFactor, (int)mps.size(), mps.data(),
                                         mpDesc.data(), kfAngle.data(), th, ORBdist,
                                         mbCheckOrientation ? 1 : 0, kpMatch.data(), &n),
          "SearchByProjection(F, KF)");
    return n;
  }

  // SearchByProjection(KeyFrame* pKF, Scw, vpPoints, vpMatched, th),
  // src/ORBmatcher.cc:311-425: vpMatched[j] = index into vpPoints or -1 (in/out).
  int SearchByProjection(const FrameView& KF, const float scw[12], const orb_camera_t& cam,
                         float logScaleFactor, const std::vector<orb_map_point_t>& mps,
                         const std::vector<uint8_t>& mpDesc, std::vector<int32_t>& vpMatched,
                         int th) {
    const orb_frame_t f = KF.c();
    if ((int)vpMatched.size() != KF.N()) vpMatched.assign(KF.N(), -1);
    int32_t n = 0;
    check(orb_search_by_projection_sim3(h_, &f, scw, &cam, logScaleFactor, (int)mps.size(),
                                        mps.data(), mpDesc.data(), (float)th, vpMatched.data(),
                                        &n),
          "SearchByProjection(KF, Scw)");
    return n;
  }

  // SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo),
  // src/ORBmatcher.cc:718-901.  hasMp[i] = GetMapPoint(i) != NULL; levelSigma2 =
  // pKF2->mvLevelSigma2; F12 row-major; Cw = pKF1 camera centre; R2w/t2w = pKF2
  // pose.  vMatchedPairs (out) = (i1, i2) in ascending i1.
  int SearchForTriangulation(const FrameView& KF1, const std::vector<uint8_t>& hasMp1,
                             const FeatureVector& fv1, const FrameView& KF2,
                             const std::vector<uint8_t>& hasMp2, const FeatureVector& fv2,
                             const std::vector<float>& levelSigma2, const float F12[9],
                             const orb_camera_t& cam, const float Cw[3], const float R2w[9],
                             const float t2w[3], bool bOnlyStereo,
                             std::vector<std::pair<size_t, size_t>>& vMatchedPairs) {
    const orb_frame_t f1 = KF1.c(), f2 = KF2.c();
    const CsrFeatureVector a = flatten(fv1), b = flatten(fv2);
    std::vector<int32_t> m12(KF1.N(), -1);
    int32_t n = 0;
    check(orb_search_for_triangulation(h_, &f1, hasMp1.data(), &f2, hasMp2.data(),
                                       levelSigma2.data(), F12, &cam, Cw, R2w, t2w, a.size(),
                                       a.nodes.data(), a.offs.data(), a.feats.data(), b.size(),
                                       b.nodes.data(), b.offs.data(), b.feats.data(),
                                       bOnlyStereo ? 1 : 0, mbCheckOrientation ? 1 : 0,
                                       m12.data(), &n),
          "SearchForTriangulation");
    vMatchedPairs.clear();
    vMatchedPairs.reserve(n);
    for (int i = 0; i < KF1.N(); ++i)
      if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);
    return n;
  }

  // SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th), src/ORBmatcher.cc:1212-1458.
  // mpsX / mpDescX = the MapPoint of keypoint i of KF X (validX[i] = non-NULL),
  // alreadyX = vbAlreadyMatchedX.  vpMatches12 (out) = idx2 per KF1 keypoint, or -1.
  int SearchBySim3(const FrameView& KF1, const FrameView& KF2, float logScaleFactor,
                   const orb_camera_t& cam, const float R1w[9], const float t1w[3],
                   const float R2w[9], const float t2w[3],
                   const std::vector<orb_map_point_t>& mps1, const std::vector<uint8_t>& valid1,
                   const std::vector<uint8_t>& already1, const std::vector<uint8_t>& mpDesc1,
                   const std::vector<orb_map_point_t>& mps2, const std::vector<uint8_t>& valid2,
                   const std::vector<uint8_t>& already2, const std::vector<uint8_t>& mpDesc2,
                   float s12, const float R12[9], const float t12[3], float th,
                   std::vector<int32_t>& vpMatches12) {
    const orb_frame_t f1 = KF1.c(), f2 = KF2.c();
    vpMatches12.assign(KF1.N(), -1);
    int32_t n = 0;
    check(orb_search_by_sim3(h_, &f1, &f2, logScaleFactor, &cam, R1w, t1w, R2w, t2w, mps1.data(),
                             valid1.data(), already1.data(), mpDesc1.data(), mps2.data(),
                             valid2.data(), already2.data(), mpDesc2.data(), s12, R12, t12, th,
                             vpMatches12.data(), &n),
          "SearchBySim3");
    return n;
  }

  // Frame::UndistortKeyPoints (src/Frame.cc:452-482): mvKeysUn from mvKeys with
  // cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK).  K = mK row-major.
  void UndistortKeyPoints(const std::vector<KeyPoint>& mvKeys, const float K[9],
                          const std::vector<float>& mDistCoef, std::vector<KeyPoint>& mvKeysUn) {
    mvKeysUn.resize(mvKeys.size());
    check(orb_undistort_keypoints(h_, (int)mvKeys.size(), mvKeys.data(), K, mDistCoef.data(),
                                  (int)mDistCoef.size(), mvKeysUn.data()),
          "UndistortKeyPoints");
  }

  // Frame::ComputeImageBounds (src/Frame.cc:484-514) -> F.mnMinX .. mnMaxY.
  void ComputeImageBounds(int cols, int rows, const float K[9],
                          const std::vector<float>& mDistCoef, FrameView& F) {
    float b[4];
    check(orb_compute_image_bounds(h_, cols, rows, K, mDistCoef.data(), (int)mDistCoef.size(), b),
          "ComputeImageBounds");
    F.mnMinX = b[0];
    F.mnMaxX = b[1];
    F.mnMinY = b[2];
    F.mnMaxY = b[3];
  }

  // A depth image as Tracking::GrabImageRGBD receives it: CV_16U or CV_32F
  // (type = ORB_DEPTH_U16 / ORB_DEPTH_F32), rows `step` bytes apart.
  struct DepthView {
    const void* data = nullptr;
    int type = ORB_DEPTH_F32;
    int cols = 0, rows = 0;
    size_t step = 0;
  };

  // Frame::ComputeStereoFromRGBD (src/Frame.cc:707-728) with GrabImageRGBD's
  // conversion (src/Tracking.cc:229-230) applied to the sampled elements:
  // mDepthMapFactor as Tracking holds it (already inverted).  A keypoint outside
  // the image gives -1 / -1 (undefined in the reference).
  void ComputeStereoFromRGBD(const std::vector<KeyPoint>& mvKeys,
                             const std::vector<KeyPoint>& mvKeysUn, const DepthView& imDepth,
                             float mDepthMapFactor, float mbf, std::vector<float>& mvuRight,
                             std::vector<float>& mvDepth) {
    assert(mvKeys.size() == mvKeysUn.size());
    mvuRight.assign(mvKeys.size(), -1.0f);
    mvDepth.assign(mvKeys.size(), -1.0f);
    check(orb_stereo_from_rgbd(h_, (int)mvKeys.size(), mvKeys.data(), mvKeysUn.data(),
                               imDepth.data, imDepth.type, imDepth.cols, imDepth.rows,
                               imDepth.step, mDepthMapFactor, mbf, mvuRight.data(),
                               mvDepth.data()),
          "ComputeStereoFromRGBD");
  }
  void stereo_from_rgbd_batch(int n_frames, const int32_t* d_n, const KeyPoint* d_keys,
                              const KeyPoint* d_keys_un, int kp_stride, const void* d_depth,
                              int depth_type, int cols, int rows, size_t row_bytes,
                              size_t image_bytes, float mDepthMapFactor, float mbf,
                              float* d_u_right, float* d_depth_out, void* stream = nullptr) {
    check(orb_stereo_from_rgbd_batch(h_, n_frames, d_n, d_keys, d_keys_un, kp_stride, d_depth,
                                     depth_type, cols, rows, row_bytes, image_bytes,
                                     mDepthMapFactor, mbf, d_u_right, d_depth_out, stream),
          "stereo_from_rgbd_batch");
  }

  // Frame::UnprojectStereo (src/Frame.cc:730-744) for every keypoint: x3D holds
  // 3 floats per keypoint (zeros where the reference returns an empty Mat,
  // valid[i] = 0).
  void UnprojectStereo(const std::vector<KeyPoint>& mvKeysUn, const std::vector<float>& mvDepth,
                       const orb_pose_t& pose, const orb_camera_t& cam, std::vector<float>& x3D,
                       std::vector<uint8_t>& valid) {
    assert(mvKeysUn.size() == mvDepth.size());
    x3D.assign(mvKeysUn.size() * 3, 0.0f);
    valid.assign(mvKeysUn.size(), 0);
    check(orb_unproject_stereo(h_, (int)mvKeysUn.size(), mvKeysUn.data(), mvDepth.data(), &pose,
                               &cam, x3D.data(), valid.data()),
          "UnprojectStereo");
  }
  void unproject_stereo_batch(int n_frames, const int32_t* d_n, const KeyPoint* d_keys_un,
                              const float* d_depth, int kp_stride, const orb_pose_t* d_poses,
                              const orb_camera_t& cam, float* d_x3d, uint8_t* d_valid,
                              void* stream = nullptr) {
    check(orb_unproject_stereo_batch(h_, n_frames, d_n, d_keys_un, d_depth, kp_stride, d_poses,
                                     &cam, d_x3d, d_valid, stream),
          "unproject_stereo_batch");
  }

  // The closest-point selection of Tracking::UpdateLastFrame / CreateNewKeyFrame
  // (src/Tracking.cc:969-1021, :1263-1318) and NeedNewKeyFrame's counts
  // (:1181-1197).  mpState[i]: 0 no MapPoint, 1 one with Observations() < 1,
  // 2 one with observations.  order = the sorted vDepthIdx's keypoint indices,
  // create = bCreateNew at each position the loop processes before its break;
  // the caller applies the side effects in that order.
  struct ClosePointsResult {
    std::vector<int32_t> order;
    std::vector<uint8_t> create;
    int nTrackedClose = 0, nNonTrackedClose = 0;
  };
  ClosePointsResult ClosePoints(const std::vector<float>& mvDepth,
                                const std::vector<uint8_t>& mpState,
                                const std::vector<uint8_t>& mvbOutlier, float mThDepth) {
    assert(mpState.size() == mvDepth.size() && mvbOutlier.size() == mvDepth.size());
    ClosePointsResult r;
    r.order.resize(mvDepth.size());
    r.create.resize(mvDepth.size());
    orb_close_counts_t c;
    check(orb_close_points(h_, (int)mvDepth.size(), mvDepth.data(), mpState.data(),
                           mvbOutlier.data(), mThDepth, r.order.data(), r.create.data(), &c),
          "ClosePoints");
    r.order.resize(c.n_sorted);
    r.create.resize(c.n_visit);
    r.nTrackedClose = c.n_tracked_close;
    r.nNonTrackedClose = c.n_non_tracked_close;
    return r;
  }
  void close_points_batch(int n_frames, const int32_t* d_n, const float* d_depth,
                          const uint8_t* d_mp_state, const uint8_t* d_outlier, int kp_stride,
                          float mThDepth, int32_t* d_order, uint8_t* d_create,
                          orb_close_counts_t* d_counts, void* stream = nullptr) {
    check(orb_close_points_batch(h_, n_frames, d_n, d_depth, d_mp_state, d_outlier, kp_stride,
                                 mThDepth, d_order, d_create, d_counts, stream),
          "close_points_batch");
  }

  // Device-batched SearchByProjection(F, vpMapPoints, th) for stereo / RGB-D
  // frames: d_u_right = mvuRight per problem at p * kp_stride
  // (orb_match_projection_local_batch_stereo).
  void search_by_projection_batch_stereo(
      int n_problems, const KeyPoint* d_keys, const uint8_t* d_desc, const float* d_u_right,
      const int32_t* d_nkeys, const uint8_t* d_locked, int kp_stride, const orb_mp_track_t* d_mps,
      const uint8_t* d_mp_desc, const int32_t* d_nmps, int mp_stride, float min_x, float max_x,
      float min_y, float max_y, const std::vector<float>& mvScaleFactors, float th,
      int32_t* d_kp_match, int32_t* d_nmatches, void* stream = nullptr) {
    check(orb_match_projection_local_batch_stereo(
              h_, n_problems, d_keys, d_desc, d_u_right, d_nkeys, d_locked, kp_stride, d_mps,
              d_mp_desc, d_nmps, mp_stride, min_x, max_x, min_y, max_y,
              (int)mvScaleFactors.size(), mvScaleFactors.data(), th, mfNNratio, d_kp_match,
              d_nmatches, stream),
          "search_by_projection_batch_stereo");
  }

  // Device-batched Optimizer::PoseOptimization (orb_pose_optimization_batch):
  // d_point_index / d_points as orb_match_projection_local_batch's d_kp_match
  // and the orb_map_point_t array (or packed float3 at stride 12).
  void pose_optimization_batch(int n_problems, const int32_t* d_nkeys, const KeyPoint* d_keys_un,
                               const float* d_u_right, int kp_stride,
                               const int32_t* d_point_index, const void* d_points,
                               int point_stride_bytes, long long pt_stride,
                               const std::vector<float>& mvInvLevelSigma2,
                               const orb_camera_t& cam, const orb_pose_t* d_pose_in,
                               orb_pose_t* d_pose_out, uint8_t* d_outlier,
                               orb_pose_opt_info_t* d_info, void* stream = nullptr) {
    check(orb_pose_optimization_batch(h_, n_problems, d_nkeys, d_keys_un, d_u_right, kp_stride,
                                      d_point_index, d_points, point_stride_bytes, pt_stride,
                                      mvInvLevelSigma2.data(), (int)mvInvLevelSigma2.size(), &cam,
                                      d_pose_in, d_pose_out, d_outlier, d_info, stream),
          "pose_optimization_batch");
  }

  // Device-batched SearchByProjection(CurrentFrame, LastFrame, th, bMono) with
  // TrackWithMotionModel's 2 * th retry below retry_below matches
  // (orb_match_projection_frame_batch; src/ORBmatcher.cc:1460-1619,
  // src/Tracking.cc:1044-1052).  d_kp_match is pose_optimization_batch's
  // d_point_index (d_points, sizeof(orb_map_point_t), mp_stride).
  void search_by_projection_frame_batch(
      int n_problems, const KeyPoint* d_keys, const uint8_t* d_desc, const float* d_u_right,
      const uint8_t* d_locked, const int32_t* d_nkeys, int kp_stride, const orb_pose_t* d_pose_cur,
      const orb_pose_t* d_pose_last, const KeyPoint* d_last_keys, const int32_t* d_last_nkeys,
      const int32_t* d_last_point_index, const uint8_t* d_last_outlier,
      const orb_map_point_t* d_points, const uint8_t* d_mp_desc, int mp_stride,
      const orb_camera_t& cam, float min_x, float max_x, float min_y, float max_y,
      const std::vector<float>& mvScaleFactors, float th, bool bMono, int retry_below,
      int32_t* d_kp_match, orb_frame_match_info_t* d_info, void* stream = nullptr) {
    check(orb_match_projection_frame_batch(
              h_, n_problems, d_keys, d_desc, d_u_right, d_locked, d_nkeys, kp_stride, d_pose_cur,
              d_pose_last, d_last_keys, d_last_nkeys, d_last_point_index, d_last_outlier, d_points,
              d_mp_desc, mp_stride, &cam, min_x, max_x, min_y, max_y, (int)mvScaleFactors.size(),
              mvScaleFactors.data(), th, bMono ? 1 : 0, mbCheckOrientation ? 1 : 0, retry_below,
              d_kp_match, d_info, stream),
          "search_by_projection_frame_batch");
  }
  static int search_by_projection_frame_batch_max_stride() {
    return orb_match_projection_frame_batch_max_stride();
  }

  // TrackWithMotionModel's "Discard outliers" loop (src/Tracking.cc:1060-1083)
  // and, with mark_seen, SearchLocalPoints' already-matched marking
  // (:1333-1354) in the problems' own map-point records
  // (orb_track_discard_outliers_batch).
  void track_discard_outliers_batch(int n_problems, const int32_t* d_nkeys, int kp_stride,
                                    int32_t* d_kp_match, uint8_t* d_outlier,
                                    orb_map_point_t* d_points, int mp_stride, bool mark_seen,
                                    const orb_frame_match_info_t* d_info,
                                    orb_track_discard_info_t* d_out, void* stream = nullptr) {
    check(orb_track_discard_outliers_batch(h_, n_problems, d_nkeys, kp_stride, d_kp_match,
                                           d_outlier, d_points, mp_stride, mark_seen ? 1 : 0,
                                           d_info, d_out, stream),
          "track_discard_outliers_batch");
  }
  // The same with the match counts read from d_n_matches[p * n_matches_stride]
  // (int32 units): the first field of either matcher's info records, stride 5
  // (orb_track_discard_outliers_batch_n; src/Tracking.cc:928-951).
  void track_discard_outliers_batch_n(int n_problems, const int32_t* d_nkeys, int kp_stride,
                                      int32_t* d_kp_match, uint8_t* d_outlier,
                                      orb_map_point_t* d_points, int mp_stride, bool mark_seen,
                                      const int32_t* d_n_matches, int n_matches_stride,
                                      orb_track_discard_info_t* d_out, void* stream = nullptr) {
    check(orb_track_discard_outliers_batch_n(h_, n_problems, d_nkeys, kp_stride, d_kp_match,
                                             d_outlier, d_points, mp_stride, mark_seen ? 1 : 0,
                                             d_n_matches, n_matches_stride, d_out, stream),
          "track_discard_outliers_batch_n");
  }

  // One side's slots of search_by_bow_batch: what ORBextractor's batch and
  // ORBVocabulary::transform_batch write with the same stride.
  struct BowSlots {
    const KeyPoint* d_keys;
    const uint8_t* d_desc;
    const int32_t* d_nkeys;
    const uint32_t* d_fv_nodes;
    const int32_t* d_fv_offs;
    const uint32_t* d_fv_feats;
    const int32_t* d_n_fv_nodes;
  };
  // Device-batched SearchByBoW(pKF, F, vpMapPointMatches) (orb_match_bow_batch;
  // src/ORBmatcher.cc:164-306 as src/Tracking.cc:904-954 and :1592-1616 call
  // it) with mfNNratio and mbCheckOrientation.  d_kf_index, d_f_index and
  // d_points may be null (identity slots / no bad point).
  void search_by_bow_batch(int n_problems, const int32_t* d_kf_index, const int32_t* d_f_index,
                           const BowSlots& kf, const int32_t* d_kf_point_index, const BowSlots& f,
                           int kp_stride, const orb_map_point_t* d_points, long long mp_stride,
                           int min_matches, int32_t* d_kp_match, orb_bow_match_info_t* d_info,
                           void* stream = nullptr) {
    check(orb_match_bow_batch(h_, n_problems, d_kf_index, d_f_index, kf.d_keys, kf.d_desc,
                              kf.d_nkeys, d_kf_point_index, kf.d_fv_nodes, kf.d_fv_offs,
                              kf.d_fv_feats, kf.d_n_fv_nodes, f.d_keys, f.d_desc, f.d_nkeys,
                              f.d_fv_nodes, f.d_fv_offs, f.d_fv_feats, f.d_n_fv_nodes, kp_stride,
                              d_points, mp_stride, mfNNratio, mbCheckOrientation ? 1 : 0,
                              min_matches, d_kp_match, d_info, stream),
          "search_by_bow_batch");
  }
  static int search_by_bow_batch_max_stride() { return orb_match_bow_batch_max_stride(); }

  // Tracking::UpdateLocalMap (src/Tracking.cc:1395-1404: UpdateLocalKeyFrames
  // :1437-1558, UpdateLocalPoints :1407-1434, SearchLocalPoints' first loop
  // :1333-1354) for n_problems frames against one device-resident map view
  // (orb_update_local_map_batch).  d_kp_match, d_local_kf and d_n_local_kf are
  // in/out; the gathered d_mps / d_mp_desc / d_nmps feed orb_frustum_batch and
  // d_locked the local matcher.
  void update_local_map_batch(int n_problems, const orb_map_view_t& view, const int32_t* d_nkeys,
                              int32_t* d_kp_match, int kp_stride, int32_t* d_local_kf,
                              int32_t* d_n_local_kf, int kf_stride, int32_t* d_local_index,
                              orb_map_point_t* d_mps, uint8_t* d_mp_desc, int32_t* d_nmps,
                              int mp_stride, uint8_t* d_locked, orb_local_map_info_t* d_info,
                              void* stream = nullptr) {
    check(orb_update_local_map_batch(h_, n_problems, &view, d_nkeys, d_kp_match, kp_stride,
                                     d_local_kf, d_n_local_kf, kf_stride, d_local_index, d_mps,
                                     d_mp_desc, d_nmps, mp_stride, d_locked, d_info, stream),
          "update_local_map_batch");
  }
  static int update_local_map_max_keyframes() { return orb_update_local_map_max_keyframes(); }
  // The local matcher's matches as global point indices in the frame's match
  // array (orb_track_local_merge_batch).
  void track_local_merge_batch(int n_problems, const int32_t* d_nkeys, int kp_stride,
                               const int32_t* d_km_local, const int32_t* d_local_index,
                               int mp_stride, int32_t* d_kp_match, void* stream = nullptr) {
    check(orb_track_local_merge_batch(h_, n_problems, d_nkeys, kp_stride, d_km_local,
                                      d_local_index, mp_stride, d_kp_match, stream),
          "track_local_merge_batch");
  }
  // mnMatchesInliers and, with null_outliers (stereo), the outliers' matches
  // reset (orb_track_local_map_finish_batch; src/Tracking.cc:1109-1135).
  void track_local_map_finish_batch(int n_problems, const int32_t* d_nkeys, int kp_stride,
                                    int32_t* d_kp_match, const uint8_t* d_outlier,
                                    const orb_map_point_t* d_points, long long pt_stride,
                                    bool only_tracking, bool null_outliers, int32_t* d_n_inliers,
                                    void* stream = nullptr) {
    check(orb_track_local_map_finish_batch(h_, n_problems, d_nkeys, kp_stride, d_kp_match,
                                           d_outlier, d_points, pt_stride, only_tracking ? 1 : 0,
                                           null_outliers ? 1 : 0, d_n_inliers, stream),
          "track_local_map_finish_batch");
  }

  // Sim3Solver's constructor with SetRansacParameters, and iterate, for
  // n_problems (pKF1, pKF2, vpMatched12) problems (orb_sim3_solver_setup_batch,
  // orb_sim3_solver_iterate_batch; src/Sim3Solver.cc).  d_kf1_slot, d_kf2_slot,
  // d_index1 and d_active may be null (identity / every problem).
  void sim3_solver_setup_batch(int n_problems, const int32_t* d_kf1_slot,
                               const int32_t* d_kf2_slot, const KeyPoint* d_kf_keys,
                               const int32_t* d_kf_nkeys, const int32_t* d_kf_point_index,
                               const orb_pose_t* d_kf_pose, int kp_stride,
                               const orb_map_point_t* d_points, const int32_t* d_match12,
                               const int32_t* d_index1, const int32_t* d_index2,
                               const std::vector<float>& levelSigma2, const orb_camera_t& cam1,
                               const orb_camera_t& cam2, bool fix_scale, double probability,
                               int min_inliers, int max_iterations, orb_sim3_state_t* d_state,
                               orb_sim3_corr_t* d_corr, void* stream = nullptr) {
    check(orb_sim3_solver_setup_batch(h_, n_problems, d_kf1_slot, d_kf2_slot, d_kf_keys,
                                      d_kf_nkeys, d_kf_point_index, d_kf_pose, kp_stride, d_points,
                                      d_match12, d_index1, d_index2, levelSigma2.data(),
                                      (int)levelSigma2.size(), &cam1, &cam2, fix_scale ? 1 : 0,
                                      probability, min_inliers, max_iterations, d_state, d_corr,
                                      stream),
          "sim3_solver_setup_batch");
  }
  void sim3_solver_iterate_batch(int n_problems, int kp_stride, orb_sim3_state_t* d_state,
                                 orb_sim3_corr_t* d_corr, const uint32_t* d_draws,
                                 int draw_stride, uint32_t rand_max, int max_iterations,
                                 int n_iterations, const uint8_t* d_active, uint8_t* d_inliers12,
                                 orb_sim3_result_t* d_result, void* stream = nullptr) {
    check(orb_sim3_solver_iterate_batch(h_, n_problems, kp_stride, d_state, d_corr, d_draws,
                                        draw_stride, rand_max, max_iterations, n_iterations,
                                        d_active, d_inliers12, d_result, stream),
          "sim3_solver_iterate_batch");
  }
  static int sim3_solver_max_stride() { return orb_sim3_solver_max_stride(); }

  // Optimizer::OptimizeSim3 for n_problems (pKF1, pKF2, vpMatches1, g2oS12)
  // problems in the solver's slot layout (orb_optimize_sim3_batch;
  // src/Optimizer.cc:1130-1326).  d_match12 is updated in place; d_start may be
  // the solver's d_result; d_kf1_slot, d_kf2_slot and d_active may be null.
  void optimize_sim3_batch(int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
                           const KeyPoint* d_kf_keys, const int32_t* d_kf_nkeys,
                           const int32_t* d_kf_point_index, const orb_pose_t* d_kf_pose,
                           int kp_stride, const orb_map_point_t* d_points, int32_t* d_match12,
                           const int32_t* d_index2, const orb_sim3_result_t* d_start,
                           const uint8_t* d_active, const std::vector<float>& invLevelSigma2,
                           const orb_camera_t& cam1, const orb_camera_t& cam2, float th2,
                           bool fix_scale, orb_sim3_opt_result_t* d_out, void* stream = nullptr) {
    check(orb_optimize_sim3_batch(h_, n_problems, d_kf1_slot, d_kf2_slot, d_kf_keys, d_kf_nkeys,
                                  d_kf_point_index, d_kf_pose, kp_stride, d_points, d_match12,
                                  d_index2, d_start, d_active, invLevelSigma2.data(),
                                  (int)invLevelSigma2.size(), &cam1, &cam2, th2, fix_scale ? 1 : 0,
                                  d_out, stream),
          "optimize_sim3_batch");
  }
  static int optimize_sim3_max_stride() { return orb_optimize_sim3_max_stride(); }

  // LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:245-537) as device
  // batches: KeyFrame::ComputeSceneMedianDepth(q) per keyframe slot
  // (orb_scene_median_depth_batch) and the neighbour loop's gate and body per
  // (current keyframe, neighbour) pair (orb_create_new_map_points_batch).
  // d_slot may be null (identity); d_kf_u_right and d_kf_depth both null:
  // monocular keyframes; d_median_depth is read only when `monocular`.
  void scene_median_depth_batch(int n_problems, const int32_t* d_slot, const int32_t* d_kf_nkeys,
                                const int32_t* d_kf_point_index, const orb_pose_t* d_kf_pose,
                                int kp_stride, const orb_map_point_t* d_points, int q,
                                float* d_median, int32_t* d_count, void* stream = nullptr) {
    check(orb_scene_median_depth_batch(h_, n_problems, d_slot, d_kf_nkeys, d_kf_point_index,
                                       d_kf_pose, kp_stride, d_points, q, d_median, d_count,
                                       stream),
          "scene_median_depth_batch");
  }
  void create_new_map_points_batch(
      int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
      const KeyPoint* d_kf_keys, const int32_t* d_kf_nkeys, int32_t* d_kf_point_index,
      const orb_pose_t* d_kf_pose, const float* d_kf_u_right, const float* d_kf_depth,
      int kp_stride, const int32_t* d_match12, const float* d_median_depth,
      const orb_camera_t& cam1, const orb_camera_t& cam2, const std::vector<float>& scaleFactors,
      const std::vector<float>& levelSigma2, bool monocular, orb_map_point_t* d_points,
      int point_capacity, int32_t* d_point_cursor, const int32_t* d_cursor_index,
      uint8_t* d_status, float* d_x3d, int32_t* d_new_pairs, orb_new_point_info_t* d_info,
      void* stream = nullptr) {
    assert(scaleFactors.size() == levelSigma2.size());
    check(orb_create_new_map_points_batch(
              h_, n_problems, d_kf1_slot, d_kf2_slot, d_kf_keys, d_kf_nkeys, d_kf_point_index,
              d_kf_pose, d_kf_u_right, d_kf_depth, kp_stride, d_match12, d_median_depth, &cam1,
              &cam2, scaleFactors.data(), levelSigma2.data(), (int)scaleFactors.size(),
              monocular ? 1 : 0, d_points, point_capacity, d_point_cursor, d_cursor_index,
              d_status, d_x3d, d_new_pairs, d_info, stream),
          "create_new_map_points_batch");
  }
  // Device-batched SearchForTriangulation (orb_search_for_triangulation_batch;
  // src/ORBmatcher.cc:718-901 as src/LocalMapping.cc:313-318 calls it) with
  // mbCheckOrientation, on the keyframe slots of search_by_bow_batch plus the
  // arrays of create_new_map_points_batch: d_match12 is the row that call
  // reads.  d_kf_u_right may be null (every keypoint monocular); cam2,
  // scaleFactors and levelSigma2 are pKF2's.
  void search_for_triangulation_batch(
      int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot, const BowSlots& kf,
      const int32_t* d_kf_point_index, const float* d_kf_u_right, const orb_pose_t* d_kf_pose,
      int kp_stride, const float* d_f12, const orb_camera_t& cam2,
      const std::vector<float>& scaleFactors, const std::vector<float>& levelSigma2,
      bool only_stereo, int32_t* d_match12, orb_tri_match_info_t* d_info,
      void* stream = nullptr) {
    assert(scaleFactors.size() == levelSigma2.size());
    check(orb_search_for_triangulation_batch(
              h_, n_problems, d_kf1_slot, d_kf2_slot, kf.d_keys, kf.d_desc, kf.d_nkeys,
              d_kf_point_index, kf.d_fv_nodes, kf.d_fv_offs, kf.d_fv_feats, kf.d_n_fv_nodes,
              d_kf_u_right, d_kf_pose, kp_stride, d_f12, &cam2, scaleFactors.data(),
              levelSigma2.data(), (int)scaleFactors.size(), only_stereo ? 1 : 0,
              mbCheckOrientation ? 1 : 0, d_match12, d_info, stream),
          "search_for_triangulation_batch");
  }
  static int search_for_triangulation_batch_max_stride() {
    return orb_search_for_triangulation_batch_max_stride();
  }
  // Device-batched SearchByBoW(pKF1, pKF2, vpMatches12) (orb_match_bow_kf_batch;
  // src/ORBmatcher.cc:581-716 as LoopClosing::ComputeSim3 calls it) with
  // mfNNratio and mbCheckOrientation, on the keyframe slots of
  // search_by_bow_batch: d_match12 / d_index2 are the rows
  // sim3_solver_setup_batch reads.  d_kf1_slot, d_kf2_slot and d_points may be
  // null (slot p / no bad point); min_matches is ComputeSim3's 20 (0: no gate).
  void search_by_bow_kf_batch(int n_problems, const int32_t* d_kf1_slot,
                              const int32_t* d_kf2_slot, const BowSlots& kf,
                              const int32_t* d_kf_point_index, int kp_stride,
                              const orb_map_point_t* d_points, int min_matches,
                              int32_t* d_match12, int32_t* d_index2, orb_bow_match_info_t* d_info,
                              void* stream = nullptr) {
    check(orb_match_bow_kf_batch(h_, n_problems, d_kf1_slot, d_kf2_slot, kf.d_keys, kf.d_desc,
                                 kf.d_nkeys, d_kf_point_index, kf.d_fv_nodes, kf.d_fv_offs,
                                 kf.d_fv_feats, kf.d_n_fv_nodes, kp_stride, d_points, mfNNratio,
                                 mbCheckOrientation ? 1 : 0, min_matches, d_match12, d_index2,
                                 d_info, stream),
          "search_by_bow_kf_batch");
  }
  static int search_by_bow_kf_batch_max_stride() { return orb_match_bow_kf_batch_max_stride(); }
  // Device-batched SearchBySim3 with ComputeSim3's inlier filter in front
  // (orb_search_by_sim3_batch; src/ORBmatcher.cc:1212-1458,
  // src/LoopClosing.cc:338-343): the solver's rows, d_inliers12 and d_result as
  // they stand, the rows updated in place for optimize_sim3_batch.
  // d_inliers12, d_active and d_new12 may be null.
  void search_by_sim3_batch(int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
                            const KeyPoint* d_kf_keys, const uint8_t* d_kf_desc,
                            const int32_t* d_kf_nkeys, const int32_t* d_kf_point_index,
                            const orb_pose_t* d_kf_pose, int kp_stride,
                            const orb_map_point_t* d_points, const uint8_t* d_mp_desc,
                            int32_t* d_match12, int32_t* d_index2, const uint8_t* d_inliers12,
                            const orb_sim3_result_t* d_sim3, const uint8_t* d_active,
                            const orb_camera_t& cam, float min_x, float max_x, float min_y,
                            float max_y, const std::vector<float>& scaleFactors,
                            float logScaleFactor, float th, int32_t* d_new12,
                            orb_sim3_search_info_t* d_info, void* stream = nullptr) {
    check(orb_search_by_sim3_batch(h_, n_problems, d_kf1_slot, d_kf2_slot, d_kf_keys, d_kf_desc,
                                   d_kf_nkeys, d_kf_point_index, d_kf_pose, kp_stride, d_points,
                                   d_mp_desc, d_match12, d_index2, d_inliers12, d_sim3, d_active,
                                   &cam, min_x, max_x, min_y, max_y, (int)scaleFactors.size(),
                                   scaleFactors.data(), logScaleFactor, th, d_new12, d_info,
                                   stream),
          "search_by_sim3_batch");
  }
  static int search_by_sim3_batch_max_stride() { return orb_search_by_sim3_batch_max_stride(); }
  static int scene_median_depth_max_stride() { return orb_scene_median_depth_max_stride(); }
  static int create_new_map_points_max_stride() {
    return orb_create_new_map_points_max_stride();
  }

  // One keyframe of LocalMapping::CreateNewMapPoints on host buffers, under the
  // reference's names.  mvpMapPoints: GetMapPointMatches() as indices into the
  // map's points (negative: NULL); a keyframe without stereo has empty mvuRight
  // and mvDepth.
  struct KeyFrameView {
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    std::vector<int32_t> mvpMapPoints;
    orb_pose_t pose;
  };
  // KeyFrame::ComputeSceneMedianDepth(q) (src/KeyFrame.cc:658-694): NaN when
  // the keyframe has no point; nDepths receives vDepths.size().
  float ComputeSceneMedianDepth(const KeyFrameView& kf, const std::vector<orb_map_point_t>& points,
                                int q = 2, int* nDepths = nullptr) {
    float median = 0.f;
    int32_t count = 0;
    check(orb_scene_median_depth(h_, (int)kf.mvpMapPoints.size(), kf.mvpMapPoints.data(),
                                 &kf.pose, points.data(), (int)points.size(), q, &median, &count),
          "ComputeSceneMedianDepth");
    if (nDepths) *nDepths = count;
    return median;
  }
  // The gate and loop body for (mpCurrentKeyFrame, pKF2) with the matches of
  // SearchForTriangulation as match12 (per keypoint of the current keyframe
  // the index in pKF2, or negative).  points.size() is the capacity; new points
  // are written from `cursor` on, which advances; both keyframes' mvpMapPoints
  // receive the new indices.  status, x3D (3 floats) and newPairs (2 ints) have
  // one entry per keypoint of the current keyframe; entries the call does not
  // write are zero.
  orb_new_point_info_t CreateNewMapPoints(
      KeyFrameView& current, KeyFrameView& kf2, const std::vector<int32_t>& match12,
      const orb_camera_t& cam1, const orb_camera_t& cam2, const std::vector<float>& scaleFactors,
      const std::vector<float>& levelSigma2, bool mbMonocular, float medianDepthKF2,
      std::vector<orb_map_point_t>& points, int& cursor, std::vector<uint8_t>& status,
      std::vector<float>& x3D, std::vector<int32_t>& newPairs) {
    const size_t n1 = current.mvKeysUn.size(), n2 = kf2.mvKeysUn.size();
    assert(match12.size() == n1 && current.mvpMapPoints.size() == n1 &&
           kf2.mvpMapPoints.size() == n2 && scaleFactors.size() == levelSigma2.size());
    const bool stereo = !current.mvuRight.empty() || !kf2.mvuRight.empty();
    std::vector<float> ur1 = current.mvuRight, dp1 = current.mvDepth, ur2 = kf2.mvuRight,
                       dp2 = kf2.mvDepth;
    if (stereo) {
      ur1.resize(n1, -1.f), dp1.resize(n1, -1.f), ur2.resize(n2, -1.f), dp2.resize(n2, -1.f);
    }
    status.assign(n1, 0);
    x3D.assign(3 * n1, 0.0f);
    newPairs.assign(2 * n1, 0);
    orb_new_point_info_t info;
    int32_t cur = cursor;
    check(orb_create_new_map_points(
              h_, (int)n1, current.mvKeysUn.data(), stereo ? ur1.data() : nullptr,
              stereo ? dp1.data() : nullptr, current.mvpMapPoints.data(), &current.pose, (int)n2,
              kf2.mvKeysUn.data(), stereo ? ur2.data() : nullptr, stereo ? dp2.data() : nullptr,
              kf2.mvpMapPoints.data(), &kf2.pose, match12.data(), medianDepthKF2, &cam1, &cam2,
              scaleFactors.data(), levelSigma2.data(), (int)scaleFactors.size(),
              mbMonocular ? 1 : 0, points.data(), (int)points.size(), &cur, status.data(),
              x3D.data(), newPairs.data(), &info),
          "CreateNewMapPoints");
    cursor = cur;
    return info;
  }

  float mfNNratio;
  bool mbCheckOrientation;
  orb_matcher_t* handle() { return h_; }

 private:
  static std::vector<float> angles(const FrameView& F) {
    std::vector<float> a(F.N());
    for (int i = 0; i < F.N(); ++i) a[i] = F.mvKeysUn[i].angle;
    return a;
  }
  orb_matcher_t* h_ = nullptr;
};

// The Frame members Optimizer::PoseOptimization reads and writes
// (src/Optimizer.cc:243-477).  mvpMapPoints[i] >= 0 names the MapPoint of
// keypoint i: its GetWorldPos() is the three floats at
// points + mvpMapPoints[i] * pointStrideBytes (12 for packed float3,
// sizeof(orb_map_point_t) for map-point records); -1 is a null pointer.
struct PoseFrame {
  const std::vector<KeyPoint>* mvKeysUn = nullptr;
  const std::vector<float>* mvuRight = nullptr;  // null: monocular
  const std::vector<int32_t>* mvpMapPoints = nullptr;
  const void* points = nullptr;
  int pointStrideBytes = 12;
  const std::vector<float>* mvInvLevelSigma2 = nullptr;
  orb_camera_t cam{};
  orb_pose_t mTcw{};                // in: the start pose; out: what SetPose receives
  std::vector<uint8_t> mvbOutlier;  // written for the keypoints that have a MapPoint
  orb_pose_opt_info_t info{};       // n_edges, lm_iterations, rejected_trials of the last call
};

// ORB_SLAM2::Sim3Solver (include/Sim3Solver.h) for one problem on the device
// batch of one.  The caller owns the device arrays (Problem) and says how a
// result reaches the host: `toHost` waits for `stream` and copies device bytes
// (hipStreamSynchronize + hipMemcpy in a HIP program; this header stays free of
// the HIP runtime).  cv::Mat results are row-major float arrays.
class Sim3Solver {
 public:
  struct Problem {  // the slot layout of orb_sim3_solver_setup_batch, one problem
    const int32_t* d_kf1_slot;  // one entry each (null: slot 0)
    const int32_t* d_kf2_slot;
    const KeyPoint* d_kf_keys;
    const int32_t* d_kf_nkeys;
    const int32_t* d_kf_point_index;
    const orb_pose_t* d_kf_pose;
    int kp_stride;
    const orb_map_point_t* d_points;
    const int32_t* d_match12;  // vpMatched12 as point indices, kp_stride entries
    const int32_t* d_index1;   // null: i1
    const int32_t* d_index2;
    const uint32_t* d_draws;   // the solver's own rand() stream, three values per iteration
    int draw_stride;
    uint32_t rand_max;
    orb_sim3_state_t* d_state;  // the solver's members between calls
    orb_sim3_corr_t* d_corr;    // kp_stride records
    uint8_t* d_inliers12;       // kp_stride bytes
    orb_sim3_result_t* d_result;
  };
  using ToHost = std::function<void(void* dst, const void* src, size_t bytes)>;

  Sim3Solver(ORBmatcher& matcher, const Problem& problem, const std::vector<float>& levelSigma2,
             const orb_camera_t& K1, const orb_camera_t& K2, bool bFixScale, ToHost toHost,
             void* stream = nullptr)
      : m_(matcher), p_(problem), sigma2_(levelSigma2), k1_(K1), k2_(K2), fix_(bFixScale),
        toHost_(std::move(toHost)), stream_(stream) {
    SetRansacParameters();
  }

  // Runs the constructor's loop again with the new parameters: mnIterations
  // and the best so far start from zero.
  void SetRansacParameters(double probability = 0.99, int minInliers = 20,
                           int maxIterations = 300) {
    maxIts_ = maxIterations;
    m_.sim3_solver_setup_batch(1, p_.d_kf1_slot, p_.d_kf2_slot, p_.d_kf_keys, p_.d_kf_nkeys,
                               p_.d_kf_point_index, p_.d_kf_pose, p_.kp_stride, p_.d_points,
                               p_.d_match12, p_.d_index1, p_.d_index2, sigma2_, k1_, k2_, fix_,
                               probability, minInliers, maxIterations, p_.d_state, p_.d_corr,
                               stream_);
  }

  // cv::Mat iterate(nIterations, bNoMore, vbInliers, nInliers): true and T12
  // (4 x 4) when a Sim3 is returned, false for the empty Mat.
  bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers,
               float T12[16]) {
    m_.sim3_solver_iterate_batch(1, p_.kp_stride, p_.d_state, p_.d_corr, p_.d_draws,
                                 p_.draw_stride, p_.rand_max, maxIts_, nIterations, nullptr,
                                 p_.d_inliers12, p_.d_result, stream_);
    toHost_(&last_, p_.d_result, sizeof(last_));
    const orb_sim3_state_t st = state();
    std::vector<uint8_t> inl((size_t)std::max(st.n1, 0));
    if (!inl.empty()) toHost_(inl.data(), p_.d_inliers12, inl.size());
    vbInliers.assign(inl.begin(), inl.end());
    bNoMore = last_.no_more != 0;
    nInliers = last_.n_inliers;
    if (last_.has_sim3) std::copy(last_.T12, last_.T12 + 16, T12);
    return last_.has_sim3 != 0;
  }

  bool find(std::vector<bool>& vbInliers12, int& nInliers, float T12[16]) {
    bool bFlag;
    return iterate(maxIts_, bFlag, vbInliers12, nInliers, T12);
  }

  void GetEstimatedRotation(float R[9]) {
    const orb_sim3_state_t st = state();
    std::copy(st.best_R, st.best_R + 9, R);
  }
  void GetEstimatedTranslation(float t[3]) {
    const orb_sim3_state_t st = state();
    std::copy(st.best_t, st.best_t + 3, t);
  }
  float GetEstimatedScale() { return state().best_scale; }

  orb_sim3_state_t state() {
    orb_sim3_state_t st;
    toHost_(&st, p_.d_state, sizeof(st));
    return st;
  }
  const orb_sim3_result_t& result() const { return last_; }

 private:
  ORBmatcher& m_;
  Problem p_;
  std::vector<float> sigma2_;
  orb_camera_t k1_, k2_;
  bool fix_;
  ToHost toHost_;
  void* stream_;
  int maxIts_ = 300;
  orb_sim3_result_t last_{};
};

// The KeyFrame members Optimizer::OptimizeSim3 reads (src/Optimizer.cc:1130-1326):
// mvKeysUn, GetMapPointMatches() as indices into the shared `points` (-1: null),
// the pose, mK and mvInvLevelSigma2.
struct Sim3KeyFrame {
  const std::vector<KeyPoint>* mvKeysUn = nullptr;
  const std::vector<int32_t>* mvpMapPoints = nullptr;  // read for pKF1 only
  orb_pose_t pose{};
  orb_camera_t mK{};
};

// g2o::Sim3 as ComputeSim3 builds it: gScm(toMatrix3d(R), toVector3d(t), s) on
// the way in, the optimised estimate (result) on the way out.
struct Sim3 {
  float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  float t[3] = {0, 0, 0};
  float s = 1.f;
  orb_sim3_opt_result_t result{};  // q, t, s as doubles and the counts of the last call
};

class Optimizer {
 public:
  // int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale):
  // vpMatches1[i] is the point index of the match of keypoint i (negative:
  // NULL) and comes back with -1 wherever the reference stores NULL; index2[i]
  // is vpMatches1[i]->GetIndexInKeyFrame(pKF2).  g2oS12 is read as R, t, s and
  // written back narrowed (with the doubles in g2oS12.result).  Both keyframes
  // share mvInvLevelSigma2.  A malformed problem leaves result.status = -1 and
  // returns 0.
  static int OptimizeSim3(ORBmatcher& matcher, const Sim3KeyFrame* pKF1, const Sim3KeyFrame* pKF2,
                          std::vector<int32_t>& vpMatches1, Sim3& g2oS12, const float th2,
                          const bool bFixScale, const std::vector<int32_t>& index2,
                          const std::vector<orb_map_point_t>& points,
                          const std::vector<float>& mvInvLevelSigma2) {
    const size_t n1 = pKF1->mvKeysUn->size();
    assert(pKF1->mvpMapPoints->size() == n1 && vpMatches1.size() == n1 && index2.size() == n1);
    orb_sim3_result_t start{};
    start.has_sim3 = 1;
    std::copy(g2oS12.R, g2oS12.R + 9, start.R);
    std::copy(g2oS12.t, g2oS12.t + 3, start.t);
    start.scale = g2oS12.s;
    check(orb_optimize_sim3(matcher.handle(), pKF1->mvKeysUn->data(), (int)n1,
                            pKF1->mvpMapPoints->data(), &pKF1->pose, pKF2->mvKeysUn->data(),
                            (int)pKF2->mvKeysUn->size(), &pKF2->pose, points.data(),
                            (int)points.size(), vpMatches1.data(), index2.data(), &start,
                            mvInvLevelSigma2.data(), (int)mvInvLevelSigma2.size(), &pKF1->mK,
                            &pKF2->mK, th2, bFixScale ? 1 : 0, &g2oS12.result),
          "OptimizeSim3");
    const orb_sim3_opt_result_t& r = g2oS12.result;
    if (r.status == 0 && r.n_corr - r.n_bad >= 10) {  // g2oS12 = vSim3_recov->estimate() (:1323)
      std::copy(r.R, r.R + 9, g2oS12.R);
      std::copy(r.t_f, r.t_f + 3, g2oS12.t);
      g2oS12.s = r.s_f;
    }
    return r.status == 0 ? r.n_inliers : 0;
  }

  // int Optimizer::PoseOptimization(Frame* pFrame): returns nInitialCorrespondences - nBad
  // (0 with fewer than 3 correspondences, pose untouched) and writes mTcw and
  // mvbOutlier.  An octave outside mvInvLevelSigma2 leaves info.n_edges = -1.
  static int PoseOptimization(ORBmatcher& matcher, PoseFrame* pFrame) {
    PoseFrame& F = *pFrame;
    const size_t n = F.mvKeysUn->size();
    assert(F.mvpMapPoints->size() == n && (!F.mvuRight || F.mvuRight->size() == n));
    F.mvbOutlier.resize(n, 0);
    orb_pose_t out{};
    check(orb_pose_optimization(
              matcher.handle(), (int)n, F.mvKeysUn->data(),
              F.mvuRight ? F.mvuRight->data() : nullptr, F.mvpMapPoints->data(), F.points,
              F.pointStrideBytes, F.mvInvLevelSigma2->data(), (int)F.mvInvLevelSigma2->size(),
              &F.cam, &F.mTcw, &out, F.mvbOutlier.data(), &F.info),
          "PoseOptimization");
    F.mTcw = out;
    return F.info.n_inliers;
  }
};

}  // namespace orb_amd
