// runtime_sim3chain.cpp -- the two matcher stages of LoopClosing::ComputeSim3 on
// the matcher handle as device batches (src/LoopClosing.cc:251-428;
// sim3chain_kernels.hip): SearchByBoW(pKF1, pKF2, vpMatches12) and SearchBySim3
// on the Sim3Solver's keyframe slots.  No CallOrder: the kernels keep their
// state in LDS and the caller's arrays and use none of the handle's scratch, so
// they are ordered by their stream alone.
#include "runtime_common.h"

extern "C" {

int orb_match_bow_kf_batch_max_stride(void) { return orb_k_bow_kf_batch_max_stride(); }
int orb_search_by_sim3_batch_max_stride(void) { return orb_k_sim3_search_max_stride(); }

orb_status_t orb_match_bow_kf_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
    const orb_keypoint_t* d_kf_keys, const uint8_t* d_kf_desc, const int32_t* d_kf_nkeys,
    const int32_t* d_kf_point_index, const uint32_t* d_kf_fv_nodes, const int32_t* d_kf_fv_offs,
    const uint32_t* d_kf_fv_feats, const int32_t* d_kf_n_fv_nodes, int kp_stride,
    const orb_map_point_t* d_points, float nnratio, int check_orientation, int min_matches,
    int32_t* d_match12, int32_t* d_index2, orb_bow_match_info_t* d_info, void* stream) {
  if (!m || n_problems < 0 || kp_stride <= 0 || !std::isfinite(nnratio)) return ORB_EINVAL;
  if (kp_stride > orb_k_bow_kf_batch_max_stride()) return ORB_ECAPACITY;  // nothing is launched
  if (n_problems == 0) return ORB_OK;
  if (!d_kf_keys || !d_kf_desc || !d_kf_nkeys || !d_kf_point_index || !d_kf_fv_nodes ||
      !d_kf_fv_offs || !d_kf_fv_feats || !d_kf_n_fv_nodes || !d_match12 || !d_index2 || !d_info)
    return ORB_EINVAL;
  std::lock_guard<std::mutex> g(m->mu);
  hipSetDevice(m->device);
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  BowKfBatchParams P;
  memset(&P, 0, sizeof(P));
  P.nProblems = n_problems;
  P.stride = kp_stride;
  P.kf1Slot = d_kf1_slot;
  P.kf2Slot = d_kf2_slot;
  P.kf = BowSlots{d_kf_keys, d_kf_desc, d_kf_nkeys, d_kf_fv_nodes, d_kf_fv_offs, d_kf_fv_feats,
                  d_kf_n_fv_nodes};
  P.pointIndex = d_kf_point_index;
  P.points = d_points;
  P.nnratio = nnratio;
  P.checkOri = check_orientation ? 1 : 0;
  P.minMatches = min_matches;
  HIP_TRY(orb_k_bow_kf_batch(&P, d_match12, d_index2, d_info, s));
  return ORB_OK;
}

orb_status_t orb_search_by_sim3_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
    const orb_keypoint_t* d_kf_keys, const uint8_t* d_kf_desc, const int32_t* d_kf_nkeys,
    const int32_t* d_kf_point_index, const orb_pose_t* d_kf_pose, int kp_stride,
    const orb_map_point_t* d_points, const uint8_t* d_mp_desc, int32_t* d_match12,
    int32_t* d_index2, const uint8_t* d_inliers12, const orb_sim3_result_t* d_sim3,
    const uint8_t* d_active, const orb_camera_t* cam, float min_x, float max_x, float min_y,
    float max_y, int n_levels, const float* scale_factors, float log_scale_factor, float th,
    int32_t* d_new12, orb_sim3_search_info_t* d_info, void* stream) {
  if (!m || n_problems < 0 || kp_stride <= 0 || !cam || !scale_factors || n_levels < 1 ||
      n_levels > ORB_MAX_LEVELS || !(max_x > min_x) || !(max_y > min_y))
    return ORB_EINVAL;
  if (kp_stride > orb_k_sim3_search_max_stride()) return ORB_ECAPACITY;  // nothing is launched
  if (n_problems == 0) return ORB_OK;
  if (!d_kf_keys || !d_kf_desc || !d_kf_nkeys || !d_kf_point_index || !d_kf_pose || !d_points ||
      !d_mp_desc || !d_match12 || !d_index2 || !d_sim3 || !d_info)
    return ORB_EINVAL;
  std::lock_guard<std::mutex> g(m->mu);
  hipSetDevice(m->device);
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  Sim3SearchParams P;
  memset(&P, 0, sizeof(P));
  P.nProblems = n_problems;
  P.stride = kp_stride;
  P.kf1Slot = d_kf1_slot;
  P.kf2Slot = d_kf2_slot;
  P.keys = d_kf_keys;
  P.desc = d_kf_desc;
  P.nkeys = d_kf_nkeys;
  P.pointIndex = d_kf_point_index;
  P.pose = d_kf_pose;
  P.points = d_points;
  P.mpDesc = d_mp_desc;
  P.match12 = d_match12;
  P.index2 = d_index2;
  P.inliers12 = d_inliers12;
  P.sim3 = d_sim3;
  P.active = d_active;
  // as pp_base (runtime.cpp) fills them for orb_search_by_sim3
  PPParams& B = P.base;
  B.fx = cam->fx; B.fy = cam->fy; B.cx = cam->cx; B.cy = cam->cy; B.bf = cam->bf;
  B.minX = min_x; B.maxX = max_x; B.minY = min_y; B.maxY = max_y;
  B.invW = (float)ORB_GRID_COLS / (max_x - min_x);
  B.invH = (float)ORB_GRID_ROWS / (max_y - min_y);
  B.th = th;
  B.logScale = log_scale_factor;
  B.nLevels = n_levels;
  B.thr = 100;
  for (int l = 0; l < n_levels; ++l) B.scale[l] = scale_factors[l];
  P.new12 = d_new12;
  P.info = d_info;
  HIP_TRY(orb_k_sim3_search(&P, s));
  return ORB_OK;
}

}  // extern "C"
