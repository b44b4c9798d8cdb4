// runtime_sim3.cpp -- Sim3Solver as two device batches on the matcher handle
// (src/Sim3Solver.cc; sim3_kernels.hip).  No CallOrder: the kernels keep their
// state in LDS and the caller's arrays and use none of the handle's scratch, so
// both calls are ordered by their stream alone.
#include "runtime_common.h"

extern "C" {

int orb_sim3_solver_max_stride(void) { return orb_k_sim3_max_stride(); }

orb_status_t orb_sim3_solver_setup_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
    const orb_keypoint_t* d_kf_keys, const int32_t* d_kf_nkeys, const int32_t* d_kf_point_index,
    const orb_pose_t* d_kf_pose, int kp_stride, const orb_map_point_t* d_points,
    const int32_t* d_match12, const int32_t* d_index1, const int32_t* d_index2,
    const float* level_sigma2, int n_levels, const orb_camera_t* cam1, const orb_camera_t* cam2,
    int fix_scale, double probability, int min_inliers, int max_iterations,
    orb_sim3_state_t* d_state, orb_sim3_corr_t* d_corr, void* stream) {
  if (!m || n_problems < 0 || kp_stride <= 0 || !level_sigma2 || n_levels < 1 ||
      n_levels > ORB_MAX_LEVELS || !cam1 || !cam2 || !(probability > 0.0 && probability < 1.0) ||
      min_inliers < 3 || max_iterations < 1)
    return ORB_EINVAL;
  for (int l = 0; l < n_levels; ++l)
    if (!(level_sigma2[l] >= 0.f && level_sigma2[l] <= 1e15f)) return ORB_EINVAL;
  if (kp_stride > orb_k_sim3_max_stride()) return ORB_ECAPACITY;  // nothing is launched
  if (n_problems == 0) return ORB_OK;
  if (!d_kf_keys || !d_kf_nkeys || !d_kf_point_index || !d_kf_pose || !d_points || !d_match12 ||
      !d_index2 || !d_state || !d_corr)
    return ORB_EINVAL;
  std::lock_guard<std::mutex> g(m->mu);
  hipSetDevice(m->device);
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  Sim3SetupParams P;
  memset(&P, 0, sizeof(P));
  P.nProblems = n_problems;
  P.stride = kp_stride;
  P.kf1Slot = d_kf1_slot;
  P.kf2Slot = d_kf2_slot;
  P.keys = d_kf_keys;
  P.nkeys = d_kf_nkeys;
  P.pointIndex = d_kf_point_index;
  P.pose = d_kf_pose;
  P.points = d_points;
  P.match12 = d_match12;
  P.index1 = d_index1;
  P.index2 = d_index2;
  P.nLevels = n_levels;
  // mvnMaxError (include/Sim3Solver.h:78-79): the double product truncated into
  // a size_t, which err < maxError converts to float (pin P16)
  for (int l = 0; l < n_levels; ++l)
    P.maxErr[l] = (float)(uint64_t)(9.210 * (double)level_sigma2[l]);
  const float k1[4] = {cam1->fx, cam1->fy, cam1->cx, cam1->cy};
  const float k2[4] = {cam2->fx, cam2->fy, cam2->cx, cam2->cy};
  memcpy(P.k1, k1, sizeof(k1));
  memcpy(P.k2, k2, sizeof(k2));
  P.fixScale = fix_scale ? 1 : 0;
  P.minInliers = min_inliers;
  P.maxIterations = max_iterations;
  P.probability = probability;
  P.state = d_state;
  P.corr = d_corr;
  HIP_TRY(orb_k_sim3_setup(&P, s));
  return ORB_OK;
}

orb_status_t orb_sim3_solver_iterate_batch(
    orb_matcher_t* m, int n_problems, int kp_stride, orb_sim3_state_t* d_state,
    orb_sim3_corr_t* d_corr, const uint32_t* d_draws, int draw_stride, uint32_t rand_max,
    int max_iterations, int n_iterations, const uint8_t* d_active, uint8_t* d_inliers12,
    orb_sim3_result_t* d_result, void* stream) {
  if (!m || n_problems < 0 || kp_stride <= 0 || max_iterations < 1 || n_iterations < 0 ||
      (long long)draw_stride < 3LL * max_iterations)
    return ORB_EINVAL;
  if (kp_stride > orb_k_sim3_max_stride()) return ORB_ECAPACITY;  // nothing is launched
  if (n_problems == 0) return ORB_OK;
  if (!d_state || !d_corr || !d_draws || !d_inliers12 || !d_result) return ORB_EINVAL;
  std::lock_guard<std::mutex> g(m->mu);
  hipSetDevice(m->device);
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  Sim3IterParams P;
  memset(&P, 0, sizeof(P));
  P.nProblems = n_problems;
  P.stride = kp_stride;
  P.state = d_state;
  P.corr = d_corr;
  P.draws = d_draws;
  P.drawStride = draw_stride;
  P.randMax = rand_max;
  P.maxIterations = max_iterations;
  P.nIterations = n_iterations;
  P.active = d_active;
  P.inliers12 = d_inliers12;
  P.result = d_result;
  HIP_TRY(orb_k_sim3_iterate(&P, s));
  return ORB_OK;
}

}  // extern "C"
