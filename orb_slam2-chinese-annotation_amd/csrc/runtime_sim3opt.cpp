// runtime_sim3opt.cpp -- Optimizer::OptimizeSim3 as a device batch on the
// matcher handle (src/Optimizer.cc:1130-1326; sim3opt_kernels.hip).  The batch
// call has no CallOrder: the kernel keeps its state in LDS and the caller's
// arrays and uses none of the handle's scratch, so it is ordered by its stream
// alone.  The one-problem call stages its host arrays in the handle's buffers
// and is an ordinary synchronous call.
#include <vector>

#include "runtime_common.h"

namespace {

orb_status_t so_fill(Sim3OptParams& P, int n_problems, int kp_stride, const float* inv_level_sigma2,
                     int n_levels, const orb_camera_t* cam1, const orb_camera_t* cam2, float th2,
                     int fix_scale) {
  memset(&P, 0, sizeof(P));
  P.nProblems = n_problems;
  P.stride = kp_stride;
  P.nLevels = n_levels;
  for (int l = 0; l < n_levels; ++l) P.invLevelSigma2[l] = inv_level_sigma2[l];
  const float k1[4] = {cam1->fx, cam1->fy, cam1->cx, cam1->cy};
  const float k2[4] = {cam2->fx, cam2->fy, cam2->cx, cam2->cy};
  memcpy(P.k1, k1, sizeof(k1));
  memcpy(P.k2, k2, sizeof(k2));
  P.th2 = th2;
  P.fixScale = fix_scale ? 1 : 0;
  return ORB_OK;
}

}  // namespace

extern "C" {

int orb_optimize_sim3_max_stride(void) { return orb_k_sim3opt_max_stride(); }

orb_status_t orb_optimize_sim3_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
    const orb_keypoint_t* d_kf_keys, const int32_t* d_kf_nkeys, const int32_t* d_kf_point_index,
    const orb_pose_t* d_kf_pose, int kp_stride, const orb_map_point_t* d_points,
    int32_t* d_match12, const int32_t* d_index2, const orb_sim3_result_t* d_start,
    const uint8_t* d_active, const float* inv_level_sigma2, int n_levels,
    const orb_camera_t* cam1, const orb_camera_t* cam2, float th2, int fix_scale,
    orb_sim3_opt_result_t* d_out, void* stream) {
  if (!m || n_problems < 0 || kp_stride <= 0 || !inv_level_sigma2 || n_levels < 1 ||
      n_levels > ORB_MAX_LEVELS || !cam1 || !cam2)
    return ORB_EINVAL;
  if (kp_stride > orb_k_sim3opt_max_stride()) return ORB_ECAPACITY;  // nothing is launched
  if (n_problems == 0) return ORB_OK;
  if (!d_kf_keys || !d_kf_nkeys || !d_kf_point_index || !d_kf_pose || !d_points || !d_match12 ||
      !d_index2 || !d_start || !d_out)
    return ORB_EINVAL;
  std::lock_guard<std::mutex> g(m->mu);
  hipSetDevice(m->device);
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  Sim3OptParams P;
  so_fill(P, n_problems, kp_stride, inv_level_sigma2, n_levels, cam1, cam2, th2, fix_scale);
  P.kf1Slot = d_kf1_slot;
  P.kf2Slot = d_kf2_slot;
  P.keys = d_kf_keys;
  P.nkeys = d_kf_nkeys;
  P.pointIndex = d_kf_point_index;
  P.pose = d_kf_pose;
  P.points = d_points;
  P.match12 = d_match12;
  P.index2 = d_index2;
  P.start = d_start;
  P.active = d_active;
  P.out = d_out;
  HIP_TRY(orb_k_optimize_sim3(&P, s));
  return ORB_OK;
}

orb_status_t orb_optimize_sim3(
    orb_matcher_t* m, const orb_keypoint_t* keys1, int n1, const int32_t* point_index1,
    const orb_pose_t* pose1, const orb_keypoint_t* keys2, int n2, const orb_pose_t* pose2,
    const orb_map_point_t* points, int n_points, int32_t* match12, const int32_t* index2,
    const orb_sim3_result_t* start, const float* inv_level_sigma2, int n_levels,
    const orb_camera_t* cam1, const orb_camera_t* cam2, float th2, int fix_scale,
    orb_sim3_opt_result_t* out) {
  if (!m || n1 < 0 || n2 < 0 || n_points < 0 || !pose1 || !pose2 || !start || !out ||
      !inv_level_sigma2 || n_levels < 1 || n_levels > ORB_MAX_LEVELS || !cam1 || !cam2 ||
      (n1 > 0 && (!keys1 || !point_index1 || !match12 || !index2)) || (n2 > 0 && !keys2) ||
      (n_points > 0 && !points))
    return ORB_EINVAL;
  for (int i = 0; i < n1; ++i)
    if (point_index1[i] >= n_points || match12[i] >= n_points) return ORB_EINVAL;
  const int S = std::max(std::max(n1, n2), 1);
  if (S > orb_k_sim3opt_max_stride()) return ORB_ECAPACITY;
  MatcherCall call(m);
  if (call.status) return call.status;
  const hipStream_t s = call.s;
  // one staged block in (dIn), 16-byte sections: keys 2S | pose 2 | point_index S
  // | match12 S | index2 S | nkeys 2, slots 2 | start | points; the result in dOut
  auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
  const size_t oKeys = 0, oPose = up16(oKeys + 2 * (size_t)S * sizeof(orb_keypoint_t));
  const size_t oPidx = up16(oPose + 2 * sizeof(orb_pose_t)), oMatch = up16(oPidx + (size_t)S * 4);
  const size_t oIdx2 = up16(oMatch + (size_t)S * 4), oInts = up16(oIdx2 + (size_t)S * 4);
  const size_t oStart = up16(oInts + 16), oPts = up16(oStart + sizeof(orb_sim3_result_t));
  const size_t total = up16(oPts + (size_t)std::max(n_points, 1) * sizeof(orb_map_point_t));
  std::vector<uint8_t> h(total, 0);
  if (n1) memcpy(&h[oKeys], keys1, (size_t)n1 * sizeof(orb_keypoint_t));
  if (n2) memcpy(&h[oKeys + (size_t)S * sizeof(orb_keypoint_t)], keys2, (size_t)n2 * sizeof(orb_keypoint_t));
  memcpy(&h[oPose], pose1, sizeof(orb_pose_t));
  memcpy(&h[oPose + sizeof(orb_pose_t)], pose2, sizeof(orb_pose_t));
  if (n1) {
    memcpy(&h[oPidx], point_index1, (size_t)n1 * 4);
    memcpy(&h[oMatch], match12, (size_t)n1 * 4);
    memcpy(&h[oIdx2], index2, (size_t)n1 * 4);
  }
  const int32_t ints[4] = {n1, n2, 0, 1};
  memcpy(&h[oInts], ints, sizeof(ints));
  orb_sim3_result_t st0 = *start;
  st0.has_sim3 = 1;
  memcpy(&h[oStart], &st0, sizeof(st0));
  if (n_points) memcpy(&h[oPts], points, (size_t)n_points * sizeof(orb_map_point_t));
  orb_status_t st;
  if ((st = upload(m->dIn, h.data(), total, s)) || (st = m->dOut.ensure(sizeof(orb_sim3_opt_result_t))))
    return st;
  uint8_t* d = m->dIn.as<uint8_t>();
  Sim3OptParams P;
  so_fill(P, 1, S, inv_level_sigma2, n_levels, cam1, cam2, th2, fix_scale);
  P.keys = reinterpret_cast<const orb_keypoint_t*>(d + oKeys);
  P.pose = reinterpret_cast<const orb_pose_t*>(d + oPose);
  P.pointIndex = reinterpret_cast<const int32_t*>(d + oPidx);
  P.match12 = reinterpret_cast<int32_t*>(d + oMatch);
  P.index2 = reinterpret_cast<const int32_t*>(d + oIdx2);
  P.nkeys = reinterpret_cast<const int32_t*>(d + oInts);
  P.kf1Slot = P.nkeys + 2;
  P.kf2Slot = P.nkeys + 3;
  P.start = reinterpret_cast<const orb_sim3_result_t*>(d + oStart);
  P.points = reinterpret_cast<const orb_map_point_t*>(d + oPts);
  P.out = m->dOut.as<orb_sim3_opt_result_t>();
  HIP_TRY(orb_k_optimize_sim3(&P, s));
  if (n1) HIP_TRY(hipMemcpyAsync(match12, P.match12, (size_t)n1 * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(out, P.out, sizeof(orb_sim3_opt_result_t), hipMemcpyDeviceToHost, s));
  return call.finish();
}

orb_status_t orb_pinned_exp_batch(orb_matcher_t* m, int n, const double* d_x, double* d_y,
                                  void* stream) {
  if (!m || n < 0) return ORB_EINVAL;
  if (n == 0) return ORB_OK;
  if (!d_x || !d_y) return ORB_EINVAL;
  std::lock_guard<std::mutex> g(m->mu);
  hipSetDevice(m->device);
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  HIP_TRY(orb_k_pinned_exp(n, d_x, d_y, s));
  return ORB_OK;
}

}  // extern "C"
