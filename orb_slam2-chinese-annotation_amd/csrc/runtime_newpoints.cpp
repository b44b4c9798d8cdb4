// runtime_newpoints.cpp -- LocalMapping::CreateNewMapPoints on the matcher handle
// (src/LocalMapping.cc:245-537; newpoints_kernels.hip).  The batches take no
// CallOrder: the kernels keep their state in LDS and the caller's arrays and use
// none of the handle's scratch, so they are ordered by their stream alone.  The
// one-problem host-buffer forms stage through the handle's scratch (MatcherCall).
#include "runtime_common.h"

namespace {
bool np_host_values(const orb_camera_t* cam1, const orb_camera_t* cam2, const float* sf,
                    const float* sig, int n_levels) {
  if (!cam1 || !cam2 || !sf || !sig || n_levels < 2 || n_levels > ORB_MAX_LEVELS) return false;
  for (int l = 0; l < n_levels; ++l)
    if (!(sf[l] > 0.f && sf[l] <= 1e15f) || !(sig[l] > 0.f && sig[l] <= 1e15f)) return false;
  return true;
}

void np_fill(NewPointsParams& P, const orb_camera_t* cam1, const orb_camera_t* cam2,
             const float* sf, const float* sig, int n_levels, int monocular) {
  const float k1[4] = {cam1->fx, cam1->fy, cam1->cx, cam1->cy};
  const float k2[4] = {cam2->fx, cam2->fy, cam2->cx, cam2->cy};
  memcpy(P.k1, k1, sizeof(k1));
  memcpy(P.k2, k2, sizeof(k2));
  // invfx = 1.0f / fx (src/Frame.cc:115)
  P.inv1[0] = 1.0f / cam1->fx, P.inv1[1] = 1.0f / cam1->fy;
  P.inv2[0] = 1.0f / cam2->fx, P.inv2[1] = 1.0f / cam2->fy;
  P.bf1 = cam1->bf, P.mb1 = cam1->mb, P.mb2 = cam2->mb;
  P.nLevels = n_levels;
  for (int l = 0; l < n_levels; ++l) P.scaleFactors[l] = sf[l], P.sigma2[l] = sig[l];
  P.ratioFactor = 1.5f * sf[1];  // :275, mfScaleFactor = mvScaleFactors[1]
  P.monocular = monocular ? 1 : 0;
}
}  // namespace

extern "C" {

int orb_scene_median_depth_max_stride(void) { return orb_k_median_depth_max_stride(); }
int orb_create_new_map_points_max_stride(void) { return orb_k_new_points_max_stride(); }

orb_status_t orb_scene_median_depth_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_slot, const int32_t* d_kf_nkeys,
    const int32_t* d_kf_point_index, const orb_pose_t* d_kf_pose, int kp_stride,
    const orb_map_point_t* d_points, int q, float* d_median, int32_t* d_count, void* stream) {
  if (!m || n_problems < 0 || kp_stride <= 0 || q < 1) return ORB_EINVAL;
  if (kp_stride > orb_k_median_depth_max_stride()) return ORB_ECAPACITY;  // nothing is launched
  if (n_problems == 0) return ORB_OK;
  if (!d_kf_nkeys || !d_kf_point_index || !d_kf_pose || !d_points || !d_median || !d_count)
    return ORB_EINVAL;
  std::lock_guard<std::mutex> g(m->mu);
  hipSetDevice(m->device);
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  MedianDepthParams P;
  memset(&P, 0, sizeof(P));
  P.nProblems = n_problems;
  P.stride = kp_stride;
  P.q = q;
  P.slot = d_slot;
  P.nkeys = d_kf_nkeys;
  P.pointIndex = d_kf_point_index;
  P.pose = d_kf_pose;
  P.points = d_points;
  P.median = d_median;
  P.count = d_count;
  HIP_TRY(orb_k_median_depth(&P, s));
  return ORB_OK;
}

orb_status_t orb_create_new_map_points_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
    const orb_keypoint_t* d_kf_keys, const int32_t* d_kf_nkeys, int32_t* d_kf_point_index,
    const orb_pose_t* d_kf_pose, const float* d_kf_u_right, const float* d_kf_depth,
    int kp_stride, const int32_t* d_match12, const float* d_median_depth,
    const orb_camera_t* cam1, const orb_camera_t* cam2, const float* scale_factors,
    const float* level_sigma2, int n_levels, int monocular, orb_map_point_t* d_points,
    int point_capacity, int32_t* d_point_cursor, const int32_t* d_cursor_index,
    uint8_t* d_status, float* d_x3d, int32_t* d_new_pairs, orb_new_point_info_t* d_info,
    void* stream) {
  if (!m || n_problems < 0 || kp_stride <= 0 || point_capacity < 0 ||
      !np_host_values(cam1, cam2, scale_factors, level_sigma2, n_levels) ||
      (d_kf_u_right == nullptr) != (d_kf_depth == nullptr))
    return ORB_EINVAL;
  if (kp_stride > orb_k_new_points_max_stride()) return ORB_ECAPACITY;  // nothing is launched
  if (n_problems == 0) return ORB_OK;
  if (!d_kf1_slot || !d_kf2_slot || !d_kf_keys || !d_kf_nkeys || !d_kf_point_index ||
      !d_kf_pose || !d_match12 || (monocular && !d_median_depth) || !d_points ||
      !d_point_cursor || !d_cursor_index || !d_status || !d_x3d || !d_new_pairs || !d_info)
    return ORB_EINVAL;
  std::lock_guard<std::mutex> g(m->mu);
  hipSetDevice(m->device);
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  NewPointsParams P;
  memset(&P, 0, sizeof(P));
  P.nProblems = n_problems;
  P.stride = kp_stride;
  P.kf1Slot = d_kf1_slot;
  P.kf2Slot = d_kf2_slot;
  P.keys = d_kf_keys;
  P.nkeys = d_kf_nkeys;
  P.pointIndex = d_kf_point_index;
  P.pose = d_kf_pose;
  P.uRight = d_kf_u_right;
  P.depth = d_kf_depth;
  P.match12 = d_match12;
  P.medianDepth = d_median_depth;
  P.points = d_points;
  P.pointCapacity = point_capacity;
  P.pointCursor = d_point_cursor;
  P.cursorIndex = d_cursor_index;
  np_fill(P, cam1, cam2, scale_factors, level_sigma2, n_levels, monocular);
  P.status = d_status;
  P.x3d = d_x3d;
  P.newPairs = d_new_pairs;
  P.info = d_info;
  HIP_TRY(orb_k_new_points(&P, s));
  return ORB_OK;
}

// SearchForTriangulation for the same pairs on the same slot arrays
// (src/ORBmatcher.cc:718-901; k_tri_batch in track_kernels.hip): its d_match12
// row is what orb_create_new_map_points_batch reads.
int orb_search_for_triangulation_batch_max_stride(void) { return orb_k_tri_batch_max_stride(); }

orb_status_t orb_search_for_triangulation_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
    const orb_keypoint_t* d_kf_keys, const uint8_t* d_kf_desc, const int32_t* d_kf_nkeys,
    const int32_t* d_kf_point_index, const uint32_t* d_kf_fv_nodes, const int32_t* d_kf_fv_offs,
    const uint32_t* d_kf_fv_feats, const int32_t* d_kf_n_fv_nodes, const float* d_kf_u_right,
    const orb_pose_t* d_kf_pose, int kp_stride, const float* d_f12, const orb_camera_t* cam2,
    const float* scale_factors, const float* level_sigma2, int n_levels, int only_stereo,
    int check_orientation, int32_t* d_match12, orb_tri_match_info_t* d_info, void* stream) {
  if (!m || n_problems < 0 || kp_stride <= 0 || !cam2 || !scale_factors || !level_sigma2 ||
      n_levels < 1 || n_levels > ORB_MAX_LEVELS)
    return ORB_EINVAL;
  for (int l = 0; l < n_levels; ++l)
    if (!(scale_factors[l] > 0.f && scale_factors[l] <= 1e15f) ||
        !(level_sigma2[l] > 0.f && level_sigma2[l] <= 1e15f))
      return ORB_EINVAL;
  if (kp_stride > orb_k_tri_batch_max_stride()) return ORB_ECAPACITY;  // nothing is launched
  if (n_problems == 0) return ORB_OK;
  if (!d_kf1_slot || !d_kf2_slot || !d_kf_keys || !d_kf_desc || !d_kf_nkeys ||
      !d_kf_point_index || !d_kf_fv_nodes || !d_kf_fv_offs || !d_kf_fv_feats ||
      !d_kf_n_fv_nodes || !d_kf_pose || !d_f12 || !d_match12 || !d_info)
    return ORB_EINVAL;
  std::lock_guard<std::mutex> g(m->mu);
  hipSetDevice(m->device);
  hipStream_t s = stream ? (hipStream_t)stream : m->stream;
  TriBatchParams P;
  memset(&P, 0, sizeof(P));
  P.nProblems = n_problems;
  P.stride = kp_stride;
  P.kf1Slot = d_kf1_slot;
  P.kf2Slot = d_kf2_slot;
  P.kf = BowSlots{d_kf_keys, d_kf_desc, d_kf_nkeys, d_kf_fv_nodes, d_kf_fv_offs, d_kf_fv_feats,
                  d_kf_n_fv_nodes};
  P.pointIndex = d_kf_point_index;
  P.uRight = d_kf_u_right;
  P.pose = d_kf_pose;
  P.f12 = d_f12;
  P.fx = cam2->fx, P.fy = cam2->fy, P.cx = cam2->cx, P.cy = cam2->cy;
  P.nLevels = n_levels;
  P.onlyStereo = only_stereo ? 1 : 0;
  P.checkOri = check_orientation ? 1 : 0;
  for (int l = 0; l < n_levels; ++l) P.scale[l] = scale_factors[l], P.sigma2[l] = level_sigma2[l];
  HIP_TRY(orb_k_tri_batch(&P, d_match12, d_info, s));
  return ORB_OK;
}

orb_status_t orb_scene_median_depth(orb_matcher_t* m, int n, const int32_t* point_index,
                                    const orb_pose_t* pose, const orb_map_point_t* points,
                                    int n_points, int q, float* median, int32_t* count) {
  if (!m || n < 0 || n_points < 0 || q < 1 || !pose || !median || !count ||
      (n > 0 && !point_index) || (n_points > 0 && !points))
    return ORB_EINVAL;
  for (int i = 0; i < n; ++i)
    if (point_index[i] >= n_points) return ORB_EINVAL;
  const int S = std::max(n, 1);
  if (S > orb_k_median_depth_max_stride()) return ORB_ECAPACITY;
  MatcherCall call(m);
  if (call.status) return call.status;
  const hipStream_t s = call.s;
  orb_status_t st;
  const int32_t nk = n;
  // dOut: median (4), count (4)
  if ((st = upload(m->dA, point_index, (size_t)n * 4, s)) || (st = upload(m->dB, &nk, 4, s)) ||
      (st = upload(m->dPose, pose, sizeof(orb_pose_t), s)) ||
      (st = upload(m->dMapPts, points, (size_t)n_points * sizeof(orb_map_point_t), s)) ||
      (st = m->dOut.ensure(16)))
    return st;
  MedianDepthParams P;
  memset(&P, 0, sizeof(P));
  P.nProblems = 1;
  P.stride = S;
  P.q = q;
  P.nkeys = m->dB.as<int32_t>();
  P.pointIndex = m->dA.as<int32_t>();
  P.pose = m->dPose.as<orb_pose_t>();
  P.points = m->dMapPts.as<orb_map_point_t>();
  P.median = m->dOut.as<float>();
  P.count = m->dOut.as<int32_t>() + 1;
  HIP_TRY(orb_k_median_depth(&P, s));
  HIP_TRY(hipMemcpyAsync(median, P.median, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(count, P.count, 4, hipMemcpyDeviceToHost, s));
  return call.finish();
}

orb_status_t orb_create_new_map_points(
    orb_matcher_t* m, int n1, const orb_keypoint_t* keys1, const float* u_right1,
    const float* depth1, int32_t* point_index1, const orb_pose_t* pose1, int n2,
    const orb_keypoint_t* keys2, const float* u_right2, const float* depth2,
    int32_t* point_index2, const orb_pose_t* pose2, const int32_t* match12, float median_depth,
    const orb_camera_t* cam1, const orb_camera_t* cam2, const float* scale_factors,
    const float* level_sigma2, int n_levels, int monocular, orb_map_point_t* points,
    int point_capacity, int32_t* cursor, uint8_t* status, float* x3d, int32_t* new_pairs,
    orb_new_point_info_t* info) {
  const bool stereo = u_right1 || depth1 || u_right2 || depth2;
  if (!m || n1 < 0 || n2 < 0 || point_capacity < 0 || !pose1 || !pose2 || !cursor || !info ||
      !np_host_values(cam1, cam2, scale_factors, level_sigma2, n_levels) ||
      (n1 > 0 && (!keys1 || !point_index1 || !match12 || !status || !x3d || !new_pairs)) ||
      (n2 > 0 && (!keys2 || !point_index2)) || (point_capacity > 0 && !points) ||
      (stereo && ((n1 > 0 && (!u_right1 || !depth1)) || (n2 > 0 && (!u_right2 || !depth2)))))
    return ORB_EINVAL;
  const int S = std::max(std::max(n1, n2), 1);
  if (S > orb_k_new_points_max_stride()) return ORB_ECAPACITY;
  MatcherCall call(m);
  if (call.status) return call.status;
  const hipStream_t s = call.s;
  // one staged block in, one out.  In (dIn): keys 2S | pose 2 | u_right 2S |
  // depth 2S | match12 S | point_index 2S | nkeys 2 | slots 2 | cursor 1 |
  // cursor index 1 | median 1.  Out (dOut): points | status S | x3d 3S | pairs 2S | info
  const size_t oKeys = 0, oPose = oKeys + 2 * (size_t)S * sizeof(orb_keypoint_t),
               oUr = oPose + 2 * sizeof(orb_pose_t), oDepth = oUr + 8 * (size_t)S,
               oM12 = oDepth + 8 * (size_t)S, oPidx = oM12 + 4 * (size_t)S,
               oMisc = oPidx + 8 * (size_t)S, inBytes = oMisc + 32;
  std::vector<uint8_t>& h = m->hostScratch;
  h.assign(inBytes, 0);
  if (n1) memcpy(&h[oKeys], keys1, (size_t)n1 * sizeof(orb_keypoint_t));
  if (n2) memcpy(&h[oKeys + (size_t)S * sizeof(orb_keypoint_t)], keys2,
                 (size_t)n2 * sizeof(orb_keypoint_t));
  memcpy(&h[oPose], pose1, sizeof(orb_pose_t));
  memcpy(&h[oPose + sizeof(orb_pose_t)], pose2, sizeof(orb_pose_t));
  if (stereo) {
    if (n1) memcpy(&h[oUr], u_right1, 4 * (size_t)n1), memcpy(&h[oDepth], depth1, 4 * (size_t)n1);
    if (n2)
      memcpy(&h[oUr + 4 * (size_t)S], u_right2, 4 * (size_t)n2),
          memcpy(&h[oDepth + 4 * (size_t)S], depth2, 4 * (size_t)n2);
  }
  if (n1) memcpy(&h[oM12], match12, 4 * (size_t)n1), memcpy(&h[oPidx], point_index1, 4 * (size_t)n1);
  if (n2) memcpy(&h[oPidx + 4 * (size_t)S], point_index2, 4 * (size_t)n2);
  const int32_t misc[6] = {n1, n2, 0, 1, *cursor, 0};
  memcpy(&h[oMisc], misc, sizeof(misc));
  memcpy(&h[oMisc + 24], &median_depth, 4);
  const size_t oPts = 0, oStatus = oPts + (((size_t)point_capacity * sizeof(orb_map_point_t) + 15) & ~(size_t)15),
               oX3d = oStatus + (((size_t)S + 15) & ~(size_t)15), oPairs = oX3d + 12 * (size_t)S,
               oInfo = oPairs + 8 * (size_t)S, outBytes = oInfo + sizeof(orb_new_point_info_t);
  orb_status_t st;
  if ((st = upload(m->dIn, h.data(), inBytes, s)) || (st = m->dOut.ensure(outBytes))) return st;
  uint8_t* in = m->dIn.as<uint8_t>();
  uint8_t* out = m->dOut.as<uint8_t>();
  // the caller's values stand where the device writes nothing
  if (n1) {
    HIP_TRY(hipMemcpyAsync(out + oStatus, status, (size_t)n1, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(out + oX3d, x3d, 12 * (size_t)n1, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(out + oPairs, new_pairs, 8 * (size_t)n1, hipMemcpyHostToDevice, s));
  }
  NewPointsParams P;
  memset(&P, 0, sizeof(P));
  P.nProblems = 1;
  P.stride = S;
  P.keys = (const orb_keypoint_t*)(in + oKeys);
  P.pose = (const orb_pose_t*)(in + oPose);
  P.uRight = stereo ? (const float*)(in + oUr) : nullptr;
  P.depth = stereo ? (const float*)(in + oDepth) : nullptr;
  P.match12 = (const int32_t*)(in + oM12);
  P.pointIndex = (int32_t*)(in + oPidx);
  P.nkeys = (const int32_t*)(in + oMisc);
  P.kf1Slot = (const int32_t*)(in + oMisc + 8);
  P.kf2Slot = (const int32_t*)(in + oMisc + 12);
  P.pointCursor = (int32_t*)(in + oMisc + 16);
  P.cursorIndex = (const int32_t*)(in + oMisc + 20);
  P.medianDepth = (const float*)(in + oMisc + 24);
  P.points = (orb_map_point_t*)(out + oPts);
  P.pointCapacity = point_capacity;
  np_fill(P, cam1, cam2, scale_factors, level_sigma2, n_levels, monocular);
  P.status = out + oStatus;
  P.x3d = (float*)(out + oX3d);
  P.newPairs = (int32_t*)(out + oPairs);
  P.info = (orb_new_point_info_t*)(out + oInfo);
  HIP_TRY(orb_k_new_points(&P, s));
  HIP_TRY(hipMemcpyAsync(info, out + oInfo, sizeof(*info), hipMemcpyDeviceToHost, s));
  if (n1) {
    HIP_TRY(hipMemcpyAsync(status, out + oStatus, (size_t)n1, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(x3d, out + oX3d, 12 * (size_t)n1, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(new_pairs, out + oPairs, 8 * (size_t)n1, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(point_index1, in + oPidx, 4 * (size_t)n1, hipMemcpyDeviceToHost, s));
  }
  if (n2)
    HIP_TRY(hipMemcpyAsync(point_index2, in + oPidx + 4 * (size_t)S, 4 * (size_t)n2,
                           hipMemcpyDeviceToHost, s));
  HIP_TRY(stream_wait(s));
  if (!info->overflow && !info->gated && info->n_new > 0) {
    HIP_TRY(hipMemcpyAsync(points + info->first_point,
                           out + oPts + (size_t)info->first_point * sizeof(orb_map_point_t),
                           (size_t)info->n_new * sizeof(orb_map_point_t), hipMemcpyDeviceToHost,
                           s));
    *cursor = info->first_point + info->n_new;
  }
  return call.finish();
}

}  // extern "C"
