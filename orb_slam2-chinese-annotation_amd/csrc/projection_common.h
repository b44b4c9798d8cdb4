// projection_common.h -- the per-point projection and gates of the
// projection-window ORBmatcher variants, shared by projection_kernels.hip and
// the SearchBySim3 batch (k_sim3_search_batch in sim3chain_kernels.hip).
#pragma once
#include "matcher_common.h"

enum PPMode { PP_RELOC = 0, PP_SIM3_SBP = 1, PP_FUSE = 2, PP_FUSE_SIM3 = 3, PP_SIM3_DIR = 4 };

// (PPParams, PPRec, TriParams: orb_kernel_params.h)

__device__ __forceinline__ void pp_xform(const float* R, const float* t, const float* P,
                                         float* o) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
    o[r] = ((R[3 * r] * P[0] + R[3 * r + 1] * P[1]) + R[3 * r + 2] * P[2]) + t[r];
}

__device__ __forceinline__ float pp_norm(const float* a) {
  const double ss = (((double)a[0] * a[0]) + (double)a[1] * a[1]) + (double)a[2] * a[2];
  return (float)__dsqrt_rn(ss);
}

__device__ __forceinline__ double pp_dot(const float* a, const float* b) {
  return (((double)a[0] * b[0]) + (double)a[1] * b[1]) + (double)a[2] * b[2];
}

// MapPoint::PredictScale (src/MapPoint.cc:417-450), logf pinned
__device__ __forceinline__ int pp_level(float maxDistance, float dist, const PPParams& P) {
  const float ratio = __fdiv_rn(maxDistance, dist);
  const float q = ceilf(__fdiv_rn((float)pinned_log((double)ratio), P.logScale));
  if (q < 0.f) return 0;
  if (q >= (float)P.nLevels) return P.nLevels - 1;
  return (int)q;
}

__device__ __forceinline__ bool pp_in_kf(const PPParams& P, float x, float y) {
  return x >= P.minX && x < P.maxX && y >= P.minY && y < P.maxY;  // KeyFrame::IsInImage
}

// The reference's per-point projection and gates for each mode.
template <int MODE>
__device__ __forceinline__ PPRec pp_project(const orb_map_point_t& mp, const PPParams& P) {
  PPRec r;
  r.u = r.v = r.ur = r.radius = 0.f;
  r.minL = r.maxL = 0;
  r.valid = 0;
  r.pad = 0;
  float Pc[3];
  pp_xform(P.R, P.t, mp.pos, Pc);
  if (MODE == PP_SIM3_DIR) {  // p3Dc2 = sR21 * (R1w P + t1w) + t21 (:1266-1268)
    float Pb[3];
    pp_xform(P.R2, P.t2, Pc, Pb);
    Pc[0] = Pb[0]; Pc[1] = Pb[1]; Pc[2] = Pb[2];
  }
  float u, v, invz;
  if (MODE == PP_RELOC) {  // no depth test (:1660-1664)
    invz = (float)(1.0 / (double)Pc[2]);
    u = P.fx * Pc[0] * invz + P.cx;
    v = P.fy * Pc[1] * invz + P.cy;
    if (u < P.minX || u > P.maxX || v < P.minY || v > P.maxY) return r;
  } else {
    if (Pc[2] < 0.0f) return r;
    if (MODE == PP_SIM3_SBP || MODE == PP_FUSE) invz = __fdiv_rn(1.0f, Pc[2]);
    else invz = (float)(1.0 / (double)Pc[2]);
    const float x = Pc[0] * invz, y = Pc[1] * invz;
    u = P.fx * x + P.cx;
    v = P.fy * y + P.cy;
    if (!pp_in_kf(P, u, v)) return r;
  }
  const float maxD = 1.2f * mp.max_distance, minD = 0.8f * mp.min_distance;
  float dist;
  if (MODE == PP_SIM3_DIR) {
    dist = pp_norm(Pc);  // cv::norm(p3Dc2) (:1288)
  } else {
    const float PO[3] = {mp.pos[0] - P.Ow[0], mp.pos[1] - P.Ow[1], mp.pos[2] - P.Ow[2]};
    dist = pp_norm(PO);
    if (dist < minD || dist > maxD) return r;
    if (MODE != PP_RELOC && pp_dot(PO, mp.normal) < 0.5 * (double)dist) return r;
  }
  if (MODE == PP_SIM3_DIR && (dist < minD || dist > maxD)) return r;
  const int lvl = pp_level(mp.max_distance, dist, P);
  r.u = u;
  r.v = v;
  r.ur = u - P.bf * invz;
  r.radius = P.th * P.scale[lvl];
  r.minL = lvl - 1;
  r.maxL = MODE == PP_RELOC ? lvl + 1 : lvl;  // GetFeaturesInArea levels / loop filter
  r.valid = 1;
  return r;
}
