// newpoints_kernels.hip -- LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:
// 245-537) as device batches: KeyFrame::ComputeSceneMedianDepth (src/KeyFrame.cc:
// 658-694), the neighbour loop's gate (:289-311) and body (:338-535), and the
// new point's MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:349-402).
//
// k_median_depth: one workgroup per keyframe slot.  The depths of the slot's
//   points go to LDS as order-preserving integer keys (an LDS counter hands out
//   the positions: the k-th order statistic does not depend on the order), then
//   every thread rank-counts its keys; the key with less <= k < less + equal is
//   the answer.
// k_new_points: one workgroup per (KF1, KF2) pair, one lane per KF1 keypoint
//   slot in rounds of NP_T.
//   pass 1   each lane runs the reference's tests on its match; the 4 x 4
//            Jacobi SVD state (16 floats of At, 16 of Vt, 4 doubles of W) lives
//            in registers: the six (i, j) pairs are unrolled over rows held as
//            separate arrays, nothing is indexed at run time.  Status, x3D and
//            the lane's ordinal among the accepted (a workgroup prefix sum of
//            the accept flags, carried across rounds) wait in LDS.
//   commit   one lane reads the cursor; on overflow only info is written.
//   pass 2   statuses, x3D, the point records in ascending i1, the pairs and
//            the two point_index rows are written; one lane advances the cursor.
// The pin list is in include/orb_abi.h (N1..N10).
#include "orb_device.h"
#include "orb_kernels.h"

#ifndef NP_T
#define NP_T 256  // threads per workgroup, both kernels (README: compile-time macros)
#endif
static_assert(NP_T % 64 == 0 && NP_T >= 64 && NP_T <= 1024, "whole waves");
static_assert(sizeof(orb_map_point_t) == 36 && sizeof(orb_new_point_info_t) == 64, "ABI records");

#define NP_FIXED_LDS ((size_t)1024)  // the kernels' static LDS, counted by the capacity rules

// ------------------------------------------------------------------- pins
// N1: Mat::dot of two 3-vectors, exact double products summed from 0
__device__ __forceinline__ double np_dot3(float a0, float a1, float a2, float b0, float b1,
                                          float b2) {
  return ((0.0 + (double)a0 * (double)b0) + (double)a1 * (double)b1) + (double)a2 * (double)b2;
}
// N1: row.dot(x) + t, narrowed once
__device__ __forceinline__ float np_row(const float* r, float t, float x, float y, float z) {
  return (float)(np_dot3(r[0], r[1], r[2], x, y, z) + (double)t);
}
// N3: cv::norm of a 3-vector, as the double it returns
__device__ __forceinline__ double np_norm3(float x, float y, float z) {
  return __builtin_sqrt(np_dot3(x, y, z, x, y, z));
}
// N4: cos(2 * atan2(mb / 2, depth)) on floats
__device__ __forceinline__ float np_cos_stereo(float mb, float depth) {
  const float a = (float)pinned_atan2((double)(mb / 2.0f), (double)depth);
  double sn, cs;
  pinned_sincos_d((double)(2.0f * a), &sn, &cs);
  return (float)cs;
}

// N6: one (i, j) pair of a sweep; true when the rows were rotated
__device__ __forceinline__ bool np_svd_pair(float (&ai)[4], float (&aj)[4], float (&vi)[4],
                                            float (&vj)[4], double& wi, double& wj) {
  const double a = wi, b = wj;
  double p = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) p += (double)ai[k] * (double)aj[k];
  const double eps = (double)(2.0f * 1.1920928955078125e-07f);
  if (__builtin_fabs(p) <= eps * __builtin_sqrt(a * b)) return false;
  p *= 2.0;
  const double beta = a - b, gamma = __builtin_sqrt(p * p + beta * beta);
  float c, s;
  if (beta < 0) {
    const double delta = (gamma - beta) * 0.5;
    s = (float)__builtin_sqrt(delta / gamma);
    c = (float)(p / ((gamma * (double)s) * 2.0));
  } else {
    c = (float)__builtin_sqrt((gamma + beta) / (gamma * 2.0));
    s = (float)(p / ((gamma * (double)c) * 2.0));
  }
  const float ms = -s;
  double na = 0.0, nb = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float t0 = c * ai[k] + s * aj[k];
    const float t1 = ms * ai[k] + c * aj[k];
    ai[k] = t0;
    aj[k] = t1;
    na += (double)t0 * (double)t0;
    nb += (double)t1 * (double)t1;
  }
  wi = na;
  wj = nb;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float t0 = c * vi[k] + s * vj[k];
    const float t1 = ms * vi[k] + c * vj[k];
    vi[k] = t0;
    vj[k] = t1;
  }
  return true;
}

__device__ __forceinline__ void np_swap_rows(bool take, float (&vi)[4], float (&vj)[4],
                                             double& wi, double& wj) {
  if (take) {
    const double w = wi;
    wi = wj;
    wj = w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float t = vi[k];
      vi[k] = vj[k];
      vj[k] = t;
    }
  }
}

__device__ __forceinline__ double np_sumsq(const float (&a)[4]) {
  double sd = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) sd += (double)a[k] * (double)a[k];
  return sd;
}

// N6: vt.row(3) of cv::SVD::compute on the 4 x 4 float A whose columns are a0..a3
__device__ __forceinline__ void np_svd_vt3(float (&a0)[4], float (&a1)[4], float (&a2)[4],
                                           float (&a3)[4], float (&out)[4]) {
  float v0[4] = {1.f, 0.f, 0.f, 0.f}, v1[4] = {0.f, 1.f, 0.f, 0.f}, v2[4] = {0.f, 0.f, 1.f, 0.f},
        v3[4] = {0.f, 0.f, 0.f, 1.f};
  double w0 = np_sumsq(a0), w1 = np_sumsq(a1), w2 = np_sumsq(a2), w3 = np_sumsq(a3);
#pragma nounroll
  for (int iter = 0; iter < 30; ++iter) {
    bool changed = false;
    changed |= np_svd_pair(a0, a1, v0, v1, w0, w1);
    changed |= np_svd_pair(a0, a2, v0, v2, w0, w2);
    changed |= np_svd_pair(a0, a3, v0, v3, w0, w3);
    changed |= np_svd_pair(a1, a2, v1, v2, w1, w2);
    changed |= np_svd_pair(a1, a3, v1, v3, w1, w3);
    changed |= np_svd_pair(a2, a3, v2, v3, w2, w3);
    if (!changed) break;
  }
  w0 = __builtin_sqrt(np_sumsq(a0));
  w1 = __builtin_sqrt(np_sumsq(a1));
  w2 = __builtin_sqrt(np_sumsq(a2));
  w3 = __builtin_sqrt(np_sumsq(a3));
  // selection sort, descending: j = the first later maximum under strict <
  {
    int j = 0;
    double wm = w0;
    if (wm < w1) j = 1, wm = w1;
    if (wm < w2) j = 2, wm = w2;
    if (wm < w3) j = 3, wm = w3;
    np_swap_rows(j == 1, v0, v1, w0, w1);
    np_swap_rows(j == 2, v0, v2, w0, w2);
    np_swap_rows(j == 3, v0, v3, w0, w3);
  }
  {
    int j = 1;
    double wm = w1;
    if (wm < w2) j = 2, wm = w2;
    if (wm < w3) j = 3, wm = w3;
    np_swap_rows(j == 2, v1, v2, w1, w2);
    np_swap_rows(j == 3, v1, v3, w1, w3);
  }
  np_swap_rows(w2 < w3, v2, v3, w2, w3);
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = v3[k];
}

// order-preserving key of a float's bit pattern (-0 before +0)
__device__ __forceinline__ uint32_t np_key(float z) {
  const uint32_t b = __builtin_bit_cast(uint32_t, z);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float np_unkey(uint32_t k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ------------------------------------------------------------ k_median_depth
__global__ __launch_bounds__(NP_T) void k_median_depth(const MedianDepthParams P) {
  extern __shared__ uint32_t np_lds[];
  __shared__ int cnt;
  const int p = (int)blockIdx.x;
  const int slot = P.slot ? P.slot[p] : p;
  const int n = min(max(P.nkeys[slot], 0), P.stride);
  const orb_pose_t* pose = P.pose + slot;
  const float r0 = pose->rcw[6], r1 = pose->rcw[7], r2 = pose->rcw[8], zcw = pose->tcw[2];
  const int32_t* pidx = P.pointIndex + (size_t)slot * P.stride;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  for (int i = (int)threadIdx.x; i < n; i += NP_T) {
    const int id = pidx[i];
    if (id >= 0) {
      const float* x = P.points[id].pos;
      const float z = (float)(np_dot3(r0, r1, r2, x[0], x[1], x[2]) + (double)zcw);
      const int at = atomicAdd(&cnt, 1);  // at < n <= stride
      np_lds[at] = np_key(z);
    }
  }
  __syncthreads();
  const int m = cnt;
  if (threadIdx.x == 0) {
    P.count[p] = m;
    if (m == 0) P.median[p] = __builtin_nanf("");
  }
  if (m == 0) return;
  const int k = (m - 1) / P.q;
  for (int i = (int)threadIdx.x; i < m; i += NP_T) {
    const uint32_t key = np_lds[i];
    int less = 0, equal = 0;
    for (int j = 0; j < m; ++j) {
      const uint32_t o = np_lds[j];
      less += o < key;
      equal += o == key;
    }
    // every holder of the answer's key writes the same bits
    if (less <= k && k < less + equal) P.median[p] = np_unkey(key);
  }
}

// -------------------------------------------------------------- k_new_points
struct NpMatch {
  int status;
  float x, y, z;
};

__device__ __forceinline__ bool np_has_x3d(int status) {
  return status == ORB_NP_ACCEPTED || (status >= ORB_NP_Z1 && status <= ORB_NP_SCALE_RATIO);
}

// the loop body (:341-512) for keypoint i1 of slot s1 matched to idx2 of slot s2
__device__ __forceinline__ NpMatch np_match(const NewPointsParams& P, int s1, int s2, int i1,
                                            int idx2, int n2) {
  NpMatch r;
  r.status = ORB_NP_UNDEFINED;
  r.x = r.y = r.z = 0.f;
  if (idx2 >= n2) return r;
  const orb_keypoint_t* kp1 = P.keys + (size_t)s1 * P.stride + i1;
  const orb_keypoint_t* kp2 = P.keys + (size_t)s2 * P.stride + idx2;
  const float u1 = kp1->x, v1 = kp1->y, u2 = kp2->x, v2 = kp2->y;
  const int o1 = kp1->octave, o2 = kp2->octave;
  if (o1 < 0 || o1 >= P.nLevels || o2 < 0 || o2 >= P.nLevels) return r;
  const float ur1 = P.uRight ? P.uRight[(size_t)s1 * P.stride + i1] : -1.f;
  const float ur2 = P.uRight ? P.uRight[(size_t)s2 * P.stride + idx2] : -1.f;
  const bool st1 = ur1 >= 0, st2 = ur2 >= 0;
  const float d1 = st1 ? P.depth[(size_t)s1 * P.stride + i1] : -1.f;
  const float d2 = st2 ? P.depth[(size_t)s2 * P.stride + idx2] : -1.f;
  if ((st1 && !(d1 > 0)) || (st2 && !(d2 > 0))) return r;
  const orb_pose_t* p1 = P.pose + s1;
  const orb_pose_t* p2 = P.pose + s2;

  // :358-364 (N2, N3)
  const float xn1x = (u1 - P.k1[2]) * P.inv1[0], xn1y = (v1 - P.k1[3]) * P.inv1[1];
  const float xn2x = (u2 - P.k2[2]) * P.inv2[0], xn2y = (v2 - P.k2[3]) * P.inv2[1];
  float ray1[3], ray2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    ray1[i] = (p1->rcw[i] * xn1x + p1->rcw[3 + i] * xn1y) + p1->rcw[6 + i] * 1.0f;
    ray2[i] = (p2->rcw[i] * xn2x + p2->rcw[3 + i] * xn2y) + p2->rcw[6 + i] * 1.0f;
  }
  const float cosRays =
      (float)(np_dot3(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]) /
              (np_norm3(ray1[0], ray1[1], ray1[2]) * np_norm3(ray2[0], ray2[1], ray2[2])));
  // :366-375 (N4): the `else if` is the reference's
  float cosStereo = cosRays + 1.0f;
  float cosStereo1 = cosStereo, cosStereo2 = cosStereo;
  if (st1) cosStereo1 = np_cos_stereo(P.mb1, d1);
  else if (st2) cosStereo2 = np_cos_stereo(P.mb2, d2);
  cosStereo = cosStereo2 < cosStereo1 ? cosStereo2 : cosStereo1;  // std::min(a, b)

  float X, Y, Z;
  if (cosRays < cosStereo && cosRays > 0 && (st1 || st2 || (double)cosRays < 0.9998)) {
    // :383-399 (N5, N6, N7): columns of A, rows Tcw = [rcw | tcw]
    float a0[4], a1[4], a2[4], a3[4];
#define NP_COL(col, T1r0, T1r1, T1r2, T2r0, T2r1, T2r2)         \
  col[0] = (xn1x * (T1r2) + (T1r0) * -1.0f) + 0.0f;             \
  col[1] = (xn1y * (T1r2) + (T1r1) * -1.0f) + 0.0f;             \
  col[2] = (xn2x * (T2r2) + (T2r0) * -1.0f) + 0.0f;             \
  col[3] = (xn2y * (T2r2) + (T2r1) * -1.0f) + 0.0f
    NP_COL(a0, p1->rcw[0], p1->rcw[3], p1->rcw[6], p2->rcw[0], p2->rcw[3], p2->rcw[6]);
    NP_COL(a1, p1->rcw[1], p1->rcw[4], p1->rcw[7], p2->rcw[1], p2->rcw[4], p2->rcw[7]);
    NP_COL(a2, p1->rcw[2], p1->rcw[5], p1->rcw[8], p2->rcw[2], p2->rcw[5], p2->rcw[8]);
    NP_COL(a3, p1->tcw[0], p1->tcw[1], p1->tcw[2], p2->tcw[0], p2->tcw[1], p2->tcw[2]);
#undef NP_COL
    float v[4];
    np_svd_vt3(a0, a1, a2, a3, v);
    if (v[3] == 0) {
      r.status = ORB_NP_W_ZERO;
      return r;
    }
    const float inv = (float)(1.0 / (double)v[3]);
    X = v[0] * inv + 0.0f;
    Y = v[1] * inv + 0.0f;
    Z = v[2] * inv + 0.0f;
  } else if (st1 && cosStereo1 < cosStereo2) {
    // KeyFrame::UnprojectStereo(idx1) (N8)
    const float x = (u1 - P.k1[2]) * d1 * P.inv1[0], y = (v1 - P.k1[3]) * d1 * P.inv1[1];
    X = ((p1->rcw[0] * x + p1->rcw[3] * y) + p1->rcw[6] * d1) + p1->ow[0];
    Y = ((p1->rcw[1] * x + p1->rcw[4] * y) + p1->rcw[7] * d1) + p1->ow[1];
    Z = ((p1->rcw[2] * x + p1->rcw[5] * y) + p1->rcw[8] * d1) + p1->ow[2];
  } else if (st2 && cosStereo2 < cosStereo1) {
    const float x = (u2 - P.k2[2]) * d2 * P.inv2[0], y = (v2 - P.k2[3]) * d2 * P.inv2[1];
    X = ((p2->rcw[0] * x + p2->rcw[3] * y) + p2->rcw[6] * d2) + p2->ow[0];
    Y = ((p2->rcw[1] * x + p2->rcw[4] * y) + p2->rcw[7] * d2) + p2->ow[1];
    Z = ((p2->rcw[2] * x + p2->rcw[5] * y) + p2->rcw[8] * d2) + p2->ow[2];
  } else {
    r.status = ORB_NP_LOW_PARALLAX;
    return r;
  }
  r.x = X, r.y = Y, r.z = Z;

  // :420-426 (N1)
  const float z1 = np_row(p1->rcw + 6, p1->tcw[2], X, Y, Z);
  if (z1 <= 0) {
    r.status = ORB_NP_Z1;
    return r;
  }
  const float z2 = np_row(p2->rcw + 6, p2->tcw[2], X, Y, Z);
  if (z2 <= 0) {
    r.status = ORB_NP_Z2;
    return r;
  }
  // :431-460 (N9)
  {
    const float sig = P.sigma2[o1];
    const float x1 = np_row(p1->rcw, p1->tcw[0], X, Y, Z);
    const float y1 = np_row(p1->rcw + 3, p1->tcw[1], X, Y, Z);
    const float invz = (float)(1.0 / (double)z1);
    const float pu = P.k1[0] * x1 * invz + P.k1[2];
    const float pv = P.k1[1] * y1 * invz + P.k1[3];
    const float ex = pu - u1, ey = pv - v1;
    bool out;
    if (!st1) {
      out = (double)(ex * ex + ey * ey) > 5.991 * (double)sig;
    } else {
      const float pur = pu - P.bf1 * invz;
      const float er = pur - ur1;
      out = (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sig;
    }
    if (out) {
      r.status = ORB_NP_REPROJ1;
      return r;
    }
  }
  // :464-487; u2_r uses the current keyframe's mbf (:480)
  {
    const float sig = P.sigma2[o2];
    const float x2 = np_row(p2->rcw, p2->tcw[0], X, Y, Z);
    const float y2 = np_row(p2->rcw + 3, p2->tcw[1], X, Y, Z);
    const float invz = (float)(1.0 / (double)z2);
    const float pu = P.k2[0] * x2 * invz + P.k2[2];
    const float pv = P.k2[1] * y2 * invz + P.k2[3];
    const float ex = pu - u2, ey = pv - v2;
    bool out;
    if (!st2) {
      out = (double)(ex * ex + ey * ey) > 5.991 * (double)sig;
    } else {
      const float pur = pu - P.bf1 * invz;
      const float er = pur - ur2;
      out = (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sig;
    }
    if (out) {
      r.status = ORB_NP_REPROJ2;
      return r;
    }
  }
  // :492-512 (N10)
  const float dist1 = (float)np_norm3(X - p1->ow[0], Y - p1->ow[1], Z - p1->ow[2]);
  const float dist2 = (float)np_norm3(X - p2->ow[0], Y - p2->ow[1], Z - p2->ow[2]);
  if (dist1 == 0 || dist2 == 0) {
    r.status = ORB_NP_ZERO_DIST;
    return r;
  }
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = P.scaleFactors[o1] / P.scaleFactors[o2];
  if (ratioDist * P.ratioFactor < ratioOctave || ratioDist > ratioOctave * P.ratioFactor) {
    r.status = ORB_NP_SCALE_RATIO;
    return r;
  }
  r.status = ORB_NP_ACCEPTED;
  return r;
}

__global__ __launch_bounds__(NP_T) void k_new_points(const NewPointsParams P) {
  extern __shared__ uint32_t np_lds[];  // per slot: x, y, z, status | ordinal << 8
  __shared__ int scan[17];
  __shared__ int counts[ORB_NP_NSTATUS];
  __shared__ int ctl[2];  // cursor, overflow
  const int p = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int s1 = P.kf1Slot[p], s2 = P.kf2Slot[p];
  const int n1 = min(max(P.nkeys[s1], 0), P.stride), n2 = min(max(P.nkeys[s2], 0), P.stride);
  const orb_pose_t* p1 = P.pose + s1;
  const orb_pose_t* p2 = P.pose + s2;
  const size_t row = (size_t)p * P.stride;
  int32_t* cursor = P.pointCursor + P.cursorIndex[p];

  // the gate (:289-311)
  const float baseline =
      (float)np_norm3(p2->ow[0] - p1->ow[0], p2->ow[1] - p1->ow[1], p2->ow[2] - p1->ow[2]);
  bool gated;
  if (!P.monocular) {
    gated = baseline < P.mb2;
  } else {
    const float median = P.medianDepth[p];
    const float ratio = baseline / median;
    gated = (median != median) || (double)ratio < 0.01;
  }
  if (gated) {
    for (int i = tid; i < n1; i += NP_T) P.status[row + i] = ORB_NP_NOT_TRIED;
    if (tid == 0) {
      orb_new_point_info_t info;
      memset(&info, 0, sizeof(info));
      info.gated = 1;
      info.first_point = *cursor;
      P.info[p] = info;
    }
    return;
  }

  if (tid < ORB_NP_NSTATUS) counts[tid] = 0;
  __syncthreads();
  // pass 1
  const int32_t* m12 = P.match12 + row;
  int base = 0;
  for (int r0 = 0; r0 < n1; r0 += NP_T) {
    const int i = r0 + tid;
    NpMatch r;
    r.status = ORB_NP_NOT_TRIED;
    r.x = r.y = r.z = 0.f;
    if (i < n1) {
      const int idx2 = m12[i];
      if (idx2 < 0) r.status = ORB_NP_NO_MATCH;
      else r = np_match(P, s1, s2, i, idx2, n2);
      atomicAdd(&counts[r.status], 1);
    }
    const int acc = r.status == ORB_NP_ACCEPTED ? 1 : 0;
    int total;
    const int ord = base + block_excl_scan(acc, scan, &total);
    base += total;
    if (i < n1) {
      np_lds[4 * i + 0] = __builtin_bit_cast(uint32_t, r.x);
      np_lds[4 * i + 1] = __builtin_bit_cast(uint32_t, r.y);
      np_lds[4 * i + 2] = __builtin_bit_cast(uint32_t, r.z);
      np_lds[4 * i + 3] = (uint32_t)r.status | ((uint32_t)ord << 8);
    }
  }
  const int nNew = base;
  // commit
  if (tid == 0) {
    const int c = *cursor;
    ctl[0] = c;
    ctl[1] = (c < 0 || (long long)c + nNew > (long long)P.pointCapacity) ? 1 : 0;
  }
  __syncthreads();
  const int c = ctl[0];
  if (ctl[1]) {
    if (tid == 0) {
      orb_new_point_info_t info;
      memset(&info, 0, sizeof(info));
      info.overflow = 1;
      P.info[p] = info;
    }
    return;
  }
  // pass 2
  const float sfLast = P.scaleFactors[P.nLevels - 1];
  for (int i = tid; i < n1; i += NP_T) {
    const uint32_t w = np_lds[4 * i + 3];
    const int status = (int)(w & 0xffu), ord = (int)(w >> 8);
    P.status[row + i] = (uint8_t)status;
    if (!np_has_x3d(status)) continue;
    const float X = __builtin_bit_cast(float, np_lds[4 * i + 0]);
    const float Y = __builtin_bit_cast(float, np_lds[4 * i + 1]);
    const float Z = __builtin_bit_cast(float, np_lds[4 * i + 2]);
    float* x3 = P.x3d + 3 * (row + i);
    x3[0] = X, x3[1] = Y, x3[2] = Z;
    if (status != ORB_NP_ACCEPTED) continue;
    // MapPoint::UpdateNormalAndDepth for {KF1, KF2}, reference keyframe KF1 (N7, N10)
    const int idx2 = m12[i];
    const int o1 = P.keys[(size_t)s1 * P.stride + i].octave;  // inside [0, nLevels): pass 1
    const float ax = X - p1->ow[0], ay = Y - p1->ow[1], az = Z - p1->ow[2];
    const float bx = X - p2->ow[0], by = Y - p2->ow[1], bz = Z - p2->ow[2];
    const double na = np_norm3(ax, ay, az), nb = np_norm3(bx, by, bz);
    const float ia = (float)(1.0 / na), ib = (float)(1.0 / nb);
    const float half = (float)(1.0 / 2.0);
    const float nx = ((0.0f + (ax * ia + 0.0f)) + (bx * ib + 0.0f)) * half + 0.0f;
    const float ny = ((0.0f + (ay * ia + 0.0f)) + (by * ib + 0.0f)) * half + 0.0f;
    const float nz = ((0.0f + (az * ia + 0.0f)) + (bz * ib + 0.0f)) * half + 0.0f;
    const float maxD = (float)na * P.scaleFactors[o1];
    const float minD = maxD / sfLast;
    const int id = c + ord;  // < pointCapacity: the commit checked c + nNew
    uint32_t* rec = reinterpret_cast<uint32_t*>(P.points + id);
    rec[0] = __builtin_bit_cast(uint32_t, X);
    rec[1] = __builtin_bit_cast(uint32_t, Y);
    rec[2] = __builtin_bit_cast(uint32_t, Z);
    rec[3] = __builtin_bit_cast(uint32_t, nx);
    rec[4] = __builtin_bit_cast(uint32_t, ny);
    rec[5] = __builtin_bit_cast(uint32_t, nz);
    rec[6] = __builtin_bit_cast(uint32_t, minD);
    rec[7] = __builtin_bit_cast(uint32_t, maxD);
    rec[8] = 0x00010000u;  // bad 0, seen 0, has_obs 1, _pad 0
    int32_t* pair = P.newPairs + 2 * (row + ord);  // ord < n1 <= stride
    pair[0] = i;
    pair[1] = idx2;
    P.pointIndex[(size_t)s1 * P.stride + i] = id;
    // idx2 < n2 <= stride: pass 1.  Several accepted i1 may name one idx2 (the
    // matcher never sets vbMatched2): the reference's last AddMapPoint is the
    // largest i1, ids ascend with i1, and the entry was below the cursor
    atomicMax(&P.pointIndex[(size_t)s2 * P.stride + idx2], id);
  }
  if (tid == 0) {
    orb_new_point_info_t info;
    memset(&info, 0, sizeof(info));
    info.n_new = nNew;
    info.first_point = c;
    for (int k = 0; k < ORB_NP_NSTATUS; ++k) info.counts[k] = counts[k];
    P.info[p] = info;
    *cursor = c + nNew;
  }
}

// ---------------------------------------------------------------- launchers
extern "C" int orb_k_median_depth_max_stride(void) {
  return (int)((ORB_LDS_PER_CU - NP_FIXED_LDS) / 4) & ~63;
}

extern "C" int orb_k_new_points_max_stride(void) {
  return (int)((ORB_LDS_PER_CU - NP_FIXED_LDS) / 16) & ~63;
}

extern "C" hipError_t orb_k_median_depth(const MedianDepthParams* params, hipStream_t s) {
  const MedianDepthParams P = *params;
  if (P.stride <= 0 || P.stride > orb_k_median_depth_max_stride() || P.q < 1)
    return hipErrorInvalidValue;
  const size_t lds = 4 * (size_t)P.stride;
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute((const void*)k_median_depth,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_median_depth, dim3(P.nProblems), dim3(NP_T), lds, s, P);
  return hipGetLastError();
}

extern "C" hipError_t orb_k_new_points(const NewPointsParams* params, hipStream_t s) {
  const NewPointsParams P = *params;
  if (P.stride <= 0 || P.stride > orb_k_new_points_max_stride() || P.nLevels < 2 ||
      P.nLevels > ORB_MAX_LEVELS)
    return hipErrorInvalidValue;
  const size_t lds = 16 * (size_t)P.stride;
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute((const void*)k_new_points,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_new_points, dim3(P.nProblems), dim3(NP_T), lds, s, P);
  return hipGetLastError();
}
