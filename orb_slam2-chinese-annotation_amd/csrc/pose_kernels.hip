// pose_kernels.hip -- Optimizer::PoseOptimization (src/Optimizer.cc:243-477) on
// the device: the motion-only optimisation of one SE3 vertex against one unary
// edge per matched keypoint, with the g2o parts it reaches restated literally
// (tests/poseopt_ref.py is the same text in numpy); those it
// shares with sim3opt_kernels.hip are in g2o_device.h.
//
//   k_pose_optimization   one 64-lane workgroup per problem, one launch per call:
//     1. the problem's edges are compacted once, in ascending keypoint order,
//        by ballot prefix into 32-byte records (Xw, observation, invSigma2,
//        keypoint slot | kind | level) in LDS (stride <= PO_LDS_EDGES) or in
//        the handle's global scratch;
//     2. an evaluation pass runs all lanes over the edges, 64 at a time: map,
//        project, error, chi2, Huber and (for buildSystem) the Jacobian and
//        the edge's 27 terms of b and the lower triangle of H;
//     3. the order-dependent sums stay exact by construction: a chunk's terms
//        go to LDS term-major, half a wave at a time (a 32-edge tile keeps a
//        1,000-slot problem under 40 KiB, four workgroups per CU), and 28
//        lanes each own one accumulator (the robust chi2, 6 of b, 21 of H) and
//        add their row in edge order, +0.0 for the edges that are not active;
//     4. the 6x6 pivoted LDLT, exp, the quaternion update and the
//        Levenberg-Marquardt driver (g2o_device.h) are the same doubles in
//        every lane: the sums reach the lanes through LDS.
//   All four rounds and every trial run inside the kernel; the loops are
//   bounded by 4 x 10 x 10 trials whatever the input (NaN included).
//
// Compiled with -ffp-contract=off: every expression evaluates as written.
#include <hip/hip_runtime.h>

#include "orb_device.h"
#include "g2o_device.h"
#include "orb_kernels.h"

namespace {

struct PoEdge {
  float X[3];     // GetWorldPos()
  float obs[3];   // kpUn.pt.x, kpUn.pt.y, mvuRight
  float inv;      // mvInvLevelSigma2[octave]
  uint32_t meta;  // keypoint slot | PO_OUTLIER (mvbOutlier == level 1) | PO_STEREO
};
static_assert(sizeof(PoEdge) == 32, "PoEdge is 32 bytes");
constexpr uint32_t PO_STEREO = 1u << 31, PO_OUTLIER = 1u << 30, PO_SLOT = PO_OUTLIER - 1;

constexpr int PO_TERMS = 28;   // 0: robust chi2, 1..6: b, 7..27: H(r, c), c <= r, at 7 + r(r+1)/2 + c
// A chunk's terms are staged half a wave at a time: the tile holds 32 edges
constexpr int PO_HALF = ORB_WAVE >= 2 ? ORB_WAVE / 2 : 1;
constexpr int PO_PITCH = PO_HALF + 1;  // doubles per term row: lane t's row starts at bank 2t
// LDS carve (dynamic, 16-byte multiples): term tile, solver state, edge records
constexpr int PO_LDS_TILE = (PO_TERMS * PO_PITCH * 8 + 15) / 16 * 16;  // 7,392
constexpr int PO_LDS_STATE = 256;
struct PoState {
  double acc[PO_TERMS];  // the sums of the last pass (acc[0] of the last pass of either kind)
};
static_assert(sizeof(PoState) <= PO_LDS_STATE, "solver state fits its carve");

struct PoEst : G2oQuat {  // SE3Quat: _r (x, y, z, w), _t
  double tx, ty, tz;
};
static_assert(sizeof(PoEst) == 56, "PoEst is seven doubles");

// SE3Quat::exp (se3quat.h:223-257)
__device__ __forceinline__ PoEst po_exp(const double* u) {
  const double eye[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  double theta, Om[9], Om2[9], R[9], V[9], s, c;
  if (g2o_rodrigues(u, theta, Om, Om2, R, s, c)) {
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i] = R[i];
  } else {
    const double b = (1.0 - c) / (theta * theta), d = (theta - s) / ((theta * theta) * theta);
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i] = (eye[i] + b * Om[i]) + d * Om2[i];
  }
  PoEst e;
  g2o_quat_from_matrix(R, e);
  g2o_normalize_rotation(e);
  e.tx = (V[0] * u[3] + V[1] * u[4]) + V[2] * u[5];
  e.ty = (V[3] * u[3] + V[4] * u[4]) + V[5] * u[5];
  e.tz = (V[6] * u[3] + V[7] * u[4]) + V[8] * u[5];
  return e;
}

// SE3Quat::operator* (se3quat.h:104-110)
__device__ __forceinline__ PoEst po_mul(const PoEst& a, const PoEst& b) {
  PoEst r;
  double rx, ry, rz;
  g2o_rotate(a, b.tx, b.ty, b.tz, rx, ry, rz);
  r.tx = a.tx + rx;
  r.ty = a.ty + ry;
  r.tz = a.tz + rz;
  g2o_quat_mul(a, b, r);
  g2o_normalize_rotation(r);
  return r;
}

struct PoCam {
  double fx, fy, cx, cy, bf;
};

// computeError of one edge (types_six_dof_expmap.h:153-157, :184-188) with
// both cam_project forms (.cpp:290-306); returns chi2 (base_edge.h) and the
// mapped point.
__device__ __forceinline__ double po_error(const PoEdge& r, bool stereo, const PoEst& est,
                                           const PoCam& cam, double& x, double& y, double& z,
                                           double& e0, double& e1, double& e2) {
  g2o_rotate(est, (double)r.X[0], (double)r.X[1], (double)r.X[2], x, y, z);
  x = x + est.tx;  // SE3Quat::map (se3quat.h:217-220)
  y = y + est.ty;
  z = z + est.tz;
  const double s = (double)r.inv;
  if (stereo) {
    const double iz = (double)(float)(1.0 / z);  // const float invz = 1.0f / z (.cpp:300)
    const double us = (x * iz) * cam.fx + cam.cx;
    e0 = (double)r.obs[0] - us;
    e1 = (double)r.obs[1] - ((y * iz) * cam.fy + cam.cy);
    e2 = (double)r.obs[2] - (us - cam.bf * iz);
    return (e0 * (s * e0) + e1 * (s * e1)) + e2 * (s * e2);
  }
  e0 = (double)r.obs[0] - ((x / z) * cam.fx + cam.cx);  // project2d (se3_ops.hpp)
  e1 = (double)r.obs[1] - ((y / z) * cam.fy + cam.cy);
  e2 = 0.0;
  return e0 * (s * e0) + e1 * (s * e1);
}

// One pass over the edges at `est`: FULL = computeActiveErrors + activeRobustChi2
// + buildSystem (28 sums), otherwise the robust chi2 alone.  The sums land in
// S.acc.  Every lane must call it.
template <bool FULL>
__device__ void po_pass(const PoEdge* recs, int E, const PoEst& est, const PoCam& cam,
                        bool robust, double deltaMono, double deltaStereo, double* tile,
                        PoState& S) {
  const int lane = lane_id();
  constexpr int NT = FULL ? PO_TERMS : 1;
  // lane t owns the terms t, t + ORB_WAVE, ...: at 28 terms and 64 lanes that is
  // one accumulator in each of the first 28 lanes
  constexpr int OWN = (PO_TERMS + ORB_WAVE - 1) / ORB_WAVE;
  double acc[OWN];
#pragma unroll
  for (int o = 0; o < OWN; ++o) acc[o] = 0.0;
  for (int c0 = 0; c0 < E; c0 += ORB_WAVE) {
    const int e = c0 + lane;
    bool active = false;
    double tv[NT];  // this lane's terms
    if (e < E) {
      const PoEdge r = recs[e];
      active = !(r.meta & PO_OUTLIER);
      if (active) {
        const bool stereo = r.meta & PO_STEREO;
        double x, y, z, e0, e1, e2;
        const double chi2 = po_error(r, stereo, est, cam, x, y, z, e0, e1, e2);
        double rho0 = chi2, rho1 = 1.0;
        if (robust) g2o_huber(chi2, stereo ? deltaStereo : deltaMono, rho0, rho1);
        tv[0] = rho0;
        if constexpr (FULL) {
          // linearizeOplus (.cpp:266-288, :335-364); row 2 only for stereo
          const double invz = 1.0 / z, invz_2 = invz * invz;
          double A[3][6];
          A[0][0] = ((x * y) * invz_2) * cam.fx;
          A[0][1] = (-(1 + ((x * x) * invz_2))) * cam.fx;
          A[0][2] = (y * invz) * cam.fx;
          A[0][3] = (-invz) * cam.fx;
          A[0][4] = 0.0;
          A[0][5] = (x * invz_2) * cam.fx;
          A[1][0] = (1 + (y * y) * invz_2) * cam.fy;
          A[1][1] = (((-x) * y) * invz_2) * cam.fy;
          A[1][2] = ((-x) * invz) * cam.fy;
          A[1][3] = 0.0;
          A[1][4] = (-invz) * cam.fy;
          A[1][5] = (y * invz_2) * cam.fy;
          A[2][0] = A[0][0] - (cam.bf * y) * invz_2;
          A[2][1] = A[0][1] + (cam.bf * x) * invz_2;
          A[2][2] = A[0][2];
          A[2][3] = A[0][3];
          A[2][4] = 0.0;
          A[2][5] = A[0][5] - cam.bf * invz_2;
          // constructQuadraticForm (base_unary_edge.hpp:43-72): ((rho1 A^T) Omega) e
          // and (A^T (rho1 Omega)) A, left-associated; without a kernel rho1 = 1
          // gives the plain forms bit for bit
          const double s = (double)r.inv, w = s * rho1;
          const double ev[3] = {e0, e1, e2};
#pragma unroll
          for (int q = 0; q < 6; ++q) {
            double t = ((rho1 * A[0][q]) * s) * ev[0] + ((rho1 * A[1][q]) * s) * ev[1];
            if (stereo) t = t + ((rho1 * A[2][q]) * s) * ev[2];
            tv[1 + q] = -t;  // b -= term: the owner adds the negation
#pragma unroll
            for (int p = 0; p <= q; ++p) {
              double h = (A[0][q] * w) * A[0][p] + (A[1][q] * w) * A[1][p];
              if (stereo) h = h + (A[2][q] * w) * A[2][p];
              tv[7 + q * (q + 1) / 2 + p] = h;
            }
          }
        }
      }
    }
    const unsigned long long mask = __ballot(active);
#pragma unroll
    for (int h = 0; h < ORB_WAVE / PO_HALF; ++h) {
      if (active && lane / PO_HALF == h) {
#pragma unroll
        for (int t = 0; t < NT; ++t) tile[t * PO_PITCH + lane % PO_HALF] = tv[t];
      }
      __syncthreads();
#pragma unroll
      for (int o = 0; o < OWN; ++o) {
        const int t = lane + o * ORB_WAVE;
        if (t < NT) {
          // the row is read whole, then added in edge order.  An edge that is
          // not active adds +0.0 in place of its stale tile entry, which leaves
          // the accumulator as it is: it starts at +0.0, and x + y is -0.0 only
          // when both are -0.0, so it never holds the one value +0.0 changes
          const double* row = tile + t * PO_PITCH;
          double v[PO_HALF];
#pragma unroll
          for (int j = 0; j < PO_HALF; ++j) v[j] = row[j];
#pragma unroll
          for (int j = 0; j < PO_HALF; ++j)
            acc[o] = acc[o] + (((mask >> (h * PO_HALF + j)) & 1ull) ? v[j] : 0.0);
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int o = 0; o < OWN; ++o)
    if (lane + o * ORB_WAVE < NT) S.acc[lane + o * ORB_WAVE] = acc[o];
  __syncthreads();
}

}  // namespace

template <bool GLOBAL>
__global__ __launch_bounds__(64) void k_pose_optimization(
    const PoseOptParams P, const int32_t* __restrict__ counts,
    const orb_keypoint_t* __restrict__ keysUn, const float* __restrict__ uRight,
    const int32_t* __restrict__ pointIndex, const uint8_t* __restrict__ points,
    const orb_pose_t* poseIn, orb_pose_t* poseOut, uint8_t* outlier,
    orb_pose_opt_info_t* __restrict__ info, PoEdge* gRecs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char poLds[];
  double* tile = reinterpret_cast<double*>(poLds);
  PoState& S = *reinterpret_cast<PoState*>(poLds + PO_LDS_TILE);
  const int f = blockIdx.x, lane = lane_id();
  PoEdge* recs = GLOBAL ? gRecs + (size_t)f * P.stride
                        : reinterpret_cast<PoEdge*>(poLds + PO_LDS_TILE + PO_LDS_STATE);
  const int n = min(max(counts ? counts[f] : P.nSingle, 0), P.stride);
  const size_t base = (size_t)f * P.stride;
  const uint8_t* pts = points + (size_t)((long long)f * P.ptStride) * (size_t)P.pointStrideBytes;
  const orb_pose_t pin = poseIn[f];

  // ---- the edges, in ascending keypoint order (:290-380)
  const unsigned long long ltMask = (1ull << lane) - 1ull;
  int E = 0;
  bool badOctave = false;
  for (int b0 = 0; b0 < n; b0 += ORB_WAVE) {  // (uniform trip count: whole waves ballot)
    const int i = b0 + lane;
    int pi = -1;
    if (i < n) pi = pointIndex[base + i];
    const bool has = pi >= 0;
    bool okOct = true;
    PoEdge r;
    if (has) {
      const orb_keypoint_t kp = keysUn[base + i];
      okOct = kp.octave >= 0 && kp.octave < P.nLevels;
      const float ur = uRight ? uRight[base + i] : -1.0f;
      const float* X = reinterpret_cast<const float*>(pts + (size_t)pi * P.pointStrideBytes);
      r.X[0] = X[0];
      r.X[1] = X[1];
      r.X[2] = X[2];
      r.obs[0] = kp.x;
      r.obs[1] = kp.y;
      r.obs[2] = ur;
      r.inv = 0.0f;
#pragma unroll
      for (int l = 0; l < ORB_MAX_LEVELS; ++l)  // (static indices into the by-value parameters)
        if (kp.octave == l && l < P.nLevels) r.inv = P.invLevelSigma2[l];
      r.meta = (uint32_t)i | (ur < 0 ? 0u : PO_STEREO);  // :298
    }
    const unsigned long long b = __ballot(has);
    if (__ballot(has && !okOct)) badOctave = true;
    if (has) recs[E + __popcll(b & ltMask)] = r;
    E += __popcll(b);
  }
  __syncthreads();
  if (badOctave || E < 3) {  // :384-385, and the ABI's answer to a bad octave
    if (!badOctave)
      for (int e = lane; e < E; e += ORB_WAVE) outlier[base + (recs[e].meta & PO_SLOT)] = 0;  // :301, :342
    if (lane == 0) {
      poseOut[f] = pin;
      orb_pose_opt_info_t r;
      r.n_inliers = 0;
      r.n_edges = badOctave ? -1 : E;
      r.lm_iterations = 0;
      r.rejected_trials = 0;
      info[f] = r;
    }
    return;
  }

  PoCam cam;
  cam.fx = (double)P.fx;
  cam.fy = (double)P.fy;
  cam.cx = (double)P.cx;
  cam.cy = (double)P.cy;
  cam.bf = (double)P.bf;
  const double deltaMono = (double)(float)sqrt(5.991), deltaStereo = (double)(float)sqrt(7.815);  // :283-284
  const float chi2Mono = 5.991f, chi2Stereo = 7.815f;  // :389-390

  // Converter::toSE3Quat (src/Converter.cc:39-49)
  PoEst est0;
  {
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (double)pin.rcw[i];
    g2o_quat_from_matrix(R, est0);
    g2o_normalize_rotation(est0);
    est0.tx = (double)pin.tcw[0];
    est0.ty = (double)pin.tcw[1];
    est0.tz = (double)pin.tcw[2];
  }
  PoEst est = est0, last = est0;  // last: where the edges' _error was last computed
  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // BlockSolver::_x
  bool robust = true, lastIsEst = true;
  int nBad = 0, lmIters = 0, rejected = 0;
  auto full_pass = [&] {
    ++lmIters;
    po_pass<true>(recs, E, est, cam, robust, deltaMono, deltaStereo, tile, S);
  };
  auto trial_pass = [&](const double* step) {
    last = po_mul(po_exp(step), est);  // oplusImpl (.h:73-76)
    po_pass<false>(recs, E, last, cam, robust, deltaMono, deltaStereo, tile, S);
  };
  auto accept = [&] { est = last; lastIsEst = true; };
  auto reject = [&] { ++rejected; lastIsEst = false; };
  for (int it = 0; it < 4; ++it) {
    est = est0;  // :397
    last = est0;
    lastIsEst = true;
    if (E - nBad > 0)  // (optimize() returns at once without active vertices)
      g2o_lm_optimize<6>(S.acc, 10, x, full_pass, trial_pass, accept, reject);  // optimize(10)
    // ---- classification (:402-465): an active edge from its last computed
    // error, a level-1 edge recomputed at the final estimate (:411-414)
    nBad = 0;
    for (int c0 = 0; c0 < E; c0 += ORB_WAVE) {
      const int e = c0 + lane;
      bool bad = false;
      if (e < E) {
        PoEdge r = recs[e];
        const bool stereo = r.meta & PO_STEREO;
        double px, py, pz, e0, e1, e2;
        const bool wasOut = r.meta & PO_OUTLIER;
        const float chi2 =
            (float)po_error(r, stereo, (wasOut || lastIsEst) ? est : last, cam, px, py, pz, e0, e1, e2);
        bad = chi2 > (stereo ? chi2Stereo : chi2Mono);
        recs[e].meta = (r.meta & ~PO_OUTLIER) | (bad ? PO_OUTLIER : 0u);
      }
      nBad += __popcll(__ballot(bad));
    }
    __syncthreads();
    if (it == 2) robust = false;  // :433-435
    if (E < 10) break;            // :467
  }

  for (int e = lane; e < E; e += ORB_WAVE) {
    const uint32_t m = recs[e].meta;
    outlier[base + (m & PO_SLOT)] = (m & PO_OUTLIER) ? 1 : 0;
  }
  if (lane == 0) {
    // Converter::toCvMat (src/Converter.cc:51-73), Frame::UpdatePoseMatrices
    // (src/Frame.cc:294-300; float products summed left to right, App. A)
    double R[9];
    g2o_to_matrix(est, R);
    orb_pose_t o;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.rcw[i] = (float)R[i];
    o.tcw[0] = (float)est.tx;
    o.tcw[1] = (float)est.ty;
    o.tcw[2] = (float)est.tz;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      o.ow[i] = -((o.rcw[i] * o.tcw[0] + o.rcw[3 + i] * o.tcw[1]) + o.rcw[6 + i] * o.tcw[2]);
    poseOut[f] = o;
    orb_pose_opt_info_t r;
    r.n_inliers = E - nBad;
    r.n_edges = E;
    r.lm_iterations = lmIters;
    r.rejected_trials = rejected;
    info[f] = r;
  }
}

extern "C" size_t orb_k_pose_optimization_scratch(int nProblems, int stride) {
  if (stride <= PO_LDS_EDGES) return 0;
  return (size_t)nProblems * (size_t)stride * sizeof(PoEdge);
}

extern "C" hipError_t orb_k_pose_optimization(const PoseOptParams* params, const int32_t* counts,
                                              const orb_keypoint_t* keysUn, const float* uRight,
                                              const int32_t* pointIndex, const void* points,
                                              const orb_pose_t* poseIn, orb_pose_t* poseOut,
                                              uint8_t* outlier, orb_pose_opt_info_t* info,
                                              void* scratch, hipStream_t s) {
  if (params->nProblems <= 0 || params->stride <= 0) return hipSuccess;
  const size_t fixed = PO_LDS_TILE + PO_LDS_STATE;
  if (params->stride <= PO_LDS_EDGES) {
    hipLaunchKernelGGL(k_pose_optimization<false>, dim3(params->nProblems), dim3(64),
                       fixed + (size_t)params->stride * sizeof(PoEdge), s, *params, counts, keysUn,
                       uRight, pointIndex, (const uint8_t*)points, poseIn, poseOut, outlier, info,
                       (PoEdge*)nullptr);
  } else {
    if (!scratch) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pose_optimization<true>, dim3(params->nProblems), dim3(64), fixed, s,
                       *params, counts, keysUn, uRight, pointIndex, (const uint8_t*)points, poseIn,
                       poseOut, outlier, info, (PoEdge*)scratch);
  }
  return hipGetLastError();
}
