// sim3opt_kernels.hip -- Optimizer::OptimizeSim3 (src/Optimizer.cc:1130-1326) on
// the device: one free VertexSim3Expmap against two binary edges per
// correspondence (EdgeSim3ProjectXYZ, EdgeInverseSim3ProjectXYZ) whose other
// vertex is fixed, with the g2o parts it reaches restated literally (DESIGN.md
// §4.12; tests/sim3opt_ref.py is the same text in numpy).  The architecture is
// k_pose_optimization's (§4.5), and what the two share is in g2o_device.h:
//
//   k_optimize_sim3   one 64-lane workgroup per problem, one launch per call:
//     1. the kept pairs are compacted once, in ascending i1, by ballot prefix
//        into 56-byte records (P3D1c, P3D2c, both observations, both
//        invSigma2, i1, removed) in LDS;
//     2. a linearisation perturbs the one free vertex, so the 15 estimates
//        Sim3(+-1e-9 e_d) * estimate (the centre included) and their 15
//        inverses are the same for every edge: every lane computes them alike
//        and lane 0 leaves them in LDS;
//     3. a pass runs all lanes over the pairs, 64 at a time: each lane
//        evaluates its pair's two edges at the 15 estimates (numeric Jacobian,
//        base_binary_edge.hpp:131-200), chi2, Huber and the edge's 36 terms
//        (robust chi2, 7 of b, 28 of the lower triangle of H) into one
//        term-major LDS tile per edge kind;
//     4. 36 lanes each own one accumulator and add their two rows in insertion
//        order e12(i), e21(i), e12(i'), ..., +0.0 for a removed pair;
//     5. the 7x7 pivoted LDLT, the Sim3 exponential, s * estimate and the
//        Levenberg-Marquardt driver are the same doubles in every lane.
//   Both optimize() calls, every trial, both classifications and the gate run
//   inside the kernel; the loops are bounded by (5 + 10) x 10 trials whatever
//   the input (NaN included).
//
// Compiled with -ffp-contract=off: every expression evaluates as written.
#include <hip/hip_runtime.h>

#include "orb_device.h"
#include "g2o_device.h"
#include "orb_kernels.h"

namespace {

struct SoRec {
  float x1[3];  // P3D1c = R1w * pos(pMP1) + t1w
  float x2[3];  // P3D2c = R2w * pos(pMP2) + t2w
  float o1[2];  // kpUn1.pt
  float o2[2];  // kpUn2.pt
  float inv1;   // pKF1->mvInvLevelSigma2[kpUn1.octave]
  float inv2;   // pKF2->mvInvLevelSigma2[kpUn2.octave]
  int32_t i1;   // vnIndexEdge
  uint32_t removed;  // vpEdges12[i] == NULL
};
static_assert(sizeof(SoRec) == 56, "SoRec is 56 bytes");

constexpr int SO_TERMS = 36;  // 0: robust chi2, 1..7: b, 8..35: H(r, c), c <= r, at 8 + r(r+1)/2 + c
constexpr int SO_PITCH = ORB_WAVE + 1;  // doubles per term row: lane t's row starts at bank 2t
// LDS carve (dynamic, 16-byte multiples): two term tiles, solver state, pair records
constexpr int SO_LDS_TILE = (SO_TERMS * SO_PITCH * 8 + 15) / 16 * 16;  // 18,720
constexpr int SO_NEST = 15;  // the centre, then +delta and -delta along each of 7 axes

struct SoEst : G2oQuat {  // g2o::Sim3: r (x, y, z, w), t, s
  double tx, ty, tz, s;
};
static_assert(sizeof(SoEst) == 64, "SoEst is eight doubles");
struct SoState {
  double acc[SO_TERMS];  // the sums of the last pass (acc[0] of the last pass of either kind)
  SoEst fwd[SO_NEST];    // the estimates an edge is evaluated at
  SoEst inv[SO_NEST];    // their inverse()
};
constexpr int SO_LDS_STATE = (sizeof(SoState) + 15) / 16 * 16;  // 2,208
constexpr size_t SO_LDS_FIXED = 2 * (size_t)SO_LDS_TILE + SO_LDS_STATE;

// Sim3(const Vector7d&) (sim3.h:70-142)
__device__ __forceinline__ SoEst so_exp(const double* u) {
  const double sigma = u[6];
  const double eye[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  double theta, Om[9], Om2[9], R[9], sn, cs;
  SoEst e;
  e.s = pinned_exp(sigma);
  const bool smallS = uni(fabs(sigma) < 0.00001);
  const bool smallT = g2o_rodrigues(u, theta, Om, Om2, R, sn, cs);
  double A, B, C;
  if (smallS) {
    C = 1;
    if (smallT) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cs) / (theta2);
      B = (theta - sn) / (theta2 * theta);
    }
  } else {
    C = (e.s - 1) / sigma;
    if (smallT) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * e.s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * e.s) / (sigma2 * sigma);
    } else {
      const double a = e.s * sn, b = e.s * cs;
      const double theta2 = theta * theta, sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  g2o_quat_from_matrix(R, e);
  double W[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) W[i] = (A * Om[i] + B * Om2[i]) + C * eye[i];
  e.tx = (W[0] * u[3] + W[1] * u[4]) + W[2] * u[5];
  e.ty = (W[3] * u[3] + W[4] * u[4]) + W[5] * u[5];
  e.tz = (W[6] * u[3] + W[7] * u[4]) + W[8] * u[5];
  return e;
}

// Sim3::operator* (sim3.h:266-272)
__device__ __forceinline__ SoEst so_mul(const SoEst& a, const SoEst& b) {
  SoEst r;
  g2o_quat_mul(a, b, r);
  double rx, ry, rz;
  g2o_rotate(a, b.tx, b.ty, b.tz, rx, ry, rz);
  r.tx = a.s * rx + a.tx;
  r.ty = a.s * ry + a.ty;
  r.tz = a.s * rz + a.tz;
  r.s = a.s * b.s;
  return r;
}

// Sim3::inverse (sim3.h:233-236)
__device__ __forceinline__ SoEst so_inverse(const SoEst& a) {
  SoEst r;
  r.qx = -a.qx;
  r.qy = -a.qy;
  r.qz = -a.qz;
  r.qw = a.qw;
  const double c = -1. / a.s;
  g2o_rotate(r, c * a.tx, c * a.ty, c * a.tz, r.tx, r.ty, r.tz);
  r.s = 1. / a.s;
  return r;
}

// computeError of either edge (types_seven_dof_expmap.h:138-145, :160-167) at
// the estimate (or inverse) `e`: obs - cam_map(project(e.map(X)))
__device__ __forceinline__ void so_error(const SoEst& e, const float* X, const float* obs,
                                         const double* K, double& e0, double& e1) {
  double x, y, z;
  g2o_rotate(e, (double)X[0], (double)X[1], (double)X[2], x, y, z);
  x = e.s * x + e.tx;  // Sim3::map (sim3.h:144-146)
  y = e.s * y + e.ty;
  z = e.s * z + e.tz;
  e0 = (double)obs[0] - ((x / z) * K[0] + K[2]);  // project, cam_map1 / cam_map2
  e1 = (double)obs[1] - ((y / z) * K[1] + K[3]);
}

// One edge's terms into column `col` of its tile.  ests: the 15 estimates of
// this edge kind (the centre alone when !FULL).
template <bool FULL>
__device__ __forceinline__ void so_edge_terms(const SoEst* ests, const float* X, const float* obs,
                                              float inv, const double* K, double delta,
                                              double* tile, int col) {
  double e0, e1;
  so_error(ests[0], X, obs, K, e0, e1);
  const double s = (double)inv;
  const double chi2 = e0 * (s * e0) + e1 * (s * e1);  // BaseEdge::chi2
  double rho0, rho1;
  g2o_huber(chi2, delta, rho0, rho1);
  tile[col] = rho0;
  if constexpr (FULL) {
    // linearizeOplus (base_binary_edge.hpp:131-200), the free vertex j alone
    const double scalar = 1.0 / (2 * 1e-9);
    double B0[7], B1[7];
#pragma unroll
    for (int d = 0; d < 7; ++d) {
      double p0, p1, m0, m1;
      so_error(ests[1 + 2 * d], X, obs, K, p0, p1);
      so_error(ests[2 + 2 * d], X, obs, K, m0, m1);
      B0[d] = scalar * (p0 - m0);
      B1[d] = scalar * (p1 - m1);
    }
    // constructQuadraticForm (:91-113), `to` alone free
    double r0 = -(s * e0), r1 = -(s * e1);
    r0 = r0 * rho1;
    r1 = r1 * rho1;
    const double w = rho1 * s;  // robustInformation (base_edge.h:96-102)
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      tile[(1 + q) * SO_PITCH + col] = B0[q] * r0 + B1[q] * r1;
#pragma unroll
      for (int p = 0; p <= q; ++p)
        tile[(8 + q * (q + 1) / 2 + p) * SO_PITCH + col] = (B0[q] * w) * B0[p] + (B1[q] * w) * B1[p];
    }
  }
}

// The estimates a pass evaluates at: S.fwd[0] = est and its inverse; FULL adds
// Sim3(+-delta e_d) * est, d = 0..6, through oplusImpl
// (types_seven_dof_expmap.h:60-69).  Every lane must call it.
template <bool FULL>
__device__ void so_setup(const SoEst& est, bool fixScale, SoState& S) {
  const bool w = lane_id() == 0;
  const SoEst ie = so_inverse(est);
  if (w) {
    S.fwd[0] = est;
    S.inv[0] = ie;
  }
  if constexpr (FULL) {
#pragma nounroll
    for (int k = 1; k < SO_NEST; ++k) {
      const int d = (k - 1) >> 1;
      const double step = (k & 1) ? 1e-9 : -1e-9;
      double u[7];
#pragma unroll
      for (int j = 0; j < 7; ++j) u[j] = j == d ? step : 0.0;
      if (fixScale) u[6] = 0;
      const SoEst pe = so_mul(so_exp(u), est);
      const SoEst pi = so_inverse(pe);
      if (w) {
        S.fwd[k] = pe;
        S.inv[k] = pi;
      }
    }
  }
  __syncthreads();
}

// One pass over the pairs at the estimates in S: FULL = computeActiveErrors +
// activeRobustChi2 + buildSystem (36 sums), otherwise the robust chi2 alone.
// The sums land in S.acc.  Every lane must call it.
template <bool FULL>
__device__ void so_pass(const SoRec* recs, int E, const double* K1, const double* K2, double delta,
                        double* tile12, double* tile21, SoState& S) {
  const int lane = lane_id();
  constexpr int NT = FULL ? SO_TERMS : 1;
  double acc = 0.0;  // lane t < NT owns term t
  for (int c0 = 0; c0 < E; c0 += ORB_WAVE) {
    const int e = c0 + lane;
    bool active = false;
    if (e < E) {
      const SoRec r = recs[e];
      active = !r.removed;
      if (active) {
        // e12: x1 = S12 * X2 (:1224-1239); e21: x2 = S21 * X1 (:1241-1257)
        so_edge_terms<FULL>(S.fwd, r.x2, r.o1, r.inv1, K1, delta, tile12, lane);
        so_edge_terms<FULL>(S.inv, r.x1, r.o2, r.inv2, K2, delta, tile21, lane);
      }
    }
    const unsigned long long mask = __ballot(active);
    __syncthreads();
    if (lane < NT) {
      // the two rows are added in insertion order e12(i), e21(i), e12(i'), ...
      // A pair that is not active adds +0.0 in place of its stale tile
      // entries, which leaves the accumulator as it is: it starts at +0.0, and
      // x + y is -0.0 only when both are -0.0, so it never holds the one value
      // +0.0 changes
      const double* row12 = tile12 + lane * SO_PITCH;
      const double* row21 = tile21 + lane * SO_PITCH;
      for (int j0 = 0; j0 < ORB_WAVE; j0 += 16) {
        double a[16], b[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          a[j] = row12[j0 + j];
          b[j] = row21[j0 + j];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const bool on = (mask >> (j0 + j)) & 1ull;
          acc = acc + (on ? a[j] : 0.0);
          acc = acc + (on ? b[j] : 0.0);
        }
      }
    }
    __syncthreads();
  }
  if (lane < NT) S.acc[lane] = acc;
  __syncthreads();
}

__device__ __forceinline__ void so_write_result(orb_sim3_opt_result_t* out, int status, int nCorr,
                                                int nBad, int nIn, const SoEst& e) {
  orb_sim3_opt_result_t r;
  r.status = status;
  r.n_corr = nCorr;
  r.n_bad = nBad;
  r.n_inliers = nIn;
  r.q[0] = e.qx;
  r.q[1] = e.qy;
  r.q[2] = e.qz;
  r.q[3] = e.qw;
  r.t[0] = e.tx;
  r.t[1] = e.ty;
  r.t[2] = e.tz;
  r.s = e.s;
  double R[9];
  g2o_to_matrix(e, R);
#pragma unroll
  for (int i = 0; i < 9; ++i) r.R[i] = (float)R[i];
  r.t_f[0] = (float)e.tx;
  r.t_f[1] = (float)e.ty;
  r.t_f[2] = (float)e.tz;
  r.s_f = (float)e.s;
  r._pad = 0;
  *out = r;
}

}  // namespace

__global__ __launch_bounds__(64) void k_optimize_sim3(const Sim3OptParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char soLds[];
  double* tile12 = reinterpret_cast<double*>(soLds);
  double* tile21 = reinterpret_cast<double*>(soLds + SO_LDS_TILE);
  SoState& S = *reinterpret_cast<SoState*>(soLds + 2 * SO_LDS_TILE);
  SoRec* recs = reinterpret_cast<SoRec*>(soLds + SO_LDS_FIXED);
  const int p = blockIdx.x, lane = lane_id();
  if (P.active && !P.active[p]) return;
  const orb_sim3_result_t* st = P.start + p;
  if (!st->has_sim3) return;
  const int s1 = P.kf1Slot ? P.kf1Slot[p] : p;
  const int s2 = P.kf2Slot ? P.kf2Slot[p] : p;
  const int n1 = min(max(P.nkeys[s1], 0), P.stride);
  const int n2 = min(max(P.nkeys[s2], 0), P.stride);
  const size_t pb = (size_t)p * P.stride, b1 = (size_t)s1 * P.stride, b2 = (size_t)s2 * P.stride;
  const orb_pose_t pose1 = P.pose[s1], pose2 = P.pose[s2];

  // ---- the pairs, in ascending i (:1183-1262)
  const unsigned long long ltMask = (1ull << lane) - 1ull;
  int E = 0;
  bool malformed = false;
  for (int c0 = 0; c0 < n1; c0 += ORB_WAVE) {  // (uniform trip count: whole waves ballot)
    const int i = c0 + lane;
    bool keep = false, bad = false;
    SoRec r;
    if (i < n1) {
      const int m2 = P.match12[pb + i];
      const int m1 = m2 >= 0 ? P.pointIndex[b1 + i] : -1;  // :1185, :1196
      if (m2 >= 0 && m1 >= 0 && !P.points[m1].bad && !P.points[m2].bad) {
        const int i2 = P.index2[pb + i];
        if (i2 >= 0) {  // :1198
          keep = true;
          if (i2 >= n2) {
            bad = true;
          } else {
            const orb_keypoint_t k1 = P.keys[b1 + i], k2 = P.keys[b2 + i2];
            bad = k1.octave < 0 || k1.octave >= P.nLevels || k2.octave < 0 || k2.octave >= P.nLevels;
            const float* w1 = P.points[m1].pos;
            const float* w2 = P.points[m2].pos;
#pragma unroll
            for (int k = 0; k < 3; ++k) {  // pin O1
              r.x1[k] = ((pose1.rcw[3 * k] * w1[0] + pose1.rcw[3 * k + 1] * w1[1]) +
                         pose1.rcw[3 * k + 2] * w1[2]) + pose1.tcw[k];
              r.x2[k] = ((pose2.rcw[3 * k] * w2[0] + pose2.rcw[3 * k + 1] * w2[1]) +
                         pose2.rcw[3 * k + 2] * w2[2]) + pose2.tcw[k];
            }
            r.o1[0] = k1.x;
            r.o1[1] = k1.y;
            r.o2[0] = k2.x;
            r.o2[1] = k2.y;
            r.inv1 = 0.0f;
            r.inv2 = 0.0f;
#pragma unroll
            for (int l = 0; l < ORB_MAX_LEVELS; ++l) {  // (static indices into the by-value parameters)
              if (k1.octave == l && l < P.nLevels) r.inv1 = P.invLevelSigma2[l];
              if (k2.octave == l && l < P.nLevels) r.inv2 = P.invLevelSigma2[l];
            }
            r.i1 = i;
            r.removed = 0;
          }
        }
      }
    }
    const unsigned long long kb = __ballot(keep);
    if (__ballot(bad)) malformed = true;
    if (keep && !bad) recs[E + __popcll(kb & ltMask)] = r;
    E += __popcll(kb);
  }
  __syncthreads();

  // g2oS12 = Sim3(toMatrix3d(R), toVector3d(t), s) (LoopClosing.cc, ComputeSim3)
  SoEst est;
  {
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (double)st->R[i];
    g2o_quat_from_matrix(R, est);
    est.tx = (double)st->t[0];
    est.ty = (double)st->t[1];
    est.tz = (double)st->t[2];
    est.s = (double)st->scale;
  }
  const SoEst est0 = est;
  if (malformed) {
    if (lane == 0) so_write_result(P.out + p, -1, 0, 0, 0, est0);
    return;
  }

  double K1[4], K2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    K1[k] = (double)P.k1[k];
    K2[k] = (double)P.k2[k];
  }
  const double th2 = (double)P.th2;
  const double delta = (double)(float)sqrt((double)P.th2);  // const float deltaHuber = sqrt(th2) (:1179)
  const bool fixScale = P.fixScale != 0;

  SoEst last = est;  // where the edges' _error was last computed
  double x[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // BlockSolver::_x
  auto full_pass = [&] {
    so_setup<true>(est, fixScale, S);
    so_pass<true>(recs, E, K1, K2, delta, tile12, tile21, S);
  };
  auto trial_pass = [&](double* step) {
    if (fixScale) step[6] = 0;  // oplusImpl writes into the solver's array (pin O6)
    last = so_mul(so_exp(step), est);
    so_setup<false>(last, fixScale, S);
    so_pass<false>(recs, E, K1, K2, delta, tile12, tile21, S);
  };
  auto accept = [&] { est = last; };
  auto reject = [] {};
  int nBad = 0, nIn = 0;
  for (int round = 0; round < 2; ++round) {
    const int iters = round == 0 ? 5 : (nBad > 0 ? 10 : 5);  // :1266, :1289-1301
    if (E - nBad > 0)  // (optimize() returns at once without active vertices)
      g2o_lm_optimize<7>(S.acc, iters, x, full_pass, trial_pass, accept, reject);
    // ---- the check (:1268-1287, :1303-1319): every remaining pair from the
    // errors of the last trial
    so_setup<false>(last, fixScale, S);
    int flagged = 0;
    for (int c0 = 0; c0 < E; c0 += ORB_WAVE) {
      const int e = c0 + lane;
      bool bad = false;
      if (e < E) {
        const SoRec r = recs[e];
        if (!r.removed) {
          double a0, a1, b0, b1;
          so_error(S.fwd[0], r.x2, r.o1, K1, a0, a1);
          so_error(S.inv[0], r.x1, r.o2, K2, b0, b1);
          const double sa = (double)r.inv1, sb = (double)r.inv2;
          const double c12 = a0 * (sa * a0) + a1 * (sa * a1);
          const double c21 = b0 * (sb * b0) + b1 * (sb * b1);
          bad = c12 > th2 || c21 > th2;
          if (bad) {
            recs[e].removed = 1;
            P.match12[pb + r.i1] = -1;
          }
        }
      }
      flagged += __popcll(__ballot(bad));
    }
    __syncthreads();
    if (round == 0) {
      nBad = flagged;
      if (E - nBad < 10) {  // :1295-1296: g2oS12 keeps the start value
        if (lane == 0) so_write_result(P.out + p, 0, E, nBad, 0, est0);
        return;
      }
    } else {
      nIn = (E - nBad) - flagged;
    }
  }
  if (lane == 0) so_write_result(P.out + p, 0, E, nBad, nIn, est);
}

__global__ __launch_bounds__(256) void k_pinned_exp(int n, const double* __restrict__ x,
                                                    double* __restrict__ y) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = pinned_exp(x[i]);
}

extern "C" int orb_k_sim3opt_max_stride(void) {
  return (int)((ORB_LDS_PER_CU - SO_LDS_FIXED) / sizeof(SoRec));
}

extern "C" hipError_t orb_k_optimize_sim3(const Sim3OptParams* params, hipStream_t s) {
  const Sim3OptParams P = *params;
  if (P.nProblems <= 0) return hipSuccess;
  if (P.stride <= 0 || P.stride > orb_k_sim3opt_max_stride()) return hipErrorInvalidValue;
  const size_t lds = SO_LDS_FIXED + (size_t)P.stride * sizeof(SoRec);
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute((const void*)k_optimize_sim3,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_optimize_sim3, dim3(P.nProblems), dim3(64), lds, s, P);
  return hipGetLastError();
}

extern "C" hipError_t orb_k_pinned_exp(int n, const double* x, double* y, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pinned_exp, dim3((n + 255) / 256), dim3(256), 0, s, n, x, y);
  return hipGetLastError();
}
