// pose_kernels.hip -- Optimizer::PoseOptimization (src/Optimizer.cc:243-477) on
// the device: the motion-only optimisation of one SE3 vertex against one unary
// edge per matched keypoint, with the g2o parts it reaches restated literally
// (tests/poseopt_ref.py is the same text in numpy).
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
//        Levenberg-Marquardt bookkeeping are the same doubles in every lane
//        (the sums reach the lanes through LDS), with every branch condition
//        read from lane 0, so the control flow is wave-uniform.
//   All four rounds and every trial run inside the kernel; the loops are
//   bounded by 4 x 10 x 10 trials whatever the input (NaN included).
//
// Compiled with -ffp-contract=off: every expression evaluates as written.
#include <hip/hip_runtime.h>

#include "orb_device.h"
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

struct PoEst {  // SE3Quat: _r (x, y, z, w), _t
  double qx, qy, qz, qw, tx, ty, tz;
};

__device__ __forceinline__ bool uni(bool c) {  // a condition every lane computed alike, as a scalar
  return __builtin_amdgcn_readfirstlane((int)c) != 0;
}

// ---- Eigen closed forms (sums left to right)
__device__ __forceinline__ void po_normalize_rotation(PoEst& e) {  // se3quat.h:280-285
  if (uni(e.qw < 0)) {
    e.qx = -e.qx;
    e.qy = -e.qy;
    e.qz = -e.qz;
    e.qw = -e.qw;
  }
  const double n = sqrt(((e.qx * e.qx + e.qy * e.qy) + e.qz * e.qz) + e.qw * e.qw);
  e.qx = e.qx / n;
  e.qy = e.qy / n;
  e.qz = e.qz / n;
  e.qw = e.qw / n;
}

// Quaterniond(Matrix3d): m row-major
__device__ __forceinline__ void po_quat_from_matrix(const double* m, PoEst& e) {
  double t = (m[0] + m[4]) + m[8];
  if (uni(t > 0.0)) {
    t = sqrt(t + 1.0);
    e.qw = 0.5 * t;
    t = 0.5 / t;
    e.qx = (m[7] - m[5]) * t;
    e.qy = (m[2] - m[6]) * t;
    e.qz = (m[3] - m[1]) * t;
    return;
  }
  int i = 0;
  double mii = m[0];
  if (m[4] > mii) {
    i = 1;
    mii = m[4];
  }
  if (m[8] > mii) i = 2;
  i = __builtin_amdgcn_readfirstlane(i);
  if (i == 0) {  // j = 1, k = 2
    t = sqrt(((m[0] - m[4]) - m[8]) + 1.0);
    e.qx = 0.5 * t;
    t = 0.5 / t;
    e.qw = (m[7] - m[5]) * t;
    e.qy = (m[3] + m[1]) * t;
    e.qz = (m[6] + m[2]) * t;
  } else if (i == 1) {  // j = 2, k = 0
    t = sqrt(((m[4] - m[8]) - m[0]) + 1.0);
    e.qy = 0.5 * t;
    t = 0.5 / t;
    e.qw = (m[2] - m[6]) * t;
    e.qz = (m[7] + m[5]) * t;
    e.qx = (m[1] + m[3]) * t;
  } else {  // j = 0, k = 1
    t = sqrt(((m[8] - m[0]) - m[4]) + 1.0);
    e.qz = 0.5 * t;
    t = 0.5 / t;
    e.qw = (m[3] - m[1]) * t;
    e.qx = (m[2] + m[6]) * t;
    e.qy = (m[5] + m[7]) * t;
  }
}

// Eigen q * v = v + w (2 q x v) + q x (2 q x v)
__device__ __forceinline__ void po_rotate(const PoEst& e, double x, double y, double z,
                                          double& rx, double& ry, double& rz) {
  double ux = e.qy * z - e.qz * y, uy = e.qz * x - e.qx * z, uz = e.qx * y - e.qy * x;
  ux = ux + ux;
  uy = uy + uy;
  uz = uz + uz;
  rx = (x + e.qw * ux) + (e.qy * uz - e.qz * uy);
  ry = (y + e.qw * uy) + (e.qz * ux - e.qx * uz);
  rz = (z + e.qw * uz) + (e.qx * uy - e.qy * ux);
}

__device__ __forceinline__ void po_to_matrix(const PoEst& e, double* m) {
  const double tx = 2.0 * e.qx, ty = 2.0 * e.qy, tz = 2.0 * e.qz;
  const double twx = tx * e.qw, twy = ty * e.qw, twz = tz * e.qw;
  const double txx = tx * e.qx, txy = ty * e.qx, txz = tz * e.qx;
  const double tyy = ty * e.qy, tyz = tz * e.qy, tzz = tz * e.qz;
  m[0] = 1.0 - (tyy + tzz);
  m[1] = txy - twz;
  m[2] = txz + twy;
  m[3] = txy + twz;
  m[4] = 1.0 - (txx + tzz);
  m[5] = tyz - twx;
  m[6] = txz - twy;
  m[7] = tyz + twx;
  m[8] = 1.0 - (txx + tyy);
}

// SE3Quat::exp (se3quat.h:223-257)
__device__ __forceinline__ PoEst po_exp(const double* u) {
  const double o0 = u[0], o1 = u[1], o2 = u[2];
  const double theta = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
  const double Om[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};  // se3_ops.hpp:27-38
  const double eye[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  double Om2[9], R[9], V[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      Om2[i * 3 + j] =
          (Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j]) + Om[i * 3 + 2] * Om[6 + j];
  if (uni(theta < 0.00001)) {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      R[i] = (eye[i] + Om[i]) + Om2[i];
      V[i] = R[i];
    }
  } else {
    double s, c;
    pinned_sincos_d(theta, &s, &c);
    const double a = s / theta, b = (1.0 - c) / (theta * theta);
    const double d = (theta - s) / ((theta * theta) * theta);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      R[i] = (eye[i] + a * Om[i]) + b * Om2[i];
      V[i] = (eye[i] + b * Om[i]) + d * Om2[i];
    }
  }
  PoEst e;
  po_quat_from_matrix(R, e);
  po_normalize_rotation(e);
  e.tx = (V[0] * u[3] + V[1] * u[4]) + V[2] * u[5];
  e.ty = (V[3] * u[3] + V[4] * u[4]) + V[5] * u[5];
  e.tz = (V[6] * u[3] + V[7] * u[4]) + V[8] * u[5];
  return e;
}

// SE3Quat::operator* (se3quat.h:104-110)
__device__ __forceinline__ PoEst po_mul(const PoEst& a, const PoEst& b) {
  PoEst r;
  double rx, ry, rz;
  po_rotate(a, b.tx, b.ty, b.tz, rx, ry, rz);
  r.tx = a.tx + rx;
  r.ty = a.ty + ry;
  r.tz = a.tz + rz;
  r.qx = ((a.qw * b.qx + a.qx * b.qw) + a.qy * b.qz) - a.qz * b.qy;
  r.qy = ((a.qw * b.qy + a.qy * b.qw) + a.qz * b.qx) - a.qx * b.qz;
  r.qz = ((a.qw * b.qz + a.qz * b.qw) + a.qx * b.qy) - a.qy * b.qx;
  r.qw = ((a.qw * b.qw - a.qx * b.qx) - a.qy * b.qy) - a.qz * b.qz;
  po_normalize_rotation(r);
  return r;
}

// LinearSolverDense::solve (linear_solver_dense.h:104-112) with Eigen's
// unblocked LDLT on the lower triangle of H + lambda I.  H is S.acc[7..], b is
// S.acc[1..6].  Every lane runs it on its own registers: the loops are unrolled
// so that every index is static, and a data-dependent pivot row c is reached by
// a wave-uniform branch per candidate.  Returns isPositive(); x keeps its
// value when the factorisation reports a negative pivot.
#define PO_SWAP(a, b)     \
  do {                    \
    const double t_ = a;  \
    a = b;                \
    b = t_;               \
  } while (0)
__device__ __forceinline__ bool po_ldlt_solve(const PoState& S, double lam, double* x) {
  double M[6][6];
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c <= r; ++c) M[r][c] = S.acc[7 + r * (r + 1) / 2 + c];
#pragma unroll
  for (int j = 0; j < 6; ++j) M[j][j] = M[j][j] + lam;  // setLambda (block_solver.hpp:564-589)
  int tr[6];
  bool positive = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    int idx = k;
    double best = fabs(M[k][k]);
#pragma unroll
    for (int i = k + 1; i < 6; ++i) {
      const double a = fabs(M[i][i]);
      if (a > best) {
        best = a;
        idx = i;
      }
    }
    idx = __builtin_amdgcn_readfirstlane(idx);
    tr[k] = idx;
#pragma unroll
    for (int c = k + 1; c < 6; ++c) {
      if (idx == c) {
#pragma unroll
        for (int j = 0; j < k; ++j) PO_SWAP(M[k][j], M[c][j]);
#pragma unroll
        for (int r = c + 1; r < 6; ++r) PO_SWAP(M[r][k], M[r][c]);
        PO_SWAP(M[k][k], M[c][c]);
#pragma unroll
        for (int i = k + 1; i < c; ++i) PO_SWAP(M[i][k], M[c][i]);
      }
    }
    if (k > 0) {
      double temp[6];
#pragma unroll
      for (int j = 0; j < k; ++j) temp[j] = M[j][j] * M[k][j];
#pragma unroll
      for (int i = k; i < 6; ++i) {
        double s = M[i][0] * temp[0];
#pragma unroll
        for (int j = 1; j < k; ++j) s = s + M[i][j] * temp[j];
        M[i][k] = M[i][k] - s;
      }
    }
    const double akk = M[k][k];
    if (uni(fabs(akk) > 0.0)) {
#pragma unroll
      for (int i = k + 1; i < 6; ++i) M[i][k] = M[i][k] / akk;
    }
    if (akk < 0.0) positive = false;
  }
  if (!uni(positive)) return false;
  double y[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) y[j] = S.acc[1 + j];  // b (its lanes add the negated terms)
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int c = k + 1; c < 6; ++c)
      if (tr[k] == c) PO_SWAP(y[k], y[c]);
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int r = i + 1; r < 6; ++r) y[r] = y[r] - y[i] * M[r][i];
  const double tol = 1.0 / 1.7976931348623157e308;
#pragma unroll
  for (int i = 0; i < 6; ++i) y[i] = fabs(M[i][i]) > tol ? y[i] / M[i][i] : 0.0;
#pragma unroll
  for (int i = 4; i >= 0; --i) {
    double s = M[i + 1][i] * y[i + 1];
#pragma unroll
    for (int j = i + 2; j < 6; ++j) s = s + M[j][i] * y[j];
    y[i] = y[i] - s;
  }
#pragma unroll
  for (int k = 5; k >= 0; --k)
#pragma unroll
    for (int c = k + 1; c < 6; ++c)
      if (tr[k] == c) PO_SWAP(y[k], y[c]);
#pragma unroll
  for (int j = 0; j < 6; ++j) x[j] = y[j];
  return true;
}
#undef PO_SWAP

struct PoCam {
  double fx, fy, cx, cy, bf;
};

// computeError of one edge (types_six_dof_expmap.h:153-157, :184-188) with
// both cam_project forms (.cpp:290-306); returns chi2 (base_edge.h) and the
// mapped point.
__device__ __forceinline__ double po_error(const PoEdge& r, bool stereo, const PoEst& est,
                                           const PoCam& cam, double& x, double& y, double& z,
                                           double& e0, double& e1, double& e2) {
  po_rotate(est, (double)r.X[0], (double)r.X[1], (double)r.X[2], x, y, z);
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
        // RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91)
        double rho0 = chi2, rho1 = 1.0;
        if (robust) {
          const double delta = stereo ? deltaStereo : deltaMono, dsqr = delta * delta;
          if (!(chi2 <= dsqr)) {
            const double sq = sqrt(chi2);
            rho0 = (2 * sq) * delta - dsqr;
            rho1 = delta / sq;
          }
        }
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
    po_quat_from_matrix(R, est0);
    po_normalize_rotation(est0);
    est0.tx = (double)pin.tcw[0];
    est0.ty = (double)pin.tcw[1];
    est0.tz = (double)pin.tcw[2];
  }
  PoEst est = est0, last = est0;
  double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // BlockSolver::_x
  bool robust = true;
  int nBad = 0, lmIters = 0, rejected = 0;
  for (int it = 0; it < 4; ++it) {
    est = est0;  // :397
    last = est0;
    bool lastIsEst = true;
    if (E - nBad > 0) {  // (optimize() returns at once without active vertices)
      double lam = 0.0, ni = 2.0;
      int nbadSteps = 0;
      for (int i = 0; i < 10; ++i) {  // optimize(10): OptimizationAlgorithmLevenberg::solve
        ++lmIters;
        po_pass<true>(recs, E, est, cam, robust, deltaMono, deltaStereo, tile, S);
        double cur = S.acc[0];
        const double ini = cur;
        double bv[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) bv[j] = S.acc[1 + j];
        if (i == 0) {  // computeLambdaInit (:166-180)
          double md = 0.0;
#pragma unroll
          for (int j = 0; j < 6; ++j) {
            const double a = fabs(S.acc[7 + j * (j + 1) / 2 + j]);
            md = a < md ? md : a;  // std::max(fabs(h), maxDiagonal)
          }
          lam = 1e-5 * md;
          ni = 2.0;
          nbadSteps = 0;
        }
        double rho = 0.0;
        int qmax = 0;
        bool again;
        do {
          const bool ok2 = po_ldlt_solve(S, lam, x);
          const PoEst trial = po_mul(po_exp(x), est);  // oplusImpl (.h:73-76)
          po_pass<false>(recs, E, trial, cam, robust, deltaMono, deltaStereo, tile, S);
          last = trial;
          double tmp = S.acc[0];
          __syncthreads();
          if (!ok2) tmp = 1.7976931348623157e308;
          double scale = 0.0;  // computeScale (:182-189)
#pragma unroll
          for (int j = 0; j < 6; ++j) scale = scale + x[j] * (lam * x[j] + bv[j]);
          scale = scale + 1e-3;
          rho = (cur - tmp) / scale;
          if (uni(rho > 0 && fabs(tmp) <= 1.7976931348623157e308)) {  // g2o_isfinite
            const double y = 2 * rho - 1;
            double alpha = 1.0 - (y * y) * y;
            alpha = (2.0 / 3.0) < alpha ? (2.0 / 3.0) : alpha;          // std::min(alpha, upper)
            const double sf = (1.0 / 3.0) < alpha ? alpha : (1.0 / 3.0);  // std::max(lower, alpha)
            lam = lam * sf;
            ni = 2.0;
            cur = tmp;
            est = trial;
            lastIsEst = true;
          } else {
            lam = lam * ni;
            ni = ni * 2;
            ++rejected;  // pop(): the vertex goes back, the edges keep their _error
            lastIsEst = false;
          }
          ++qmax;
          again = uni(rho < 0 && qmax < 10);
        } while (again);
        if (uni(qmax == 10 || rho == 0)) break;
        if (uni((ini - cur) * 1e3 < ini))
          ++nbadSteps;
        else
          nbadSteps = 0;
        if (nbadSteps >= 3) break;
      }
    }
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
    po_to_matrix(est, R);
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
