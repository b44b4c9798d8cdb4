// g2o_device.h -- the g2o and Eigen pieces that pose_kernels.hip
// and sim3opt_kernels.hip (§4.12) both reach, restated literally once;
// tests/poseopt_ref.py is the same text in numpy, and the bit-for-bit tests pin
// the order of every expression.  Every lane runs the same doubles, with every
// branch condition read from lane 0 (`uni`): the control flow is wave-uniform.
// Compiled with -ffp-contract=off: every expression evaluates as written.
#pragma once
#include "orb_device.h"

__device__ __forceinline__ bool uni(bool c) {  // a condition every lane computed alike, as a scalar
  return __builtin_amdgcn_readfirstlane((int)c) != 0;
}

// The rotation of an SE3Quat (_r) or a g2o::Sim3 (r): x, y, z, w
struct G2oQuat {
  double qx, qy, qz, qw;
};

// ---- Eigen closed forms (sums left to right)
// SE3Quat::normalizeRotation (se3quat.h:280-285).  g2o::Sim3 never normalises.
__device__ __forceinline__ void g2o_normalize_rotation(G2oQuat& e) {
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

// Quaterniond(Matrix3d): m row-major; never normalised here
__device__ __forceinline__ void g2o_quat_from_matrix(const double* m, G2oQuat& e) {
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
__device__ __forceinline__ void g2o_rotate(const G2oQuat& e, double x, double y, double z,
                                           double& rx, double& ry, double& rz) {
  double ux = e.qy * z - e.qz * y, uy = e.qz * x - e.qx * z, uz = e.qx * y - e.qy * x;
  ux = ux + ux;
  uy = uy + uy;
  uz = uz + uz;
  rx = (x + e.qw * ux) + (e.qy * uz - e.qz * uy);
  ry = (y + e.qw * uy) + (e.qz * ux - e.qx * uz);
  rz = (z + e.qw * uz) + (e.qx * uy - e.qy * ux);
}

// Quaterniond::toRotationMatrix: m row-major
__device__ __forceinline__ void g2o_to_matrix(const G2oQuat& e, double* m) {
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

// Eigen a * b of two quaternions
__device__ __forceinline__ void g2o_quat_mul(const G2oQuat& a, const G2oQuat& b, G2oQuat& r) {
  r.qx = ((a.qw * b.qx + a.qx * b.qw) + a.qy * b.qz) - a.qz * b.qy;
  r.qy = ((a.qw * b.qy + a.qy * b.qw) + a.qz * b.qx) - a.qx * b.qz;
  r.qz = ((a.qw * b.qz + a.qz * b.qw) + a.qx * b.qy) - a.qy * b.qx;
  r.qw = ((a.qw * b.qw - a.qx * b.qx) - a.qy * b.qy) - a.qz * b.qz;
}

// The head SE3Quat::exp (se3quat.h:223-257) and Sim3(const Vector7d&)
// (sim3.h:70-142) share: theta = |u[0..2]|, Om = skew(u[0..2]) (se3_ops.hpp:27-38),
// Om2 = Om Om, and R = (I + Om) + Om2 when theta < 0.00001, otherwise (I + (sn /
// theta) Om) + ((1 - cs) / theta^2) Om2.  Returns theta < 0.00001 (sn = cs = 0).
__device__ __forceinline__ bool g2o_rodrigues(const double* u, double& theta, double* Om,
                                              double* Om2, double* R, double& sn, double& cs) {
  const double o0 = u[0], o1 = u[1], o2 = u[2];
  theta = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
  const double eye[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  Om[0] = 0.0; Om[1] = -o2; Om[2] = o1;
  Om[3] = o2; Om[4] = 0.0; Om[5] = -o0;
  Om[6] = -o1; Om[7] = o0; Om[8] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      Om2[i * 3 + j] =
          (Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j]) + Om[i * 3 + 2] * Om[6 + j];
  const bool smallT = uni(theta < 0.00001);
  sn = cs = 0.0;
  if (smallT) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (eye[i] + Om[i]) + Om2[i];
  } else {
    pinned_sincos_d(theta, &sn, &cs);
    const double a = sn / theta, b = (1 - cs) / (theta * theta);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (eye[i] + a * Om[i]) + b * Om2[i];
  }
  return smallT;
}

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho[0], rho[1]
__device__ __forceinline__ void g2o_huber(double chi2, double delta, double& rho0, double& rho1) {
  const double dsqr = delta * delta;
  double r0 = chi2, r1 = 1.0;
  if (!(chi2 <= dsqr)) {
    const double sq = sqrt(chi2);
    r0 = (2 * sq) * delta - dsqr;
    r1 = delta / sq;
  }
  rho0 = r0;
  rho1 = r1;
}

// LinearSolverDense::solve (linear_solver_dense.h:104-112) with Eigen's
// unblocked LDLT on the lower triangle of H + lambda I.  `acc` holds the sums of
// a full pass: b is acc[1..N], H(r, c), c <= r, is acc[1 + N + r(r+1)/2 + c].
// Every lane runs it on its own registers: the loops are unrolled so that every
// index is static, and a data-dependent pivot row c is reached by a
// wave-uniform branch per candidate.  Returns isPositive(); x keeps its value
// when the factorisation reports a negative pivot.
#define G2O_SWAP(a, b) do { const double t_ = a; a = b; b = t_; } while (0)
template <int N>
__device__ __forceinline__ bool g2o_ldlt_solve(const double* acc, double lam, double* x) {
  double M[N][N];
#pragma unroll
  for (int r = 0; r < N; ++r)
#pragma unroll
    for (int c = 0; c <= r; ++c) M[r][c] = acc[1 + N + r * (r + 1) / 2 + c];
#pragma unroll
  for (int j = 0; j < N; ++j) M[j][j] = M[j][j] + lam;  // setLambda (block_solver.hpp:564-589)
  int tr[N];
  bool positive = true;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    int idx = k;
    double best = fabs(M[k][k]);
#pragma unroll
    for (int i = k + 1; i < N; ++i) {
      const double a = fabs(M[i][i]);
      if (a > best) {
        best = a;
        idx = i;
      }
    }
    idx = __builtin_amdgcn_readfirstlane(idx);
    tr[k] = idx;
#pragma unroll
    for (int c = k + 1; c < N; ++c) {
      if (idx == c) {
#pragma unroll
        for (int j = 0; j < k; ++j) G2O_SWAP(M[k][j], M[c][j]);
#pragma unroll
        for (int r = c + 1; r < N; ++r) G2O_SWAP(M[r][k], M[r][c]);
        G2O_SWAP(M[k][k], M[c][c]);
#pragma unroll
        for (int i = k + 1; i < c; ++i) G2O_SWAP(M[i][k], M[c][i]);
      }
    }
    if (k > 0) {
      double temp[N];
#pragma unroll
      for (int j = 0; j < k; ++j) temp[j] = M[j][j] * M[k][j];
#pragma unroll
      for (int i = k; i < N; ++i) {
        double s = M[i][0] * temp[0];
#pragma unroll
        for (int j = 1; j < k; ++j) s = s + M[i][j] * temp[j];
        M[i][k] = M[i][k] - s;
      }
    }
    const double akk = M[k][k];
    if (uni(fabs(akk) > 0.0)) {
#pragma unroll
      for (int i = k + 1; i < N; ++i) M[i][k] = M[i][k] / akk;
    }
    if (akk < 0.0) positive = false;
  }
  if (!uni(positive)) return false;
  double y[N];
#pragma unroll
  for (int j = 0; j < N; ++j) y[j] = acc[1 + j];  // b (its lanes add the negated terms)
#pragma unroll
  for (int k = 0; k < N; ++k)
#pragma unroll
    for (int c = k + 1; c < N; ++c)
      if (tr[k] == c) G2O_SWAP(y[k], y[c]);
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int r = i + 1; r < N; ++r) y[r] = y[r] - y[i] * M[r][i];
  const double tol = 1.0 / 1.7976931348623157e308;
#pragma unroll
  for (int i = 0; i < N; ++i) y[i] = fabs(M[i][i]) > tol ? y[i] / M[i][i] : 0.0;
#pragma unroll
  for (int i = N - 2; i >= 0; --i) {
    double s = M[i + 1][i] * y[i + 1];
#pragma unroll
    for (int j = i + 2; j < N; ++j) s = s + M[j][i] * y[j];
    y[i] = y[i] - s;
  }
#pragma unroll
  for (int k = N - 1; k >= 0; --k)
#pragma unroll
    for (int c = k + 1; c < N; ++c)
      if (tr[k] == c) G2O_SWAP(y[k], y[c]);
#pragma unroll
  for (int j = 0; j < N; ++j) x[j] = y[j];
  return true;
}
#undef G2O_SWAP

// OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp),
// once per iteration of optimize(iters), for one free vertex of N dimensions.
// acc holds the sums of the last pass as g2o_ldlt_solve reads them; x is
// BlockSolver::_x, kept across calls.  The kernel supplies
//   full_pass()    computeActiveErrors, activeRobustChi2 and buildSystem at the estimate
//   trial_pass(x)  oplus of the step x, then the robust chi2 there into acc[0]
//   accept()       the trial becomes the estimate (discardTop)
//   reject()       pop(): the vertex goes back, the edges keep their _error
// Every lane must call it.  At most iters x 10 trials whatever the input (NaN included).
template <int N, class Full, class Trial, class Accept, class Reject>
__device__ __forceinline__ void g2o_lm_optimize(const double* acc, int iters, double* x,
                                                Full full_pass, Trial trial_pass, Accept accept,
                                                Reject reject) {
  double lam = 0.0, ni = 2.0;
  int nbadSteps = 0;
  for (int i = 0; i < iters; ++i) {
    full_pass();
    double cur = acc[0];
    const double ini = cur;
    double bv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) bv[j] = acc[1 + j];
    if (i == 0) {  // computeLambdaInit (:166-180)
      double md = 0.0;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const double a = fabs(acc[1 + N + j * (j + 1) / 2 + j]);
        md = a < md ? md : a;  // std::max(fabs(h), maxDiagonal)
      }
      lam = 1e-5 * md;
      ni = 2.0;
      nbadSteps = 0;
    }
    double rho = 0.0;
    int qmax = 0;
    do {
      const bool ok2 = g2o_ldlt_solve<N>(acc, lam, x);
      trial_pass(x);
      double tmp = acc[0];
      __syncthreads();
      if (!ok2) tmp = 1.7976931348623157e308;
      double scale = 0.0;  // computeScale (:182-189)
#pragma unroll
      for (int j = 0; j < N; ++j) scale = scale + x[j] * (lam * x[j] + bv[j]);
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
        accept();
      } else {
        lam = lam * ni;
        ni = ni * 2;
        reject();
      }
      ++qmax;
    } while (uni(rho < 0 && qmax < 10));
    if (uni(qmax == 10 || rho == 0)) break;
    nbadSteps = uni((ini - cur) * 1e3 < ini) ? nbadSteps + 1 : 0;
    if (nbadSteps >= 3) break;
  }
}
