// sim3_kernels.hip -- Sim3Solver (src/Sim3Solver.cc, include/Sim3Solver.h) as
// a device-resident batch for LoopClosing::ComputeSim3: the constructor with
// SetRansacParameters (:37-141) and iterate / find (:144-220) with ComputeSim3
// (:237-351), CheckInliers (:354-378) and Project (:396-417).
//
// k_sim3_setup: one workgroup per problem.  Pass 1 evaluates the reference's
//   skips per i1 and looks for a malformed kept correspondence (block OR);
//   pass 2 compacts the kept ones in ascending i1 (block scan of the keep flags
//   per trip of SIM3_T) and writes their records; one thread evaluates
//   SetRansacParameters.
// k_sim3_iterate: one workgroup per problem.
//   stage    the records' twelve floats go to LDS once, field-major
//   chunk    the call's window of iterations is taken SIM3_CHUNK hypotheses at
//            a time; a wave per hypothesis evaluates its three draws and solves
//            Horn wave-uniformly (every lane the same double chain, the 4 x 4
//            Jacobi on a per-wave LDS workspace), then its lanes stride over
//            the correspondences; the inlier masks are ballots kept in LDS
//            with the count and the transform
//   replay   one lane replays the acceptance rule (:190-207) over the chunk's
//            counts in iteration order; a taken best is copied to the best row
//   Work past a return is wasted, never visible.  The state depends on the
//   replay alone, so it is the same however the iterations are split in calls.
// The pin list is in include/orb_abi.h (P1..P16).
#include <algorithm>

#include "orb_device.h"
#include "orb_kernels.h"

#ifndef SIM3_T
#define SIM3_T 512       // threads per workgroup, both kernels (README: compile-time macros)
#endif
#ifndef SIM3_CHUNK
#define SIM3_CHUNK 8     // hypotheses evaluated side by side before the rule is replayed
#endif
#define SIM3_NW (SIM3_T / 64)
#define SIM3_FIELDS 12   // x1[3] x2[3] p1[2] p2[2] max_err1 max_err2
#define SIM3_HYP_WORDS 32  // per hypothesis: s, R[9], t[3], T12[16], count, bad, pad
#define SIM3_JAC_WORDS 48  // per wave: A[16], V[16], W[4], indR[4], indC[4], pad
static_assert(SIM3_T % 64 == 0 && SIM3_T >= 64 && SIM3_T <= 1024, "whole waves");
static_assert(SIM3_CHUNK >= 1 && SIM3_CHUNK <= 32, "chunk length");
static_assert(sizeof(orb_sim3_corr_t) == 56 && sizeof(orb_sim3_state_t) == 184 &&
              sizeof(orb_sim3_result_t) == 132, "ABI records");

// what a workgroup keeps beside the per-slot part (all of it in the dynamic region)
#define SIM3_FIXED_LDS ((size_t)8192)
static_assert(4 * (SIM3_CHUNK * SIM3_HYP_WORDS + SIM3_NW * SIM3_JAC_WORDS + 64) <= SIM3_FIXED_LDS,
              "capacity rule counts these");

static __host__ __device__ inline size_t sim3_s64(int stride) {
  return ((size_t)stride + 63) & ~(size_t)63;
}
// dynamic LDS of one k_sim3_iterate workgroup at `stride` slots
static size_t sim3_iter_lds(int stride) {
  const size_t S = sim3_s64(stride);
  return 4 * SIM3_FIELDS * S + (SIM3_CHUNK + 1) * (S / 8) + SIM3_FIXED_LDS;
}

// --------------------------------------------------------------------- pins
// P9: pinned_atan / pinned_atan2 (fdlibm's s_atan.c / e_atan2.c) are in orb_device.h

// P7's hypot
__device__ __forceinline__ float sim3_hypot(float a, float b) {
  return (float)__builtin_sqrt((double)a * (double)a + (double)b * (double)b);
}

// P7: cv::eigen on a symmetric 4 x 4 float matrix (JacobiImpl_<float>), on a
// per-wave LDS workspace: every lane runs the same chain on the same words.
// ws: A[16], V[16], W[4], then indR[4], indC[4] as ints.  Eigenvalues
// descending in W, eigenvectors as the rows of V.
__device__ __forceinline__ void sim3_jacobi4(float* ws) {
  float* A = ws;
  float* V = ws + 16;
  float* W = ws + 32;
  int* indR = (int*)(ws + 36);
  int* indC = (int*)(ws + 40);
  const int n = 4;
  const float eps = 1.1920928955078125e-07f;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) V[i * 4 + j] = i == j ? 1.f : 0.f;
  for (int k = 0; k < n; ++k) {
    W[k] = A[5 * k];
    if (k < n - 1) {
      int m = k + 1;
      float mv = fabsf(A[4 * k + m]);
      for (int i = k + 2; i < n; ++i) {
        const float val = fabsf(A[4 * k + i]);
        if (mv < val) mv = val, m = i;
      }
      indR[k] = m;
    }
    if (k > 0) {
      int m = 0;
      float mv = fabsf(A[k]);
      for (int i = 1; i < k; ++i) {
        const float val = fabsf(A[4 * i + k]);
        if (mv < val) mv = val, m = i;
      }
      indC[k] = m;
    }
  }
  for (int iters = 0; iters < n * n * 30; ++iters) {
    int k = 0;
    float mv = fabsf(A[indR[0]]);
    for (int i = 1; i < n - 1; ++i) {
      const float val = fabsf(A[4 * i + indR[i]]);
      if (mv < val) mv = val, k = i;
    }
    int l = indR[k];
    for (int i = 1; i < n; ++i) {
      const float val = fabsf(A[4 * indC[i] + i]);
      if (mv < val) mv = val, k = indC[i], l = i;
    }
    const float p = A[4 * k + l];
    if (fabsf(p) <= eps) break;
    const float y = (float)((double)(W[l] - W[k]) * 0.5);
    float t = fabsf(y) + sim3_hypot(p, y);
    float s = sim3_hypot(p, t);
    const float c = t / s;
    s = p / s;
    t = (p / t) * p;
    if (y < 0) s = -s, t = -t;
    A[4 * k + l] = 0;
    W[k] = W[k] - t;
    W[l] = W[l] + t;
#define SIM3_ROTATE(i0, i1)                  \
  do {                                       \
    const float a0 = A[i0], b0 = A[i1];      \
    A[i0] = a0 * c - b0 * s;                 \
    A[i1] = a0 * s + b0 * c;                 \
  } while (0)
    for (int i = 0; i < k; ++i) SIM3_ROTATE(4 * i + k, 4 * i + l);
    for (int i = k + 1; i < l; ++i) SIM3_ROTATE(4 * k + i, 4 * i + l);
    for (int i = l + 1; i < n; ++i) SIM3_ROTATE(4 * k + i, 4 * l + i);
#undef SIM3_ROTATE
    for (int i = 0; i < n; ++i) {
      const float a0 = V[4 * k + i], b0 = V[4 * l + i];
      V[4 * k + i] = a0 * c - b0 * s;
      V[4 * l + i] = a0 * s + b0 * c;
    }
    for (int j = 0; j < 2; ++j) {
      const int idx = j == 0 ? k : l;
      if (idx < n - 1) {
        int m = idx + 1;
        float mw = fabsf(A[4 * idx + m]);
        for (int i = idx + 2; i < n; ++i) {
          const float val = fabsf(A[4 * idx + i]);
          if (mw < val) mw = val, m = i;
        }
        indR[idx] = m;
      }
      if (idx > 0) {
        int m = 0;
        float mw = fabsf(A[idx]);
        for (int i = 1; i < idx; ++i) {
          const float val = fabsf(A[4 * i + idx]);
          if (mw < val) mw = val, m = i;
        }
        indC[idx] = m;
      }
    }
  }
  for (int k = 0; k < n - 1; ++k) {
    int m = k;
    for (int i = k + 1; i < n; ++i)
      if (W[m] < W[i]) m = i;
    if (k != m) {
      const float wk = W[k];
      W[k] = W[m];
      W[m] = wk;
      for (int i = 0; i < n; ++i) {
        const float a = V[4 * m + i];
        V[4 * m + i] = V[4 * k + i];
        V[4 * k + i] = a;
      }
    }
  }
}

// ComputeSim3 (:237-351) on P1 = columns a[0..2] (set 1), P2 = columns b[0..2]:
// out[0] = ms12i, out[1..9] = mR12i, out[10..12] = mt12i, out[13..28] = mT12i;
// t21[0..8] = sRinv, t21[9..11] = tinv (mT21i's rows 0..2).
__device__ __forceinline__ void sim3_horn(const float a[3][3], const float b[3][3], int fixScale,
                                          float* ws, float* out, float* t21) {
  // Step 1 (ComputeCentroid, P2 P3): a[i] is column i
  const float third = (float)(1.0 / 3.0);
  float O1[3], O2[3], Pr1[3][3], Pr2[3][3];  // Pr[row][col]
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    O1[r] = ((a[0][r] + a[2][r]) + a[1][r]) * third + 0.0f;
    O2[r] = ((b[0][r] + b[2][r]) + b[1][r]) * third + 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Pr1[r][c] = a[c][r] - O1[r];
      Pr2[r][c] = b[c][r] - O2[r];
    }
  }
  // Step 2 (P4): M = Pr2 * Pr1.t()
  float M[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) acc += (double)Pr2[i][k] * (double)Pr1[j][k];
      M[i][j] = (float)acc;
    }
  // Step 3 (P6)
  const float N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2],
              N14 = M[0][1] - M[1][0], N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0],
              N24 = M[2][0] + M[0][2], N33 = -M[0][0] + M[1][1] - M[2][2],
              N34 = M[1][2] + M[2][1], N44 = -M[0][0] - M[1][1] + M[2][2];
  ws[0] = N11, ws[1] = N12, ws[2] = N13, ws[3] = N14;
  ws[4] = N12, ws[5] = N22, ws[6] = N23, ws[7] = N24;
  ws[8] = N13, ws[9] = N23, ws[10] = N33, ws[11] = N34;
  ws[12] = N14, ws[13] = N24, ws[14] = N34, ws[15] = N44;
  // Step 4 (P7 P8 P9 P2 P10)
  sim3_jacobi4(ws);
  const float q0 = ws[16], q1 = ws[17], q2 = ws[18], q3 = ws[19];
  const double nrm = __builtin_sqrt(
      ((0.0 + (double)q1 * (double)q1) + (double)q2 * (double)q2) + (double)q3 * (double)q3);
  const double ang = pinned_atan2(nrm, (double)q0);
  const float sc = (float)((2.0 * ang) * (1.0 / nrm));
  const double rx0 = (double)(q1 * sc + 0.0f), ry0 = (double)(q2 * sc + 0.0f),
               rz0 = (double)(q3 * sc + 0.0f);
  const double theta = __builtin_sqrt((rx0 * rx0 + ry0 * ry0) + rz0 * rz0);
  float R[9];
  {
    double sn, cs;
    pinned_sincos_d(theta, &sn, &cs);
    const double c1 = 1.0 - cs, itheta = 1.0 / theta;
    const double r[3] = {rx0 * itheta, ry0 * itheta, rz0 * itheta};
    const double rxm[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
    const bool ident = theta < 2.2204460492503131e-16;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double e = i == j ? 1.0 : 0.0;
        const double v = (cs * e + c1 * (r[i] * r[j])) + sn * rxm[3 * i + j];
        R[3 * i + j] = ident ? (float)e : (float)v;
      }
  }
  // Step 5 (P5): P3 = R * Pr2; Step 6 (P11 P12)
  float s12 = 1.0f;
  {
    float P3[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        P3[i][j] = (R[3 * i] * Pr2[0][j] + R[3 * i + 1] * Pr2[1][j]) + R[3 * i + 2] * Pr2[2][j];
    double pr[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) pr[i] = (double)Pr1[i / 3][i % 3] * (double)P3[i / 3][i % 3];
    double nom = 0.0;
    nom += ((pr[0] + pr[1]) + pr[2]) + pr[3];
    nom += ((pr[4] + pr[5]) + pr[6]) + pr[7];
    nom += pr[8];
    double den = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) den += (double)(P3[i / 3][i % 3] * P3[i / 3][i % 3]);
    if (!fixScale) s12 = (float)(nom / den);
  }
  // Step 7 (P13), Step 8 (P2 P14)
  out[0] = s12;
#pragma unroll
  for (int i = 0; i < 9; ++i) out[1 + i] = R[i];
  float t[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float u = (R[3 * k] * O2[0] + R[3 * k + 1] * O2[1]) + R[3 * k + 2] * O2[2];
    t[k] = (float)((double)u * -(double)s12 + (double)O1[k]);
    out[10 + k] = t[k];
  }
  const float sinv = (float)(1.0 / (double)s12);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      out[13 + 4 * i + j] = R[3 * i + j] * s12 + 0.0f;
      t21[3 * i + j] = R[3 * j + i] * sinv + 0.0f;
    }
    out[13 + 4 * i + 3] = t[i];
    out[13 + 12 + i] = 0.f;
  }
  out[13 + 15] = 1.f;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    t21[9 + k] = 0.0f - ((t21[3 * k] * t[0] + t21[3 * k + 1] * t[1]) + t21[3 * k + 2] * t[2]);
}

// Project (:396-417) of one point (P1)
__device__ __forceinline__ void sim3_project(const float* Rm, int rs, const float* tv, float x,
                                             float y, float z, const float* K, float* u, float* v) {
  const float cx_ = ((Rm[0] * x + Rm[1] * y) + Rm[2] * z) + tv[0];
  const float cy_ = ((Rm[rs] * x + Rm[rs + 1] * y) + Rm[rs + 2] * z) + tv[1];
  const float cz_ = ((Rm[2 * rs] * x + Rm[2 * rs + 1] * y) + Rm[2 * rs + 2] * z) + tv[2];
  const float invz = 1.0f / cz_;
  const float px = cx_ * invz, py = cy_ * invz;
  *u = K[0] * px + K[2];
  *v = K[1] * py + K[3];
}

// ------------------------------------------------------------- k_sim3_setup
// the reference's skips for i1 (:64-79), then the malformed checks
// returns 1 kept, 0 skipped; *bad set when a kept one is malformed
__device__ __forceinline__ int sim3_keep(const Sim3SetupParams& P, int p, int i1, int s1, int s2,
                                         int n1, int n2, int* ik1, int* ik2, int* pm1, int* pm2,
                                         int* bad) {
  const size_t pb = (size_t)p * P.stride;
  const int m2 = P.match12[pb + i1];
  if (m2 < 0) return 0;  // vpMatched12[i1] NULL
  const int m1 = P.pointIndex[(size_t)s1 * P.stride + i1];
  if (m1 < 0) return 0;  // pMP1 NULL
  if (P.points[m1].bad || P.points[m2].bad) return 0;
  const int k1 = P.index1 ? P.index1[pb + i1] : i1;
  const int k2 = P.index2[pb + i1];
  if (k1 < 0 || k2 < 0) return 0;
  *ik1 = k1, *ik2 = k2, *pm1 = m1, *pm2 = m2;
  if (k1 >= n1 || k2 >= n2) {
    *bad = 1;
    return 1;
  }
  const int o1 = P.keys[(size_t)s1 * P.stride + k1].octave;
  const int o2 = P.keys[(size_t)s2 * P.stride + k2].octave;
  if (o1 < 0 || o1 >= P.nLevels || o2 < 0 || o2 >= P.nLevels) *bad = 1;
  return 1;
}

__global__ __launch_bounds__(SIM3_T) void k_sim3_setup(Sim3SetupParams P) {
  __shared__ int scan[20];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int s1 = P.kf1Slot ? P.kf1Slot[p] : p;
  const int s2 = P.kf2Slot ? P.kf2Slot[p] : p;
  const int n1 = min(max(P.nkeys[s1], 0), P.stride);
  const int n2 = min(max(P.nkeys[s2], 0), P.stride);
  orb_sim3_state_t* st = P.state + p;
  orb_sim3_corr_t* C = P.corr + (size_t)p * P.stride;
  int ik1 = 0, ik2 = 0, pm1 = 0, pm2 = 0;

  int bad = 0;
  for (int i1 = tid; i1 < n1; i1 += SIM3_T)
    sim3_keep(P, p, i1, s1, s2, n1, n2, &ik1, &ik2, &pm1, &pm2, &bad);
  bad = __syncthreads_or(bad);

  int N = 0;
  if (!bad) {
    const orb_pose_t pose1 = P.pose[s1], pose2 = P.pose[s2];
    for (int base = 0; base < n1; base += SIM3_T) {  // uniform trip count
      const int i1 = base + tid;
      int dummy = 0;
      const int keep =
          i1 < n1 ? sim3_keep(P, p, i1, s1, s2, n1, n2, &ik1, &ik2, &pm1, &pm2, &dummy) : 0;
      int total;
      const int pos = N + block_excl_scan(keep, scan, &total);
      N += total;
      if (keep) {
        const int o1 = P.keys[(size_t)s1 * P.stride + ik1].octave;
        const int o2 = P.keys[(size_t)s2 * P.stride + ik2].octave;
        const float* w1 = P.points[pm1].pos;
        const float* w2 = P.points[pm2].pos;
        orb_sim3_corr_t c;
        c.index1 = i1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          c.x1[k] = ((pose1.rcw[3 * k] * w1[0] + pose1.rcw[3 * k + 1] * w1[1]) +
                     pose1.rcw[3 * k + 2] * w1[2]) + pose1.tcw[k];
          c.x2[k] = ((pose2.rcw[3 * k] * w2[0] + pose2.rcw[3 * k + 1] * w2[1]) +
                     pose2.rcw[3 * k + 2] * w2[2]) + pose2.tcw[k];
        }
        {  // FromCameraToImage (:419-437)
          const float invz = 1.0f / c.x1[2];
          const float x = c.x1[0] * invz, y = c.x1[1] * invz;
          c.p1[0] = P.k1[0] * x + P.k1[2];
          c.p1[1] = P.k1[1] * y + P.k1[3];
        }
        {
          const float invz = 1.0f / c.x2[2];
          const float x = c.x2[0] * invz, y = c.x2[1] * invz;
          c.p2[0] = P.k2[0] * x + P.k2[2];
          c.p2[1] = P.k2[1] * y + P.k2[3];
        }
        c.max_err1 = P.maxErr[o1];
        c.max_err2 = P.maxErr[o2];
        c.best_inlier = 0;
        c._pad[0] = c._pad[1] = c._pad[2] = 0;
        C[pos] = c;
      }
    }
  }

  if (tid == 0) {
    orb_sim3_state_t s;
    memset(&s, 0, sizeof(s));
    s.n1 = n1;
    if (bad) {
      s.status = -1;
    } else {
      s.n = N;
      s.min_inliers = P.minInliers;
      s.fix_scale = P.fixScale;
#pragma unroll
      for (int k = 0; k < 4; ++k) s.k1[k] = P.k1[k], s.k2[k] = P.k2[k];
      // SetRansacParameters (:117-141)
      int its = 0;
      if (N >= P.minInliers) {
        int nIt;
        if (P.minInliers == N) {
          nIt = 1;
        } else {
          const float epsilon = (float)P.minInliers / (float)N;
          const double e = (double)epsilon;
          const double q =
              __builtin_ceil(pinned_log(1.0 - P.probability) / pinned_log(1.0 - (e * e) * e));
          nIt = q >= (double)P.maxIterations ? P.maxIterations : (int)q;
        }
        its = max(1, min(nIt, P.maxIterations));
      }
      s.max_its = its;
    }
    *st = s;
  }
}

// ----------------------------------------------------------- k_sim3_iterate
// vAvailableIndices after the swap-with-back removals (:175-183): position
// `pos` of a list that started as 0..N-1 and had `nmod` entries overwritten
__device__ __forceinline__ int sim3_avail(int pos, const int* mpos, const int* mval, int nmod) {
  int v = pos;
  for (int i = 0; i < nmod; ++i)
    if (mpos[i] == pos) v = mval[i];  // the latest write wins
  return v;
}

__global__ __launch_bounds__(SIM3_T) void k_sim3_iterate(Sim3IterParams P) {
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (P.active && !P.active[p]) return;
  const int S = (int)sim3_s64(P.stride), Wn = S >> 6;
  float* F = (float*)dyn;                                              // SIM3_FIELDS x S
  unsigned long long* bits = (unsigned long long*)(F + SIM3_FIELDS * S);  // SIM3_CHUNK x Wn
  unsigned long long* bestBits = bits + (size_t)SIM3_CHUNK * Wn;          // Wn
  float* hyp = (float*)(bestBits + Wn);                   // SIM3_CHUNK x SIM3_HYP_WORDS
  float* jac = hyp + SIM3_CHUNK * SIM3_HYP_WORDS;         // SIM3_NW x SIM3_JAC_WORDS
  int* ctl = (int*)(jac + SIM3_NW * SIM3_JAC_WORDS);      // 64 ints

  orb_sim3_state_t* st = P.state + p;
  orb_sim3_corr_t* C = P.corr + (size_t)p * P.stride;
  uint8_t* IN = P.inliers12 + (size_t)p * P.stride;
  orb_sim3_result_t* res = P.result + p;
  const uint32_t* D = P.draws + (size_t)p * (size_t)P.drawStride;

  const int status = st->status;
  const int n1 = min(max(st->n1, 0), P.stride);
  const int N = min(max(st->n, 0), P.stride);
  const int minInl = st->min_inliers;
  const int maxIts = min(max(st->max_its, 0), P.maxIterations);
  const int it0 = max(st->iterations, 0);
  const int fixScale = st->fix_scale;
  float K1[4], K2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) K1[k] = st->k1[k], K2[k] = st->k2[k];

  // vbInliers = vector<bool>(mN1, false) (:148)
  for (int i = tid; i < n1; i += SIM3_T) IN[i] = 0;

  if (status < 0 || N < minInl || N < 3) {  // :151-156 (and a malformed problem)
    if (tid == 0) {
      orb_sim3_result_t r;
      memset(&r, 0, sizeof(r));
      r.no_more = 1;
      *res = r;
    }
    return;
  }

  // stage the records field-major: word f of record i -> F[(f - 1) * S + i]
  {
    const uint32_t* cw = (const uint32_t*)C;
    const int nw = N * 14;
    for (int d = tid; d < nw; d += SIM3_T) {
      const int rec = d / 14, f = d - rec * 14;
      if (f >= 1 && f <= SIM3_FIELDS) dyn[(f - 1) * S + rec] = cw[d];
    }
  }
  if (tid == 0) {
    ctl[0] = st->best_inliers;  // mnBestInliers
    ctl[1] = 0;                 // stop: 1 success, 2 malformed draw
    ctl[2] = -1;                // the chunk's hypothesis taken as best
    ctl[3] = 0;                 // iterations run
    ctl[4] = 0;                 // the best changed in this call
    ctl[5] = st->best_iteration;
    ctl[6] = 0;                 // nInliers of the success
  }
  __syncthreads();

  const int window = max(min(P.nIterations, maxIts - it0), 0);
  const int trips = (N + 63) >> 6;
  float* best = (float*)(ctl + 16);  // 29 words: s, R, t, T12 of the best taken in this call

  for (int c0 = 0; c0 < window; c0 += SIM3_CHUNK) {
    const int nh = min(SIM3_CHUNK, window - c0);
    for (int h = wave; h < nh; h += SIM3_NW) {
      const int it = it0 + c0 + h;
      // the three draws (:173-184), wave-uniform
      int idx[3], mpos[2], mval[2], badDraw = 0;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const uint32_t r = D[3 * it + j];
        badDraw |= r > P.randMax;
        const int size = N - j;
        int randi = (int)(((double)r / ((double)P.randMax + 1.0)) * (double)size);
        randi = min(max(randi, 0), size - 1);  // r <= rand_max keeps it there already
        idx[j] = sim3_avail(randi, mpos, mval, j);
        if (j < 2) {
          mval[j] = sim3_avail(size - 1, mpos, mval, j);
          mpos[j] = randi;
        }
      }
      float a[3][3], b[3][3];
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          a[j][k] = F[k * S + idx[j]];
          b[j][k] = F[(3 + k) * S + idx[j]];
        }
      float out[29], t21[12];
      sim3_horn(a, b, fixScale, jac + wave * SIM3_JAC_WORDS, out, t21);
      // CheckInliers (:354-378), a correspondence per lane
      int cnt = 0;
      for (int tr = 0; tr < trips; ++tr) {
        const int i = (tr << 6) + lane;
        int inl = 0;
        if (i < N) {
          float u, v;
          // vP2im1 = Project(mvX3Dc2, mT12i, mK1)
          const float x2 = F[3 * S + i], y2 = F[4 * S + i], z2 = F[5 * S + i];
          const float tv12[3] = {out[13 + 3], out[13 + 7], out[13 + 11]};
          sim3_project(out + 13, 4, tv12, x2, y2, z2, K1, &u, &v);
          const float d1x = F[6 * S + i] - u, d1y = F[7 * S + i] - v;
          const float err1 = (float)((0.0 + (double)d1x * (double)d1x) + (double)d1y * (double)d1y);
          // vP1im2 = Project(mvX3Dc1, mT21i, mK2)
          const float x1 = F[i], y1 = F[S + i], z1 = F[2 * S + i];
          sim3_project(t21, 3, t21 + 9, x1, y1, z1, K2, &u, &v);
          const float d2x = u - F[8 * S + i], d2y = v - F[9 * S + i];
          const float err2 = (float)((0.0 + (double)d2x * (double)d2x) + (double)d2y * (double)d2y);
          inl = err1 < F[10 * S + i] && err2 < F[11 * S + i];
        }
        const unsigned long long mask = __ballot(inl);
        if (lane == 0) bits[(size_t)h * Wn + tr] = mask;
        cnt += __popcll(mask);
      }
      if (lane == 0) {
        float* H = hyp + h * SIM3_HYP_WORDS;
        for (int k = 0; k < 29; ++k) H[k] = out[k];
        ((int*)H)[29] = cnt;
        ((int*)H)[30] = badDraw;
      }
    }
    __syncthreads();
    if (tid == 0) {  // the acceptance rule in iteration order (:190-207)
      int bestInl = ctl[0], taken = -1, stop = 0, ran = ctl[3];
      for (int h = 0; h < nh; ++h) {
        const int* H = (const int*)(hyp + h * SIM3_HYP_WORDS);
        if (H[30]) {  // a draw above rand_max: this iteration is not run
          stop = 2;
          break;
        }
        ++ran;
        const int cnt = H[29];
        if (cnt >= bestInl) {
          bestInl = cnt;
          taken = h;
          ctl[5] = it0 + c0 + h + 1;
          if (cnt > minInl) {
            ctl[6] = cnt;
            stop = 1;
            break;
          }
        }
      }
      ctl[0] = bestInl;
      ctl[1] = stop;
      ctl[2] = taken;
      ctl[3] = ran;
      if (taken >= 0) ctl[4] = 1;
    }
    __syncthreads();
    const int taken = ctl[2], stop = ctl[1];
    if (taken >= 0) {
      for (int w = tid; w < trips; w += SIM3_T) bestBits[w] = bits[(size_t)taken * Wn + w];
      if (tid < 29) best[tid] = hyp[taken * SIM3_HYP_WORDS + tid];
    }
    __syncthreads();  // before the next chunk overwrites bits / hyp
    if (stop) break;
  }

  const int stop = ctl[1], changed = ctl[4], ran = ctl[3];
  if (changed) {
    for (int i = tid; i < N; i += SIM3_T)
      C[i].best_inlier = (uint8_t)((bestBits[i >> 6] >> (i & 63)) & 1ull);
    if (stop == 1) {  // vbInliers[mvnIndices1[i]] = true (:202-204)
      __syncthreads();  // after the zeroing above
      for (int i = tid; i < N; i += SIM3_T)
        if ((bestBits[i >> 6] >> (i & 63)) & 1ull) {
          const int i1 = C[i].index1;
          if (i1 >= 0 && i1 < n1) IN[i1] = 1;
        }
    }
  }
  if (tid == 0) {
    const int its = it0 + ran;
    st->iterations = its;
    if (stop == 2) st->status = -1;
    if (changed) {
      st->best_inliers = ctl[0];
      st->best_iteration = ctl[5];
      st->best_scale = best[0];
      for (int k = 0; k < 9; ++k) st->best_R[k] = best[1 + k];
      for (int k = 0; k < 3; ++k) st->best_t[k] = best[10 + k];
      for (int k = 0; k < 16; ++k) st->best_T12[k] = best[13 + k];
    }
    orb_sim3_result_t r;
    memset(&r, 0, sizeof(r));
    r.iterations_run = ran;
    if (stop == 1) {
      r.has_sim3 = 1;
      r.n_inliers = ctl[6];
      r.scale = best[0];
      for (int k = 0; k < 9; ++k) r.R[k] = best[1 + k];
      for (int k = 0; k < 3; ++k) r.t[k] = best[10 + k];
      for (int k = 0; k < 16; ++k) r.T12[k] = best[13 + k];
    } else {
      r.no_more = (stop == 2 || its >= maxIts) ? 1 : 0;  // :210-211
    }
    *res = r;
  }
}

// ---------------------------------------------------------------- launchers
extern "C" int orb_k_sim3_max_stride(void) {
  int s = (int)((ORB_LDS_PER_CU - SIM3_FIXED_LDS) / (4 * SIM3_FIELDS)) & ~63;
  while (s > 0 && sim3_iter_lds(s) > ORB_LDS_PER_CU) s -= 64;
  return s;
}

extern "C" hipError_t orb_k_sim3_setup(const Sim3SetupParams* params, hipStream_t s) {
  const Sim3SetupParams P = *params;
  if (P.stride <= 0 || P.stride > orb_k_sim3_max_stride()) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sim3_setup, dim3(P.nProblems), dim3(SIM3_T), 0, s, P);
  return hipGetLastError();
}

extern "C" hipError_t orb_k_sim3_iterate(const Sim3IterParams* params, hipStream_t s) {
  const Sim3IterParams P = *params;
  if (P.stride <= 0 || P.stride > orb_k_sim3_max_stride()) return hipErrorInvalidValue;
  const size_t lds = sim3_iter_lds(P.stride);
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute((const void*)k_sim3_iterate,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_sim3_iterate, dim3(P.nProblems), dim3(SIM3_T), lds, s, P);
  return hipGetLastError();
}
