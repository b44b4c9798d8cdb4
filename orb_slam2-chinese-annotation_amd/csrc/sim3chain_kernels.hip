// sim3chain_kernels.hip -- gfx950 kernels of the two matcher stages of
// LoopClosing::ComputeSim3 (src/LoopClosing.cc:251-428) as device batches on
// the Sim3Solver's keyframe slots:
//   SearchByBoW(pKF1, pKF2, vpMatches12)   src/ORBmatcher.cc:581-716
//   SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)   :1212-1458,
//   with the inlier filter of src/LoopClosing.cc:338-343 in front of it.
// One workgroup of eight waves per problem, all state in LDS and the caller's
// arrays.  k_bow_kf_batch writes the solver's d_match12 / d_index2 rows;
// k_sim3_search_batch reads the solver's result and inliers and updates the
// same rows in place for the optimiser, so that a round of ComputeSim3 is
// iterate -> SearchBySim3 -> OptimizeSim3 on one stream.
#include <algorithm>

#include "bow_common.h"
#include "orb_kernels.h"
#include "projection_common.h"

// ======================================== SearchByBoW(KF, KF) as a batch
// k_bow_batch's structure (track_kernels.hip) with KF1 as the side that is
// walked in list order and KF2 as the side that is claimed: a keypoint lies in
// exactly one node, so nodes are independent and the waves draw KF1 nodes from
// an LDS counter; inside a node the KF1 keypoints are sequential through
// vbMatched2.  Per problem the LDS holds one word per KF2 keypoint (-2: no
// usable MapPoint, never a candidate; -1: free; else the KF1 keypoint that
// claimed it | its rotation bin << 24) and one word per KF1 node (the position
// of KF2's node with the same id); once the matching is over the node table is
// dead and becomes the row over KF1's keypoints (the KF2 keypoint, -1 none).
// Differences from SearchByBoW(KF, F): KF2's candidates need a non-NULL,
// non-bad point (:621-628), TH_LOW is strict (:650), the rows are indexed by
// KF1 and vbMatched2 is never cleared by the rotation filter.
#define BK_STATIC_LDS ((size_t)512)  // budget for hist[32], ctl[8] and the block vote
#define BK_TH_LOW 50

__global__ __launch_bounds__(BB_T) void k_bow_kf_batch(BowKfBatchParams P,
                                                       int32_t* __restrict__ match12,
                                                       int32_t* __restrict__ index2,
                                                       orb_bow_match_info_t* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
  __shared__ int hist[32];
  __shared__ int ctl[8];  // next node, tried, common nodes, accepted, removed
  static_assert(sizeof(hist) + sizeof(ctl) + 256 <= BK_STATIC_LDS, "capacity rule counts these");
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int S = (P.stride + 3) & ~3;
  int* claim2 = (int*)dyn;     // per KF2 keypoint: -2 unusable, -1 free, KF1 keypoint | bin << 24
  int* partner = claim2 + S;   // per KF1 node: position of KF2's node, -1 none; then the KF1 row

  const int s1 = P.kf1Slot ? P.kf1Slot[p] : p;
  const int s2 = P.kf2Slot ? P.kf2Slot[p] : p;
  const size_t b1 = (size_t)s1 * P.stride, b2 = (size_t)s2 * P.stride;
  const int n1 = min(max(P.kf.nkeys[s1], 0), P.stride);
  const int n2 = min(max(P.kf.nkeys[s2], 0), P.stride);
  const int nn1 = min(max(P.kf.nFvNodes[s1], 0), n1);
  const int nn2 = min(max(P.kf.nFvNodes[s2], 0), n2);
  const orb_keypoint_t* keys1 = P.kf.keys + b1;
  const uint8_t* desc1 = P.kf.desc + b1 * 32;
  const uint32_t* nodes1 = P.kf.fvNodes + b1;
  const int32_t* offs1 = P.kf.fvOffs + (size_t)s1 * ((size_t)P.stride + 1);
  const uint32_t* feats1 = P.kf.fvFeats + b1;
  const int32_t* PI1 = P.pointIndex + b1;
  const orb_keypoint_t* keys2 = P.kf.keys + b2;
  const uint8_t* desc2 = P.kf.desc + b2 * 32;
  const uint32_t* nodes2 = P.kf.fvNodes + b2;
  const int32_t* offs2 = P.kf.fvOffs + (size_t)s2 * ((size_t)P.stride + 1);
  const uint32_t* feats2 = P.kf.fvFeats + b2;
  const int32_t* PI2 = P.pointIndex + b2;
  const orb_map_point_t* PTS = P.points;
  int32_t* M12 = match12 + (size_t)p * P.stride;
  int32_t* IX2 = index2 + (size_t)p * P.stride;

  // ---- malformed slots: the offsets first, then (inside good offsets) the
  // feature indices; a bad value is reported and never used as an index
  int bad = bb_bad_offsets(offs1, nn1, n1, tid) | bb_bad_offsets(offs2, nn2, n2, tid);
  bad = __syncthreads_or(bad);
  if (!bad) {
    bad = bb_bad_feats(offs1, feats1, nn1, n1, tid) | bb_bad_feats(offs2, feats2, nn2, n2, tid);
    bad = __syncthreads_or(bad);
  }
  if (bad) {
    for (int i = tid; i < n1; i += BB_T) M12[i] = IX2[i] = -1;
    if (tid == 0) {
      info[p].n_matches = -1;
      info[p].n_accepted = 0;
      info[p].n_common_nodes = 0;
      info[p].n_tried = 0;
      info[p].enough = 0;
    }
    return;
  }

  // ---- KF2's usable keypoints (:621-628) and the merge-join on node id
  for (int i = tid; i < n2; i += BB_T) {
    const int pi = PI2[i];
    claim2[i] = (pi >= 0 && !(PTS && PTS[pi].bad)) ? -1 : -2;
  }
  if (tid < 32) hist[tid] = 0;
  if (tid < 8) ctl[tid] = 0;
  __syncthreads();
  {
    const int common = wave_sum(bb_join_nodes(nodes1, nn1, nodes2, nn2, partner, tid));
    if (lane == 0 && common) atomicAdd(&ctl[2], common);
  }
  __syncthreads();

  // ---- matching: a wave per KF1 node
  int tried = 0;
  for (;;) {
    int a = 0;
    if (lane == 0) a = atomicAdd(&ctl[0], 1);
    a = __builtin_amdgcn_readfirstlane(a);
    if (a >= nn1) break;
    const int fp = __builtin_amdgcn_readfirstlane(partner[a]);
    if (fp < 0) continue;
    const int kb0 = __builtin_amdgcn_readfirstlane(offs1[a]);
    const int ke0 = __builtin_amdgcn_readfirstlane(offs1[a + 1]);
    const int fb0 = __builtin_amdgcn_readfirstlane(offs2[fp]);
    const int fc = __builtin_amdgcn_readfirstlane(offs2[fp + 1]) - fb0;
    const bool fast = fc <= 64;
    // KF2's node in registers (fast path): a feature per lane
    int myF = 0;
    ulonglong4 dF = make_ulonglong4(0, 0, 0, 0);
    float aF = 0.0f;
    bool avail = false;
    if (fast && lane < fc) {
      myF = (int)feats2[fb0 + lane];
      avail = claim2[myF] == -1;
      if (avail) {
        dF = load_desc(desc2 + (size_t)myF * 32);
        aF = keys2[myF].angle;
      }
    }
    for (int c = kb0; c < ke0; c += 64) {
      // 64 KF1 features of the node, a feature per lane
      int kf = 0;
      ulonglong4 dK = make_ulonglong4(0, 0, 0, 0);
      float aK = 0.0f;
      bool ok = false;
      if (c + lane < ke0) {
        kf = (int)feats1[c + lane];
        const int pi = PI1[kf];
        ok = pi >= 0 && !(PTS && PTS[pi].bad);  // :607-612
        if (ok) {
          dK = load_desc(desc1 + (size_t)kf * 32);
          aK = keys1[kf].angle;
        }
      }
      unsigned long long todo = __ballot(ok);
      tried += __popcll(todo);
      while (todo) {  // in list order
        const int j = (int)__builtin_ctzll(todo);
        todo &= todo - 1;
        ulonglong4 q;
        q.x = lane_bcast64(dK.x, j);
        q.y = lane_bcast64(dK.y, j);
        q.z = lane_bcast64(dK.z, j);
        q.w = lane_bcast64(dK.w, j);
        int best1, best2, win, pos = 0;
        if (fast) {
          const int dist = avail ? hamming256(q, dF) : 256;
          const int key = wave_min((dist << 8) | lane);
          best1 = key >> 8;
          win = key & 63;
          best2 = wave_min(lane == win ? 256 : dist);
        } else {
          // per lane the first two of its trips in (distance, position) order
          int d1 = 256, q1 = 0xFFFF, d2 = 256;
          for (int t = lane; t < fc; t += 64) {
            const int rf = (int)feats2[fb0 + t];
            if (claim2[rf] != -1) continue;  // :618-628
            const int dist = hamming256(q, load_desc(desc2 + (size_t)rf * 32));
            if (dist < d1) { d2 = d1; d1 = dist; q1 = t; }
            else if (dist < d2) { d2 = dist; }
          }
          const int key = wave_min((d1 << 16) | q1);
          best1 = key >> 16;
          pos = key & 0xFFFF;
          win = pos & 63;  // position t is scanned by lane t & 63
          best2 = wave_min(lane == win ? d2 : d1);
        }
        if (best1 < BK_TH_LOW && (float)best1 < P.nnratio * (float)best2) {  // :650
          const int kfj = __builtin_amdgcn_readlane(kf, j);
          const float akj = __builtin_bit_cast(
              float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, aK), j));
          if (lane == win) {
            int rf = myF;
            float af = aF;
            if (!fast) {
              rf = (int)feats2[fb0 + pos];
              af = keys2[rf].angle;
            }
            const int bin = P.checkOri ? rot_bin(akj - af) : 0;  // :657-668
            claim2[rf] = kfj | (bin << 24);
            if (P.checkOri) atomicAdd(&hist[bin], 1);
            avail = false;
          }
        }
        if (!fast) {  // the next feature's trips read this claim
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
      }
    }
  }
  if (lane == 0 && tried) atomicAdd(&ctl[1], tried);
  __syncthreads();

  // ---- rotation filter (:675-691), the gate and the rows: the node table is
  // dead and receives, per KF1 keypoint, the KF2 keypoint that survived
  for (int i = tid; i < n1; i += BB_T) partner[i] = -1;
  int ind1 = -1, ind2 = -1, ind3 = -1;
  if (P.checkOri) three_maxima(hist, ind1, ind2, ind3);
  __syncthreads();
  int accepted = 0, removed = 0;
  for (int i = tid; i < n2; i += BB_T) {
    const int e = claim2[i];
    if (e < 0) continue;
    ++accepted;
    const int b = e >> 24;
    if (P.checkOri && b != ind1 && b != ind2 && b != ind3) ++removed;
    else partner[e & 0xFFFFFF] = i;
  }
  accepted = wave_sum(accepted);
  removed = wave_sum(removed);
  if (lane == 0) {
    atomicAdd(&ctl[3], accepted);
    atomicAdd(&ctl[4], removed);
  }
  __syncthreads();
  const int nm = ctl[3] - ctl[4];
  const bool enough = nm >= P.minMatches;
  for (int i = tid; i < n1; i += BB_T) {
    const int j = enough ? partner[i] : -1;
    M12[i] = j >= 0 ? PI2[j] : -1;
    IX2[i] = j;
  }
  if (tid == 0) {
    info[p].n_matches = nm;
    info[p].n_accepted = ctl[3];
    info[p].n_common_nodes = ctl[2];
    info[p].n_tried = ctl[1];
    info[p].enough = enough;
  }
}

// dynamic LDS of one k_bow_kf_batch workgroup at `stride` keypoint slots
static size_t bow_kf_batch_lds(int stride) {
  return 8 * (((size_t)stride + 3) & ~(size_t)3);
}

extern "C" int orb_k_bow_kf_batch_max_stride(void) {
  // 8 B per slot plus the static part within 160 KiB; the claim word holds 24
  // index bits
  int s = (int)((ORB_LDS_PER_CU - BK_STATIC_LDS) / 8) & ~3;
  while (bow_kf_batch_lds(s) + BK_STATIC_LDS > ORB_LDS_PER_CU) s -= 4;
  return std::min(s, (1 << 24) - 4);
}

extern "C" hipError_t orb_k_bow_kf_batch(const BowKfBatchParams* params, int32_t* match12,
                                         int32_t* index2, orb_bow_match_info_t* info,
                                         hipStream_t s) {
  const BowKfBatchParams P = *params;
  if (P.stride <= 0 || P.stride > orb_k_bow_kf_batch_max_stride()) return hipErrorInvalidValue;
  const size_t lds = bow_kf_batch_lds(P.stride);
  if (lds > 65536 - BK_STATIC_LDS) {
    hipError_t e = hipFuncSetAttribute((const void*)k_bow_kf_batch,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_bow_kf_batch, dim3(P.nProblems), dim3(BB_T), lds, s, P, match12, index2,
                     info);
  return hipGetLastError();
}

// ============================================= SearchBySim3 as a batch
// Phases of the workgroup (a barrier between two):
//  1  the inlier filter (src/LoopClosing.cc:338-343) on the two rows, and
//     vbAlreadyMatched1 into best1[] (-2 already matched, -1 free); best2[] free
//  2  vbAlreadyMatched2 (-2) from the kept index2 entries inside KF2's count;
//     threads 0 and 1 write the two directions' parameters (R1w, t1w, sR21,
//     t21 / R2w, t2w, sR12, t12) from the Sim3 record; both cell tables zeroed
//  3  cell counts of both keyframes (LDS atomics, all threads)
//  4  wave 0 / wave 1: exclusive scan of KF1's / KF2's table and the stable
//     scatter of k_grid_build (64 keypoints a round in index order; lanes of
//     the same cell find each other with 12 ballots over the cell id bits)
//  5  both directions at once, a thread per (direction, keypoint): the gates
//     of pp_project<PP_SIM3_DIR>, the window walk of for_features_in_area on
//     the LDS grid, the first minimum Hamming distance, accepted iff <= 100
//  6  the agreement (:1437-1452) into the rows and d_new12, and the counts
// LDS map: tbl[2][SS_TBL] ints (three pad words, then the 3,073 cell starts of
// a keyframe, so that the first cell's cursor is 16-byte aligned), then four
// arrays of S = (stride + 3) & ~3 ints: the cell-ordered index lists of KF1
// and KF2, best1 (vnMatch1) and best2 (vnMatch2).
#define SS_T 512
#define SS_TBL (GRID_CELLS + 4)
#define SS_STATIC_LDS ((size_t)1024)  // two PPParams, ctl[8] and the block vote
#define SS_TH_HIGH 100

// Exclusive scan of the 3,072 counts at t[1..] in place (t[0] = 0 stays), by
// one wave: 48 consecutive cells per lane, as k_grid_build.
__device__ __forceinline__ void ss_scan_cells(int* t, int lane) {
  constexpr int per = GRID_CELLS / 64;
  static_assert(per * 64 == GRID_CELLS && per % 4 == 0, "cells split evenly over the lanes");
  int4* c4 = reinterpret_cast<int4*>(t + 1 + lane * per);
  int4 v[per / 4];
  int s = 0;
#pragma unroll
  for (int i = 0; i < per / 4; ++i) {
    v[i] = c4[i];
    s += v[i].x + v[i].y + v[i].z + v[i].w;
  }
  int ex = wave_incl_scan(s) - s;
#pragma unroll
  for (int i = 0; i < per / 4; ++i) {
    const int4 e = make_int4(ex, ex + v[i].x, ex + v[i].x + v[i].y, ex + v[i].x + v[i].y + v[i].z);
    ex = e.w + v[i].w;
    c4[i] = e;
  }
}

__device__ __forceinline__ void ss_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The stable scatter of k_grid_build by one wave: t[1 + c] is cell c's cursor
// (its start on entry, its end = the next cell's start on return, so that t
// is the cell-start table afterwards); ci receives the keypoints in cell
// order, ascending index inside a cell.
__device__ __forceinline__ void ss_scatter(const orb_keypoint_t* K, int n, const PPParams& G,
                                           int* t, int* ci, int lane) {
  const unsigned long long ltMask = (1ull << lane) - 1ull;
  for (int base = 0; base < n; base += 64) {
    const int k = base + lane;
    int c = -1;
    if (k < n) c = grid_cell(K[k], G.minX, G.minY, G.invW, G.invH);
    const int id = c < 0 ? 4095 : c;
    unsigned long long peers = __ballot(1);
#pragma unroll
    for (int bit = 0; bit < 12; ++bit) {
      const unsigned long long m = __ballot((id >> bit) & 1);
      peers &= ((id >> bit) & 1) ? m : ~m;
    }
    int pos = 0;
    if (c >= 0) pos = t[1 + c] + __popcll(peers & ltMask);
    __builtin_amdgcn_wave_barrier();
    if (c >= 0) {
      ci[pos] = k;
      if ((peers >> lane) == 1ull) t[1 + c] += __popcll(peers);  // highest lane of the group
    }
    ss_wave_sync();
  }
}

__global__ __launch_bounds__(SS_T) void k_sim3_search_batch(Sim3SearchParams P) {
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
  __shared__ PPParams dirP[2];  // [0]: KF1's points into KF2, [1]: KF2's points into KF1
  __shared__ int ctl[8];        // kept, best12, best21, found
  static_assert(sizeof(dirP) + sizeof(ctl) + 256 <= SS_STATIC_LDS, "capacity rule counts these");
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (P.active && !P.active[p]) return;
  if (!P.sim3[p].has_sim3) return;
  const int S = (P.stride + 3) & ~3;
  int* tbl = (int*)dyn;          // tbl + 3 + g * SS_TBL: keyframe g's cell-start table
  int* ci1 = tbl + 2 * SS_TBL;   // KF1's keypoints in cell order
  int* ci2 = ci1 + S;
  int* best1 = ci2 + S;          // vnMatch1: -2 already matched, -1 none, else the KF2 keypoint
  int* best2 = best1 + S;
  int* t1 = tbl + 3;
  int* t2 = tbl + 3 + SS_TBL;

  const int s1 = P.kf1Slot ? P.kf1Slot[p] : p;
  const int s2 = P.kf2Slot ? P.kf2Slot[p] : p;
  const size_t b1 = (size_t)s1 * P.stride, b2 = (size_t)s2 * P.stride;
  const int n1 = min(max(P.nkeys[s1], 0), P.stride);
  const int n2 = min(max(P.nkeys[s2], 0), P.stride);
  const orb_keypoint_t* keys1 = P.keys + b1;
  const orb_keypoint_t* keys2 = P.keys + b2;
  const uint8_t* desc1 = P.desc + b1 * 32;
  const uint8_t* desc2 = P.desc + b2 * 32;
  const int32_t* PI1 = P.pointIndex + b1;
  const int32_t* PI2 = P.pointIndex + b2;
  int32_t* M12 = P.match12 + (size_t)p * P.stride;
  int32_t* IX2 = P.index2 + (size_t)p * P.stride;
  const uint8_t* INL = P.inliers12 ? P.inliers12 + (size_t)p * P.stride : nullptr;
  int32_t* NEW = P.new12 ? P.new12 + (size_t)p * P.stride : nullptr;

  // ---- 1: the inlier filter and vbAlreadyMatched1
  int kept = 0;
  for (int i = tid; i < n1; i += SS_T) {
    int m = M12[i];
    if (INL && !INL[i]) {
      m = -1;
      M12[i] = -1;
      IX2[i] = -1;
    }
    best1[i] = m >= 0 ? -2 : -1;
    kept += m >= 0;
  }
  for (int i = tid; i < n2; i += SS_T) best2[i] = -1;
  for (int i = tid; i < 2 * SS_TBL; i += SS_T) tbl[i] = 0;
  if (tid < 8) ctl[tid] = 0;
  __syncthreads();

  // ---- 2: vbAlreadyMatched2 (:1250-1256) and the two directions' parameters
  for (int i = tid; i < n1; i += SS_T) {
    if (best1[i] != -2) continue;
    const int j = IX2[i];
    if (j >= 0 && j < n2) best2[j] = -2;
  }
  if (tid < 2) {
    // field by field with constant indices: a struct copy of the by-value
    // block goes through scratch
    PPParams& D = dirP[tid];
    D.fx = P.base.fx; D.fy = P.base.fy; D.cx = P.base.cx; D.cy = P.base.cy; D.bf = P.base.bf;
    D.minX = P.base.minX; D.maxX = P.base.maxX; D.minY = P.base.minY; D.maxY = P.base.maxY;
    D.invW = P.base.invW; D.invH = P.base.invH;
    D.th = P.base.th; D.logScale = P.base.logScale;
    D.nLevels = P.base.nLevels; D.thr = P.base.thr; D.checkOri = 0;
#pragma unroll
    for (int l = 0; l < ORB_MAX_LEVELS; ++l) {
      D.scale[l] = P.base.scale[l];
      D.invSigma2[l] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) D.Ow[i] = 0.f;
    const orb_sim3_result_t& X = P.sim3[p];
    const orb_pose_t& pose = P.pose[tid == 0 ? s1 : s2];
    const double s = (double)X.scale;
#pragma unroll
    for (int i = 0; i < 9; ++i) D.R[i] = pose.rcw[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) D.t[i] = pose.tcw[i];
    if (tid == 0) {  // sR21 = (1 / s) R12^T, t21 = -sR21 t12 (:1231-1235)
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) D.R2[3 * r + c] = (float)((1.0 / s) * (double)X.R[3 * c + r]);
#pragma unroll
      for (int r = 0; r < 3; ++r)
        D.t2[r] = -((D.R2[3 * r] * X.t[0] + D.R2[3 * r + 1] * X.t[1]) + D.R2[3 * r + 2] * X.t[2]);
    } else {  // sR12 = s R12, t12
#pragma unroll
      for (int i = 0; i < 9; ++i) D.R2[i] = (float)(s * (double)X.R[i]);
#pragma unroll
      for (int i = 0; i < 3; ++i) D.t2[i] = X.t[i];
    }
  }
  // ---- 3: cell counts
  for (int i = tid; i < n1 + n2; i += SS_T) {
    const bool second = i >= n1;
    const int c = grid_cell(second ? keys2[i - n1] : keys1[i], P.base.minX, P.base.minY,
                            P.base.invW, P.base.invH);
    if (c >= 0) atomicAdd(&(second ? t2 : t1)[1 + c], 1);
  }
  __syncthreads();

  // ---- 4: scan and stable scatter, a wave per keyframe
  if (wave < 2) {
    int* t = wave ? t2 : t1;
    ss_scan_cells(t, lane);
    ss_wave_sync();
    ss_scatter(wave ? keys2 : keys1, wave ? n2 : n1, P.base, t, wave ? ci2 : ci1, lane);
  }
  __syncthreads();

  // ---- 5: both directions (:1264-1348, :1351-1434)
  ProjParams G;
  G.minX = P.base.minX; G.minY = P.base.minY; G.invW = P.base.invW; G.invH = P.base.invH;
  int nb12 = 0, nb21 = 0;
  for (int i = tid; i < n1 + n2; i += SS_T) {
    const bool second = i >= n1;
    const int ia = second ? i - n1 : i;
    int* bestA = second ? best2 : best1;
    if (bestA[ia] == -2) continue;  // vbAlreadyMatched
    const int pi = (second ? PI2 : PI1)[ia];
    if (pi < 0) continue;
    const orb_map_point_t mp = P.points[pi];
    if (mp.bad) continue;
    const PPRec r = pp_project<PP_SIM3_DIR>(mp, dirP[second ? 1 : 0]);
    if (!r.valid) continue;
    const orb_keypoint_t* keysB = second ? keys1 : keys2;
    const uint8_t* descB = second ? desc1 : desc2;
    const ulonglong4 q = load_desc(P.mpDesc + (size_t)pi * 32);
    int bd = 256, bi = -1;
    for_features_in_area(keysB, second ? t1 : t2, second ? ci1 : ci2, G, r.u, r.v, r.radius,
                         r.minL, r.maxL, [&](int idx, const orb_keypoint_t&) {
                           const int d = hamming256(q, load_desc(descB + (size_t)idx * 32));
                           if (d < bd) { bd = d; bi = idx; }
                         });
    if (bd <= SS_TH_HIGH) {
      bestA[ia] = bi;
      if (second) ++nb21; else ++nb12;
    }
  }
  __syncthreads();

  // ---- 6: the agreement (:1437-1452), the rows and the counts
  int found = 0;
  for (int i = tid; i < n1; i += SS_T) {
    const int j = best1[i];
    const bool ok = j >= 0 && best2[j] == i;
    if (ok) {
      M12[i] = PI2[j];
      IX2[i] = j;
      ++found;
    }
    if (NEW) NEW[i] = ok ? j : -1;
  }
  kept = wave_sum(kept);
  nb12 = wave_sum(nb12);
  nb21 = wave_sum(nb21);
  found = wave_sum(found);
  if (lane == 0) {
    atomicAdd(&ctl[0], kept);
    atomicAdd(&ctl[1], nb12);
    atomicAdd(&ctl[2], nb21);
    atomicAdd(&ctl[3], found);
  }
  __syncthreads();
  if (tid == 0) {
    orb_sim3_search_info_t o;
    o.n_found = ctl[3];
    o.n_kept = ctl[0];
    o.n_total = ctl[0] + ctl[3];
    o.n_best12 = ctl[1];
    o.n_best21 = ctl[2];
    P.info[p] = o;
  }
}

// dynamic LDS of one k_sim3_search_batch workgroup at `stride` keypoint slots
static size_t sim3_search_lds(int stride) {
  return 4 * (2 * (size_t)SS_TBL + 4 * (((size_t)stride + 3) & ~(size_t)3));
}

extern "C" int orb_k_sim3_search_max_stride(void) {
  // 16 B per slot beside the two cell tables and the static part within 160 KiB
  int s = (int)((ORB_LDS_PER_CU - SS_STATIC_LDS - 8 * (size_t)SS_TBL) / 16) & ~3;
  while (sim3_search_lds(s) + SS_STATIC_LDS > ORB_LDS_PER_CU) s -= 4;
  return s;
}

extern "C" hipError_t orb_k_sim3_search(const Sim3SearchParams* params, hipStream_t s) {
  const Sim3SearchParams P = *params;
  if (P.stride <= 0 || P.stride > orb_k_sim3_search_max_stride()) return hipErrorInvalidValue;
  const size_t lds = sim3_search_lds(P.stride);
  if (lds > 65536 - SS_STATIC_LDS) {
    hipError_t e = hipFuncSetAttribute((const void*)k_sim3_search_batch,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_sim3_search_batch, dim3(P.nProblems), dim3(SS_T), lds, s, P);
  return hipGetLastError();
}
