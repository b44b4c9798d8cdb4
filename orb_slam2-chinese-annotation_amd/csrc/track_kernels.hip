// track_kernels.hip -- gfx950 kernels of Tracking::TrackWithMotionModel's
// matcher stage as a device-resident batch: SearchByProjection(CurrentFrame,
// LastFrame, th, bMono) (src/ORBmatcher.cc:1460-1619) with the 2 * th retry
// (src/Tracking.cc:1044-1052), and the "Discard outliers" loop (:1060-1083)
// with SearchLocalPoints' already-matched marking (:1333-1354); and of
// TrackReferenceKeyFrame's and Relocalization's matcher stage, SearchByBoW(pKF,
// F, vpMapPointMatches) (src/ORBmatcher.cc:164-306), as the same kind of batch
// (k_bow_batch, at the end of the file); and, after it, of the neighbour loop
// of LocalMapping::CreateNewMapPoints, SearchForTriangulation
// (src/ORBmatcher.cc:718-901), on the same keyframe slots (k_tri_batch).
//
// k_frame_batch: one workgroup of four waves per problem, the problem's grid
// built before it by k_grid_build.  Per pass: every wave projects last-frame
// points with the poses read on the device and scans their windows, leaving
// per point the first TOPK candidates in (distance, scan order), the count and
// has_obs in LDS; wave 0 then replays the sequential loop over speculative
// 64-point windows exactly as k_frame_resolve does (matcher_kernels.hip), with
// every value on its serial chain in LDS: the candidate entries carry the
// keypoint, the distance and the rotation bin, so the replay loads nothing from
// global memory except in the exact re-scan of a point whose top-K ran dry;
// all waves apply the rotation filter and count.  The workgroup itself decides
// whether the problem runs again with 2 * th.
#include <algorithm>

#include "bow_common.h"
#include "matcher_common.h"
#include "orb_kernels.h"

#define FB_T 256
#define FB_STATIC_LDS ((size_t)512)  // budget for hist[32], ctl[4] and the block vote

// Candidate entry: keypoint index (14b) | rotation bin (5b) << 14 | distance
// (9b) << 19; the distance sits where Top4 reads it (cand_dist), an empty slot
// is 0xFFFFFFFF (distance 511).
__device__ __forceinline__ uint32_t fb_pack(int idx, int bin, int dist) {
  return (uint32_t)idx | ((uint32_t)bin << 14) | ((uint32_t)dist << 19);
}
__device__ __forceinline__ int fb_idx(uint32_t e) { return (int)(e & 0x3FFFu); }
__device__ __forceinline__ int fb_bin(uint32_t e) { return (int)((e >> 14) & 31u); }

__device__ __forceinline__ bool fb_locked(const uint32_t* bm, int idx) {
  return (bm[idx >> 5] >> (idx & 31)) & 1u;
}

// ((r0 x + r1 y) + r2 z) + t: cv::Mat's float product row by row, then the sum
__device__ __forceinline__ float fb_row(const float* R, int r, float x, float y, float z, float t) {
  return ((R[3 * r] * x + R[3 * r + 1] * y) + R[3 * r + 2] * z) + t;
}

struct FbWindow {
  float u, v, invzc, radius;
  int minL, maxL;
};

// src/ORBmatcher.cc:1489-1535 for last-frame keypoint m: false when the
// reference skips the point before its window scan.  The octave is in range
// (checked for the whole problem first).
__device__ __forceinline__ bool fb_window(const FrameBatchParams& P, const float* Rcw,
                                          const float* tcw, const orb_keypoint_t* lastKeys,
                                          const int32_t* lastIdx, const uint8_t* lastOut,
                                          const orb_map_point_t* pts, int m, float th, bool fwd,
                                          bool bwd, FbWindow& w, int& pointIdx) {
  const int pi = lastIdx[m];
  pointIdx = pi;
  if (pi < 0) return false;
  if (lastOut && lastOut[m]) return false;
  const float x = pts[pi].pos[0], y = pts[pi].pos[1], z = pts[pi].pos[2];
  const float xc = fb_row(Rcw, 0, x, y, z, tcw[0]);
  const float yc = fb_row(Rcw, 1, x, y, z, tcw[1]);
  const float zc = fb_row(Rcw, 2, x, y, z, tcw[2]);
  w.invzc = __fdiv_rn(1.0f, zc);
  if (w.invzc < 0) return false;
  w.u = P.fx * xc * w.invzc + P.cx;
  w.v = P.fy * yc * w.invzc + P.cy;
  if (w.u < P.minX || w.u > P.maxX) return false;
  if (w.v < P.minY || w.v > P.maxY) return false;
  const int o = lastKeys[m].octave;
  w.radius = th * P.scale[o];
  if (fwd) { w.minL = o; w.maxL = -1; }
  else if (bwd) { w.minL = 0; w.maxL = o; }
  else { w.minL = o - 1; w.maxL = o + 1; }
  return true;
}

__global__ __launch_bounds__(FB_T) void k_frame_batch(
    FrameBatchParams P, const orb_keypoint_t* __restrict__ keys, const uint8_t* __restrict__ desc,
    const float* __restrict__ uright, const uint8_t* __restrict__ locked,
    const int32_t* __restrict__ nkeys, const orb_pose_t* __restrict__ poseCur,
    const orb_pose_t* __restrict__ poseLast, const orb_keypoint_t* __restrict__ lastKeys,
    const int32_t* __restrict__ lastNkeys, const int32_t* __restrict__ lastPointIndex,
    const uint8_t* __restrict__ lastOutlier, const orb_map_point_t* __restrict__ points,
    const uint8_t* __restrict__ mpDesc, const int32_t* __restrict__ cellStart,
    const int32_t* __restrict__ cellIdx, int32_t* __restrict__ kpMatch,
    orb_frame_match_info_t* __restrict__ info) {
  // LDS per keypoint slot: four candidate entries, the point's count | has_obs,
  // its accepted keypoint | bin, the window's earliest claiming lane and the
  // last point assigned per keypoint; then the lock bits
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
  __shared__ int hist[32];
  __shared__ int ctl[4];  // accepted, removed
  static_assert(sizeof(hist) + sizeof(ctl) + 256 <= FB_STATIC_LDS, "capacity rule counts these");
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = (P.stride + 3) & ~3;
  uint32_t* top = dyn;
  int* meta = (int*)(dyn + 4 * (size_t)S);
  int* acc = meta + S;
  int* claimBy = acc + S;
  int* lastWriter = claimBy + S;
  uint32_t* bm = (uint32_t*)(lastWriter + S);

  const int n = min(max(nkeys[p], 0), P.stride);
  const int nlast = min(max(lastNkeys[p], 0), P.stride);
  const int words = (n + 31) >> 5;
  const size_t kb = (size_t)p * P.stride;
  const orb_keypoint_t* K = keys + kb;
  const uint8_t* D = desc + kb * 32;
  const float* UR = uright ? uright + kb : nullptr;
  const uint8_t* LK = locked ? locked + kb : nullptr;
  const orb_keypoint_t* LKEYS = lastKeys + kb;
  const int32_t* LIDX = lastPointIndex + kb;
  const uint8_t* LOUT = lastOutlier ? lastOutlier + kb : nullptr;
  const size_t mb = (size_t)p * (size_t)P.mpStride;
  const orb_map_point_t* PTS = points + mb;
  const uint8_t* MD = mpDesc + mb * 32;
  const int32_t* cs = cellStart + (size_t)p * (GRID_CELLS + 1);
  const int32_t* ci = cellIdx + kb;
  int32_t* KM = kpMatch + kb;

  // poses: Rcw, tcw of the current frame; the last frame's third row for tlc.z
  float Rcw[9], tcw[3];
  for (int i = 0; i < 9; ++i) Rcw[i] = poseCur[p].rcw[i];
  for (int i = 0; i < 3; ++i) tcw[i] = poseCur[p].tcw[i];
  float twc[3];  // src/ORBmatcher.cc:1475, as Frame::UpdatePoseMatrices' mOw
  for (int i = 0; i < 3; ++i)
    twc[i] = -((Rcw[i] * tcw[0] + Rcw[3 + i] * tcw[1]) + Rcw[6 + i] * tcw[2]);
  const float tlcz = fb_row(poseLast[p].rcw, 2, twc[0], twc[1], twc[2], poseLast[p].tcw[2]);
  const bool fwd = tlcz > P.mb && !P.mono;   // :1482
  const bool bwd = -tlcz > P.mb && !P.mono;  // :1484

  // an octave the scale table does not have: the problem is reported, not run
  {
    int bad = 0;
    for (int m = tid; m < nlast; m += FB_T) {
      if (LIDX[m] < 0 || (LOUT && LOUT[m])) continue;
      const int o = LKEYS[m].octave;
      bad |= (o < 0 || o >= P.nLevels);
    }
    if (__syncthreads_or(bad)) {
      for (int i = tid; i < n; i += FB_T) KM[i] = -1;
      if (tid == 0) {
        info[p].n_matches = -1;
        info[p].n_matches_first_pass = -1;
        info[p].retried = 0;
        info[p].forward = fwd;
        info[p].backward = bwd;
      }
      return;
    }
  }

  ProjParams G;  // the grid geometry for_features_in_area reads
  G.minX = P.minX; G.minY = P.minY; G.invW = P.invW; G.invH = P.invH;

  float th = P.th;
  int first = 0, retried = 0, nm = 0;
  for (int pass = 0;; ++pass) {
    for (int i = tid; i < words; i += FB_T) bm[i] = 0u;
    for (int i = tid; i < n; i += FB_T) { claimBy[i] = 64; lastWriter[i] = -1; }
    if (tid < 32) hist[tid] = 0;
    if (tid < 4) ctl[tid] = 0;

    // ---- projection and candidate scan, a point per thread
    for (int m = tid; m < nlast; m += FB_T) {
      FbWindow w;
      int pi;
      Top4 t4;
      int count = -1, hasObs = 0;
      if (fb_window(P, Rcw, tcw, LKEYS, LIDX, LOUT, PTS, m, th, fwd, bwd, w, pi)) {
        hasObs = PTS[pi].has_obs != 0;
        const ulonglong4 q = load_desc(MD + (size_t)pi * 32);
        const float la = LKEYS[m].angle;
        count = 0;
        for_features_in_area(K, cs, ci, G, w.u, w.v, w.radius, w.minL, w.maxL,
                             [&](int idx, const orb_keypoint_t& kp) {
                               if (idx >= n) return;
                               if (LK && LK[idx]) return;
                               if (UR && UR[idx] > 0) {
                                 const float ur = w.u - P.bf * w.invzc;
                                 const float er = fabsf(ur - UR[idx]);
                                 if (er > w.radius) return;
                               }
                               const int dist = hamming256(q, load_desc(D + (size_t)idx * 32));
                               if (dist >= 256) return;
                               ++count;
                               const int bin = P.checkOri ? rot_bin(la - kp.angle) : 0;
                               t4.insert(fb_pack(idx, bin, dist), dist);
                             });
      }
      t4.store(top + (size_t)m * TOPK);
      meta[m] = count < 0 ? -1 : (count | (hasObs << 24));
      acc[m] = -1;
    }
    __syncthreads();

    // ---- the ordered replay, wave 0 (k_frame_resolve's windows)
    if (wave == 0) {
      int start = 0;
      while (start < nlast) {
        const int m = start + lane;
        const bool active = m < nlast;
        int nc = -1;
        uint32_t e[TOPK] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        bool hasObs = false;
        if (active) {
          const int mt = meta[m];
          nc = mt < 0 ? -1 : (mt & 0xFFFFFF);
          hasObs = mt >= 0 && (mt >> 24) != 0;
          const uint4 t = *reinterpret_cast<const uint4*>(top + (size_t)m * TOPK);
          e[0] = t.x; e[1] = t.y; e[2] = t.z; e[3] = t.w;
        }
        int best = -1, bestDist = 256, bestBin = 0, consumed = 0;
        const int avail = nc < TOPK ? nc : TOPK;  // <= 0: no candidate
#pragma unroll
        for (int j = 0; j < TOPK; ++j) {
          if (j < avail && best < 0) {
            ++consumed;
            if (!fb_locked(bm, fb_idx(e[j]))) {
              best = fb_idx(e[j]);
              bestDist = cand_dist(e[j]);
              bestBin = fb_bin(e[j]);
            }
          }
        }
        const bool slow = nc > TOPK && best < 0;
        const bool accept = !slow && best >= 0 && bestDist <= 100;  // TH_HIGH
        const bool locks = accept && hasObs;
        if (locks) atomicMin(&claimBy[best], lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        bool conflict = false;
#pragma unroll
        for (int q = 0; q < TOPK; ++q)
          if (q < consumed) conflict |= claimBy[fb_idx(e[q])] < lane;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (locks) claimBy[best] = 64;
        const unsigned long long bad = __ballot(active && (conflict || (slow && lane > 0)));
        const unsigned long long slowFirst = __ballot(lane == 0 && active && slow);
        int commit = bad ? (int)__builtin_ctzll(bad) : 64;
        if (slowFirst) {
          if (lane == 0) {  // exact re-scan against the current locks
            FbWindow w;
            int pi;
            fb_window(P, Rcw, tcw, LKEYS, LIDX, LOUT, PTS, m, th, fwd, bwd, w, pi);
            const ulonglong4 q = load_desc(MD + (size_t)pi * 32);
            int bd = 256, bi = -1;
            for_features_in_area(K, cs, ci, G, w.u, w.v, w.radius, w.minL, w.maxL,
                                 [&](int idx, const orb_keypoint_t& kp) {
                                   if (idx >= n) return;
                                   if ((LK && LK[idx]) || fb_locked(bm, idx)) return;
                                   if (UR && UR[idx] > 0) {
                                     const float ur = w.u - P.bf * w.invzc;
                                     if (fabsf(ur - UR[idx]) > w.radius) return;
                                   }
                                   const int dist =
                                       hamming256(q, load_desc(D + (size_t)idx * 32));
                                   if (dist < bd) { bd = dist; bi = idx; }
                                 });
            if (bd <= 100) {
              const int bin = P.checkOri ? rot_bin(LKEYS[m].angle - K[bi].angle) : 0;
              acc[m] = bi | (bin << 16);
              atomicMax(&lastWriter[bi], m);
              if (hasObs) bm[bi >> 5] |= 1u << (bi & 31);
              if (P.checkOri) atomicAdd(&hist[bin], 1);
            }
          }
          commit = 1;
        } else {
          if (active && lane < commit && accept) {
            acc[m] = best | (bestBin << 16);
            atomicMax(&lastWriter[best], m);
            if (locks) atomicOr(&bm[best >> 5], 1u << (best & 31));
            if (P.checkOri) atomicAdd(&hist[bestBin], 1);
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        start += commit;
      }
    }
    __syncthreads();

    // ---- rotation filter (:1597-1616): the records of the bins outside the
    // top three are undone; bm becomes "reset to NULL by the filter"
    int ind1 = -1, ind2 = -1, ind3 = -1;
    if (P.checkOri) three_maxima(hist, ind1, ind2, ind3);
    for (int i = tid; i < words; i += FB_T) bm[i] = 0u;
    __syncthreads();
    int removed = 0, accepted = 0;
    for (int m = tid; m < nlast; m += FB_T) {
      const int a = acc[m];
      if (a < 0) continue;
      ++accepted;
      if (!P.checkOri) continue;
      const int b = a >> 16, bi = a & 0xFFFF;
      if (b != ind1 && b != ind2 && b != ind3) {
        ++removed;
        atomicOr(&bm[bi >> 5], 1u << (bi & 31));
      }
    }
    accepted = wave_sum(accepted);
    removed = wave_sum(removed);
    if (lane == 0) {
      atomicAdd(&ctl[0], accepted);
      atomicAdd(&ctl[1], removed);
    }
    __syncthreads();
    nm = ctl[0] - ctl[1];
    if (pass == 0) first = nm;
    if (pass == 0 && P.retryBelow > 0 && nm < P.retryBelow) {  // src/Tracking.cc:1048-1052
      retried = 1;
      th = 2.0f * P.th;
      __syncthreads();  // ctl and bm are read before the next pass clears them
      continue;
    }
    break;
  }

  // kp_match: the map-point index assigned by the (last) pass, -1 untouched,
  // -2 reset to NULL by the filter
  for (int i = tid; i < n; i += FB_T) {
    const int wr = lastWriter[i];
    if ((bm[i >> 5] >> (i & 31)) & 1u) KM[i] = -2;
    else KM[i] = wr >= 0 ? LIDX[wr] : -1;
  }
  if (tid == 0) {
    info[p].n_matches = nm;
    info[p].n_matches_first_pass = first;
    info[p].retried = retried;
    info[p].forward = fwd;
    info[p].backward = bwd;
  }
}

// dynamic LDS of one k_frame_batch workgroup at `stride` keypoint slots
static size_t frame_batch_lds(int stride) {
  const size_t S = ((size_t)stride + 3) & ~(size_t)3;
  const size_t W = ((S + 31) / 32 + 3) & ~(size_t)3;
  return (8 * S + W) * 4;
}

extern "C" int orb_k_frame_batch_max_stride(void) {
  // 32 B and one bit per slot, plus the static part, within 160 KiB; the
  // candidate entries hold 14 index bits
  int s = (int)((ORB_LDS_PER_CU - FB_STATIC_LDS) / 32) & ~3;
  while (frame_batch_lds(s) + FB_STATIC_LDS > ORB_LDS_PER_CU) s -= 4;
  return std::min(s, (1 << 14) - 4);
}

extern "C" hipError_t orb_k_frame_batch(
    const FrameBatchParams* params, const orb_keypoint_t* keys, const uint8_t* desc,
    const float* uright, const uint8_t* locked, const int32_t* nkeys, const orb_pose_t* poseCur,
    const orb_pose_t* poseLast, const orb_keypoint_t* lastKeys, const int32_t* lastNkeys,
    const int32_t* lastPointIndex, const uint8_t* lastOutlier, const orb_map_point_t* points,
    const uint8_t* mpDesc, const int32_t* cellStart, const int32_t* cellIdx, int32_t* kpMatch,
    orb_frame_match_info_t* info, hipStream_t s) {
  const FrameBatchParams P = *params;
  if (P.stride <= 0 || P.stride > orb_k_frame_batch_max_stride()) return hipErrorInvalidValue;
  const size_t lds = frame_batch_lds(P.stride);
  if (lds > 65536 - FB_STATIC_LDS) {
    hipError_t e = hipFuncSetAttribute((const void*)k_frame_batch,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_frame_batch, dim3(P.nProblems), dim3(FB_T), lds, s, P, keys, desc, uright,
                     locked, nkeys, poseCur, poseLast, lastKeys, lastNkeys, lastPointIndex,
                     lastOutlier, points, mpDesc, cellStart, cellIdx, kpMatch, info);
  return hipGetLastError();
}

// ------------------------------------------------ discard outliers and mark
// src/Tracking.cc:1060-1083 over one problem's keypoints, then (markSeen) the
// first loop of SearchLocalPoints (:1333-1354) on what is kept.  Several
// keypoints may hold one point: their `seen` stores write the same byte value.
// The matcher's count is nMatches[p * nMatchesStride] (the first field of
// either matcher's info records).
__global__ __launch_bounds__(256) void k_track_discard(
    int stride, long long mpStride, int markSeen, const int32_t* __restrict__ nkeys,
    int32_t* __restrict__ kpMatch, uint8_t* __restrict__ outlier, orb_map_point_t* points,
    const int32_t* __restrict__ nMatches, int nMatchesStride,
    orb_track_discard_info_t* __restrict__ out) {
  __shared__ int cnt[2];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(nkeys[p], 0), stride);
  int32_t* KM = kpMatch + (size_t)p * stride;
  uint8_t* OL = outlier + (size_t)p * stride;
  orb_map_point_t* PTS = points + (size_t)p * (size_t)mpStride;
  if (tid < 2) cnt[tid] = 0;
  __syncthreads();
  int discarded = 0, inMap = 0;
  for (int i = tid; i < n; i += 256) {
    const int pi = KM[i];
    if (pi < 0) continue;
    if (OL[i]) {
      KM[i] = -1;
      OL[i] = 0;
      if (markSeen) PTS[pi].seen = 1;  // mnLastFrameSeen = mCurrentFrame.mnId (:1076)
      ++discarded;
    } else {
      if (PTS[pi].has_obs) ++inMap;
      if (markSeen) {
        if (PTS[pi].bad) KM[i] = -1;  // :1340-1343
        else PTS[pi].seen = 1;        // :1350
      }
    }
  }
  discarded = wave_sum(discarded);
  inMap = wave_sum(inMap);
  if ((tid & 63) == 0) {
    atomicAdd(&cnt[0], discarded);
    atomicAdd(&cnt[1], inMap);
  }
  __syncthreads();
  if (tid == 0) {
    out[p].n_discarded = cnt[0];
    out[p].n_matches_map = cnt[1];
    out[p].n_matches = nMatches[(size_t)p * nMatchesStride] - cnt[0];
  }
}

extern "C" hipError_t orb_k_track_discard(int nProblems, int stride, long long mpStride,
                                          int markSeen, const int32_t* nkeys, int32_t* kpMatch,
                                          uint8_t* outlier, orb_map_point_t* points,
                                          const int32_t* nMatches, int nMatchesStride,
                                          orb_track_discard_info_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_track_discard, dim3(nProblems), dim3(256), 0, s, stride, mpStride,
                     markSeen, nkeys, kpMatch, outlier, points, nMatches, nMatchesStride, out);
  return hipGetLastError();
}

// ============================== SearchByBoW(KeyFrame*, Frame&, ...) as a batch
// src/ORBmatcher.cc:164-306 for Tracking::TrackReferenceKeyFrame
// (src/Tracking.cc:904-954) and Relocalization's candidates (:1592-1616): one
// workgroup of eight waves per problem, one launch for validation, matching, the rotation
// filter, the min_matches gate and the outputs.  A frame feature belongs to
// exactly one node, so nodes are independent (k_bow_match): the waves draw
// keyframe nodes from an LDS counter.  Per problem the LDS holds one word per
// frame keypoint (the keyframe keypoint that claimed it | its rotation bin <<
// 24, -1 unclaimed: claim flag and accepted list in one, with no word shared
// between nodes and so no atomics on it), and per keyframe node the position
// of the frame's node with the same id, found by all threads at once before
// the matching, so that no binary search sits between two nodes of a wave.
// A node of at most 64 frame features keeps a frame descriptor, its angle and
// the claimed flag per lane in registers for the whole node; the keyframe
// features are loaded a feature per lane too (64 at a time) and broadcast from
// there by readlane, so the serial loop over them loads nothing: a step is one
// Hamming distance and two wave-wide minima, by (distance, position) and of
// the distance over the lanes other than the winner.  Larger frame nodes scan
// in 64-lane trips with the claims read from LDS.
// (BB_T, wave_min, lane_bcast64, the FeatureVector checks and the node join:
// bow_common.h, shared with k_bow_kf_batch in sim3chain_kernels.hip)
#define BB_STATIC_LDS ((size_t)512)  // budget for hist[32], ctl[8] and the block vote
#define BB_TH_LOW 50

__global__ __launch_bounds__(BB_T) void k_bow_batch(BowBatchParams P, int32_t* __restrict__ kpMatch,
                                                    orb_bow_match_info_t* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
  __shared__ int hist[32];
  __shared__ int ctl[8];  // next node, tried, common nodes, accepted, removed
  static_assert(sizeof(hist) + sizeof(ctl) + 256 <= BB_STATIC_LDS, "capacity rule counts these");
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int S = (P.stride + 3) & ~3;
  int* fmatch = (int*)dyn;    // per frame keypoint: keyframe keypoint | bin << 24, -1 unclaimed
  int* partner = fmatch + S;  // per keyframe node: position of the frame's node, -1 none

  const int ks = P.kfIndex ? P.kfIndex[p] : p;
  const int fs = P.fIndex ? P.fIndex[p] : p;
  const size_t kb = (size_t)ks * P.stride, fb = (size_t)fs * P.stride;
  const int nK = min(max(P.kf.nkeys[ks], 0), P.stride);
  const int nF = min(max(P.f.nkeys[fs], 0), P.stride);
  const int nnK = min(max(P.kf.nFvNodes[ks], 0), nK);
  const int nnF = min(max(P.f.nFvNodes[fs], 0), nF);
  const orb_keypoint_t* kKeys = P.kf.keys + kb;
  const uint8_t* kDesc = P.kf.desc + kb * 32;
  const uint32_t* kNodes = P.kf.fvNodes + kb;
  const int32_t* kOffs = P.kf.fvOffs + (size_t)ks * ((size_t)P.stride + 1);
  const uint32_t* kFeats = P.kf.fvFeats + kb;
  const int32_t* PI = P.kfPointIndex + kb;
  const orb_keypoint_t* fKeys = P.f.keys + fb;
  const uint8_t* fDesc = P.f.desc + fb * 32;
  const uint32_t* fNodes = P.f.fvNodes + fb;
  const int32_t* fOffs = P.f.fvOffs + (size_t)fs * ((size_t)P.stride + 1);
  const uint32_t* fFeats = P.f.fvFeats + fb;
  const orb_map_point_t* PTS = P.points ? P.points + (size_t)p * (size_t)P.mpStride : nullptr;
  int32_t* KM = kpMatch + (size_t)p * P.stride;

  // ---- malformed slots: the offsets first, then (inside good offsets) the
  // feature indices; a bad value is reported and never used as an index
  int bad = bb_bad_offsets(kOffs, nnK, nK, tid) | bb_bad_offsets(fOffs, nnF, nF, tid);
  bad = __syncthreads_or(bad);
  if (!bad) {
    bad = bb_bad_feats(kOffs, kFeats, nnK, nK, tid) | bb_bad_feats(fOffs, fFeats, nnF, nF, tid);
    bad = __syncthreads_or(bad);
  }
  if (bad) {
    for (int i = tid; i < nF; i += BB_T) KM[i] = -1;
    if (tid == 0) {
      info[p].n_matches = -1;
      info[p].n_accepted = 0;
      info[p].n_common_nodes = 0;
      info[p].n_tried = 0;
      info[p].enough = 0;
    }
    return;
  }

  // ---- the merge-join on node id, a keyframe node per thread
  for (int i = tid; i < nF; i += BB_T) fmatch[i] = -1;
  if (tid < 32) hist[tid] = 0;
  if (tid < 8) ctl[tid] = 0;
  __syncthreads();
  {
    const int common = wave_sum(bb_join_nodes(kNodes, nnK, fNodes, nnF, partner, tid));
    if (lane == 0 && common) atomicAdd(&ctl[2], common);
  }
  __syncthreads();

  // ---- matching: a wave per keyframe node
  int tried = 0;
  for (;;) {
    int a = 0;
    if (lane == 0) a = atomicAdd(&ctl[0], 1);
    a = __builtin_amdgcn_readfirstlane(a);
    if (a >= nnK) break;
    const int fp = __builtin_amdgcn_readfirstlane(partner[a]);
    if (fp < 0) continue;
    const int kb0 = __builtin_amdgcn_readfirstlane(kOffs[a]);
    const int ke0 = __builtin_amdgcn_readfirstlane(kOffs[a + 1]);
    const int fb0 = __builtin_amdgcn_readfirstlane(fOffs[fp]);
    const int fc = __builtin_amdgcn_readfirstlane(fOffs[fp + 1]) - fb0;
    if (fc <= 0) continue;
    const bool fast = fc <= 64;
    // the frame's node in registers (fast path): a feature per lane
    int myF = 0;
    ulonglong4 dF = make_ulonglong4(0, 0, 0, 0);
    float aF = 0.0f;
    bool avail = false;
    if (fast && lane < fc) {
      myF = (int)fFeats[fb0 + lane];
      dF = load_desc(fDesc + (size_t)myF * 32);
      aF = fKeys[myF].angle;
      avail = true;
    }
    for (int c = kb0; c < ke0; c += 64) {
      // 64 keyframe features of the node, a feature per lane
      int kf = 0;
      ulonglong4 dK = make_ulonglong4(0, 0, 0, 0);
      float aK = 0.0f;
      bool ok = false;
      if (c + lane < ke0) {
        kf = (int)kFeats[c + lane];
        const int pi = PI[kf];
        ok = pi >= 0 && !(PTS && PTS[pi].bad);  // :204-209
        if (ok) {
          dK = load_desc(kDesc + (size_t)kf * 32);
          aK = kKeys[kf].angle;
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
            const int rf = (int)fFeats[fb0 + t];
            if (fmatch[rf] >= 0) continue;  // :222-223
            const int dist = hamming256(q, load_desc(fDesc + (size_t)rf * 32));
            if (dist < d1) { d2 = d1; d1 = dist; q1 = t; }
            else if (dist < d2) { d2 = dist; }
          }
          const int key = wave_min((d1 << 16) | q1);
          best1 = key >> 16;
          pos = key & 0xFFFF;
          win = pos & 63;  // position t is scanned by lane t & 63
          best2 = wave_min(lane == win ? d2 : d1);
        }
        if (best1 <= BB_TH_LOW && (float)best1 < P.nnratio * (float)best2) {  // :239-241
          const int kfj = __builtin_amdgcn_readlane(kf, j);
          const float akj = __builtin_bit_cast(
              float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, aK), j));
          if (lane == win) {
            int rf = myF;
            float af = aF;
            if (!fast) {
              rf = (int)fFeats[fb0 + pos];
              af = fKeys[rf].angle;
            }
            const int bin = P.checkOri ? rot_bin(akj - af) : 0;  // :247-258
            fmatch[rf] = kfj | (bin << 24);
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

  // ---- rotation filter (:265-281), the gate and the outputs
  int ind1 = -1, ind2 = -1, ind3 = -1;
  if (P.checkOri) three_maxima(hist, ind1, ind2, ind3);
  int accepted = 0, removed = 0;
  for (int i = tid; i < nF; i += BB_T) {
    const int e = fmatch[i];
    if (e < 0) continue;
    ++accepted;
    const int b = e >> 24;
    if (P.checkOri && b != ind1 && b != ind2 && b != ind3) {
      ++removed;
      fmatch[i] = -1;
    }
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
  for (int i = tid; i < nF; i += BB_T) {
    const int e = fmatch[i];
    KM[i] = (enough && e >= 0) ? PI[e & 0xFFFFFF] : -1;
  }
  if (tid == 0) {
    info[p].n_matches = nm;
    info[p].n_accepted = ctl[3];
    info[p].n_common_nodes = ctl[2];
    info[p].n_tried = ctl[1];
    info[p].enough = enough;
  }
}

// dynamic LDS of one k_bow_batch workgroup at `stride` keypoint slots
static size_t bow_batch_lds(int stride) {
  return 8 * (((size_t)stride + 3) & ~(size_t)3);
}

extern "C" int orb_k_bow_batch_max_stride(void) {
  // 8 B per slot plus the static part within 160 KiB; the match word holds 24
  // index bits
  int s = (int)((ORB_LDS_PER_CU - BB_STATIC_LDS) / 8) & ~3;
  while (bow_batch_lds(s) + BB_STATIC_LDS > ORB_LDS_PER_CU) s -= 4;
  return std::min(s, (1 << 24) - 4);
}

extern "C" hipError_t orb_k_bow_batch(const BowBatchParams* params, int32_t* kpMatch,
                                      orb_bow_match_info_t* info, hipStream_t s) {
  const BowBatchParams P = *params;
  if (P.stride <= 0 || P.stride > orb_k_bow_batch_max_stride()) return hipErrorInvalidValue;
  const size_t lds = bow_batch_lds(P.stride);
  if (lds > 65536 - BB_STATIC_LDS) {
    hipError_t e = hipFuncSetAttribute((const void*)k_bow_batch,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_bow_batch, dim3(P.nProblems), dim3(BB_T), lds, s, P, kpMatch, info);
  return hipGetLastError();
}

// ================================== SearchForTriangulation as a device batch
// src/ORBmatcher.cc:718-901 for the neighbour loop of
// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:313-318): one
// workgroup of eight waves per (KF1, KF2) problem, one launch for validation,
// the epipole, matching, the rotation filter and the outputs.  vbMatched2 is
// never set, so every KF1 keypoint is independent and so is every (KF1
// keypoint, KF2 candidate) pair: the waves draw KF1 nodes from an LDS counter
// and spread the node's c1 x c2 pairs over their lanes, so that a node of
// eight features on either side is one trip of 64 lanes, not eight trips of
// eight.  A passing pair leaves (dist << 20) | (0xFFFFF - position in KF2's
// feature list) in the KF1 keypoint's LDS word by atomicMin: the minimum is
// the last passing candidate of minimum distance (k_tri_match's key).  The
// words become KF2 index | rotation bin << 24 once the matching is over; the
// partner table of the node join is dead by then and counts the matches per
// KF2 keypoint (n_shared2).
#define TB_T BB_T  // the FeatureVector checks above stride by BB_T
#define TB_STATIC_LDS ((size_t)1024)  // hist[32], ctl[8], two level tables and the block vote
#define TB_NONE 0xFFFFFFFFu

// ComputeThreeMaxima (src/ORBmatcher.cc:1765-1809) as three_maxima states it,
// with the if / else-if chain written as selects (max1 >= max2 >= max3, so
// s > max1 implies s > max2 implies s > max3): the chain's index shuffle ends
// up in scratch memory, this form stays in registers.
__device__ __forceinline__ void tb_three_maxima(const int* h, int& ind1, int& ind2, int& ind3) {
  int max1 = 0, max2 = 0, max3 = 0;
  ind1 = ind2 = ind3 = -1;
#pragma unroll 1
  for (int i = 0; i < 30; ++i) {
    const int s = h[i];
    const bool g1 = s > max1, g2 = s > max2, g3 = s > max3;
    max3 = g2 ? max2 : (g3 ? s : max3);
    ind3 = g2 ? ind2 : (g3 ? i : ind3);
    max2 = g1 ? max1 : (g2 ? s : max2);
    ind2 = g1 ? ind1 : (g2 ? i : ind2);
    max1 = g1 ? s : max1;
    ind1 = g1 ? i : ind1;
  }
  if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
  else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
}

__global__ __launch_bounds__(TB_T) void k_tri_batch(TriBatchParams P, int32_t* __restrict__ match12,
                                                    orb_tri_match_info_t* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
  __shared__ int hist[32];
  __shared__ int ctl[8];  // next node, tried, common nodes, accepted, removed, shared, undefined
  __shared__ float lvScale[ORB_MAX_LEVELS], lvSigma2[ORB_MAX_LEVELS];
  static_assert(sizeof(hist) + sizeof(ctl) + sizeof(lvScale) + sizeof(lvSigma2) + 256 <=
                    TB_STATIC_LDS, "capacity rule counts these");
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int S = (P.stride + 3) & ~3;
  uint32_t* mword = dyn;            // per KF1 keypoint: the match key, then KF2 index | bin << 24
  int* partner = (int*)(dyn + S);   // per KF1 node: position of KF2's node, -1 none; then
  int* cnt2 = partner;              // per KF2 keypoint: final matches that name it

  const int s1 = P.kf1Slot[p], s2 = P.kf2Slot[p];
  const size_t b1 = (size_t)s1 * P.stride, b2 = (size_t)s2 * P.stride;
  const int n1 = min(max(P.kf.nkeys[s1], 0), P.stride);
  const int n2 = min(max(P.kf.nkeys[s2], 0), P.stride);
  const int nn1 = min(max(P.kf.nFvNodes[s1], 0), n1);
  const int nn2 = min(max(P.kf.nFvNodes[s2], 0), n2);
  const orb_keypoint_t* K1 = P.kf.keys + b1;
  const uint8_t* D1 = P.kf.desc + b1 * 32;
  const uint32_t* N1 = P.kf.fvNodes + b1;
  const int32_t* O1 = P.kf.fvOffs + (size_t)s1 * ((size_t)P.stride + 1);
  const uint32_t* F1 = P.kf.fvFeats + b1;
  const int32_t* PI1 = P.pointIndex + b1;
  const float* UR1 = P.uRight ? P.uRight + b1 : nullptr;
  const orb_keypoint_t* K2 = P.kf.keys + b2;
  const uint8_t* D2 = P.kf.desc + b2 * 32;
  const uint32_t* N2 = P.kf.fvNodes + b2;
  const int32_t* O2 = P.kf.fvOffs + (size_t)s2 * ((size_t)P.stride + 1);
  const uint32_t* F2 = P.kf.fvFeats + b2;
  const int32_t* PI2 = P.pointIndex + b2;
  const float* UR2 = P.uRight ? P.uRight + b2 : nullptr;
  int32_t* M12 = match12 + (size_t)p * P.stride;

  // ---- malformed slots, as k_bow_batch finds them
  int bad = bb_bad_offsets(O1, nn1, n1, tid) | bb_bad_offsets(O2, nn2, n2, tid);
  bad = __syncthreads_or(bad);
  if (!bad) {
    bad = bb_bad_feats(O1, F1, nn1, n1, tid) | bb_bad_feats(O2, F2, nn2, n2, tid);
    bad = __syncthreads_or(bad);
  }
  if (bad) {
    for (int i = tid; i < n1; i += TB_T) M12[i] = -1;
    if (tid == 0) {
      info[p].n_matches = -1;
      info[p].n_accepted = 0;
      info[p].n_common_nodes = 0;
      info[p].n_tried = 0;
      info[p].n_shared2 = 0;
      info[p].n_undefined = 0;
    }
    return;
  }

  // ---- the epipole of KF1 in KF2 (:728-733), the arithmetic of the one-problem
  // entry: C2 = R2w * Cw + t2w row by row, invz = 1.0f / C2z
  float ex, ey, F[9];
  {
    const orb_pose_t* p1 = P.pose + s1;
    const orb_pose_t* p2 = P.pose + s2;
    const float cwx = p1->ow[0], cwy = p1->ow[1], cwz = p1->ow[2];
    const float c2x = fb_row(p2->rcw, 0, cwx, cwy, cwz, p2->tcw[0]);
    const float c2y = fb_row(p2->rcw, 1, cwx, cwy, cwz, p2->tcw[1]);
    const float c2z = fb_row(p2->rcw, 2, cwx, cwy, cwz, p2->tcw[2]);
    const float invz = __fdiv_rn(1.0f, c2z);
    ex = P.fx * c2x * invz + P.cx;
    ey = P.fy * c2y * invz + P.cy;
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = P.f12[(size_t)p * 9 + i];
  }

  for (int i = tid; i < n1; i += TB_T) mword[i] = TB_NONE;
  if (tid < 32) hist[tid] = 0;
  if (tid < 8) ctl[tid] = 0;
  if (tid < ORB_MAX_LEVELS) {
    lvScale[tid] = P.scale[tid];
    lvSigma2[tid] = P.sigma2[tid];
  }
  __syncthreads();
  {
    const int common = wave_sum(bb_join_nodes(N1, nn1, N2, nn2, partner, tid));
    if (lane == 0 && common) atomicAdd(&ctl[2], common);
  }
  __syncthreads();

  // ---- matching: a wave per KF1 node, lanes over its (KF1, KF2) feature pairs
  int tried = 0, undefined = 0;
  for (;;) {
    int a = 0;
    if (lane == 0) a = atomicAdd(&ctl[0], 1);
    a = __builtin_amdgcn_readfirstlane(a);
    if (a >= nn1) break;
    const int fp = __builtin_amdgcn_readfirstlane(partner[a]);
    if (fp < 0) continue;
    const int k0 = __builtin_amdgcn_readfirstlane(O1[a]);
    const int c1 = __builtin_amdgcn_readfirstlane(O1[a + 1]) - k0;
    const int f0 = __builtin_amdgcn_readfirstlane(O2[fp]);
    const int c2 = __builtin_amdgcn_readfirstlane(O2[fp + 1]) - f0;
    for (int t = lane; t < c1; t += 64) {  // the outer loop's tests alone (:768-778)
      const int idx1 = (int)F1[k0 + t];
      const bool st1 = UR1 && UR1[idx1] >= 0;
      tried += PI1[idx1] < 0 && (st1 || !P.onlyStereo);
    }
    if (c1 <= 0 || c2 <= 0) continue;
    const int total = c1 * c2;  // <= stride^2 < 2^31 (orb_k_tri_batch_max_stride)
    for (int t = lane; t < total; t += 64) {
      const int i = (int)((unsigned)t / (unsigned)c2), j = t - i * c2;
      const int idx1 = (int)F1[k0 + i];
      if (PI1[idx1] >= 0) continue;  // :768-772
      const bool st1 = UR1 && UR1[idx1] >= 0;
      if (P.onlyStereo && !st1) continue;
      const int idx2 = (int)F2[f0 + j];
      if (PI2[idx2] >= 0) continue;  // :792-797
      const bool st2 = UR2 && UR2[idx2] >= 0;
      if (P.onlyStereo && !st2) continue;
      const int dist = hamming256(load_desc(D1 + (size_t)idx1 * 32),
                                  load_desc(D2 + (size_t)idx2 * 32));
      if (dist > 50) continue;  // TH_LOW, and bestDist starts there (:784, :809)
      const orb_keypoint_t kp2 = K2[idx2];
      if (kp2.octave < 0 || kp2.octave >= P.nLevels) {  // the reference reads past mvScaleFactors
        ++undefined;
        continue;
      }
      if (!st1 && !st2) {  // :814-821
        const float dx = ex - kp2.x, dy = ey - kp2.y;
        if (dx * dx + dy * dy < 100 * lvScale[kp2.octave]) continue;
      }
      const float x1 = K1[idx1].x, y1 = K1[idx1].y;
      const float la = x1 * F[0] + y1 * F[3] + F[6];  // epipolar line (:147-149)
      const float lb = x1 * F[1] + y1 * F[4] + F[7];
      const float lc = x1 * F[2] + y1 * F[5] + F[8];
      const float den = la * la + lb * lb;
      if (den == 0) continue;
      const float num = la * kp2.x + lb * kp2.y + lc;
      const float dsqr = __fdiv_rn(num * num, den);
      if (!((double)dsqr < 3.84 * (double)lvSigma2[kp2.octave])) continue;
      atomicMin(&mword[idx1], ((uint32_t)dist << 20) | (uint32_t)(0xFFFFF - (f0 + j)));
    }
  }
  tried = wave_sum(tried);
  undefined = wave_sum(undefined);
  if (lane == 0) {
    if (tried) atomicAdd(&ctl[1], tried);
    if (undefined) atomicAdd(&ctl[6], undefined);
  }
  __syncthreads();

  // ---- the winners: KF2 index and rotation bin per KF1 keypoint (:830-850)
  int accepted = 0;
  for (int i = tid; i < n1; i += TB_T) {
    const uint32_t key = mword[i];
    if (key == TB_NONE) continue;
    ++accepted;
    const int idx2 = (int)F2[0xFFFFF - (int)(key & 0xFFFFFu)];
    const int bin = P.checkOri ? rot_bin(K1[i].angle - K2[idx2].angle) : 0;
    if (P.checkOri) atomicAdd(&hist[bin], 1);
    mword[i] = (uint32_t)idx2 | ((uint32_t)bin << 24);
  }
  for (int i = tid; i < n2; i += TB_T) cnt2[i] = 0;  // the partner table is dead
  accepted = wave_sum(accepted);
  if (lane == 0 && accepted) atomicAdd(&ctl[3], accepted);
  __syncthreads();

  // ---- rotation filter (:867-886) and the row
  int ind1 = -1, ind2 = -1, ind3 = -1;
  if (P.checkOri) tb_three_maxima(hist, ind1, ind2, ind3);
  int removed = 0;
  for (int i = tid; i < n1; i += TB_T) {
    const uint32_t e = mword[i];
    int m = -1;
    if (e != TB_NONE) {
      const int b = (int)(e >> 24);
      if (P.checkOri && b != ind1 && b != ind2 && b != ind3) {
        ++removed;
        mword[i] = TB_NONE;
      } else {
        m = (int)(e & 0xFFFFFFu);
        atomicAdd(&cnt2[m], 1);
      }
    }
    M12[i] = m;
  }
  removed = wave_sum(removed);
  if (lane == 0 && removed) atomicAdd(&ctl[4], removed);
  __syncthreads();
  int shared = 0;
  for (int i = tid; i < n1; i += TB_T) {
    const uint32_t e = mword[i];
    shared += e != TB_NONE && cnt2[e & 0xFFFFFFu] > 1;
  }
  shared = wave_sum(shared);
  if (lane == 0 && shared) atomicAdd(&ctl[5], shared);
  __syncthreads();
  if (tid == 0) {
    info[p].n_matches = ctl[3] - ctl[4];
    info[p].n_accepted = ctl[3];
    info[p].n_common_nodes = ctl[2];
    info[p].n_tried = ctl[1];
    info[p].n_shared2 = ctl[5];
    info[p].n_undefined = ctl[6];
  }
}

// dynamic LDS of one k_tri_batch workgroup at `stride` keypoint slots
static size_t tri_batch_lds(int stride) {
  return 8 * (((size_t)stride + 3) & ~(size_t)3);
}

extern "C" int orb_k_tri_batch_max_stride(void) {
  // 8 B per slot plus the static part within 160 KiB; the match key holds 20
  // position bits, the match word 24 index bits
  int s = (int)((ORB_LDS_PER_CU - TB_STATIC_LDS) / 8) & ~3;
  while (tri_batch_lds(s) + TB_STATIC_LDS > ORB_LDS_PER_CU) s -= 4;
  return std::min(s, (1 << 15) - 4);
}

extern "C" hipError_t orb_k_tri_batch(const TriBatchParams* params, int32_t* match12,
                                      orb_tri_match_info_t* info, hipStream_t s) {
  const TriBatchParams P = *params;
  if (P.stride <= 0 || P.stride > orb_k_tri_batch_max_stride() || P.nLevels < 1 ||
      P.nLevels > ORB_MAX_LEVELS)
    return hipErrorInvalidValue;
  const size_t lds = tri_batch_lds(P.stride);
  if (lds > 65536 - TB_STATIC_LDS) {
    hipError_t e = hipFuncSetAttribute((const void*)k_tri_batch,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_tri_batch, dim3(P.nProblems), dim3(TB_T), lds, s, P, match12, info);
  return hipGetLastError();
}

// ------------------------------------------ TrackLocalMap's two small tails
// After SearchByProjection(F, localMap): the local matcher's matches (indices
// into the problem's local map) become global point indices in the frame's
// match array, F.mvpMapPoints[bestIdx] = pMP (src/ORBmatcher.cc:127).  A
// keypoint is one entry of both arrays, so no two writes meet.
__global__ __launch_bounds__(256) void k_track_local_merge(
    int stride, int mpStride, const int32_t* __restrict__ nkeys,
    const int32_t* __restrict__ kmLocal, const int32_t* __restrict__ localIndex,
    int32_t* __restrict__ kpMatch) {
  const int p = blockIdx.x;
  const int n = min(max(nkeys[p], 0), stride);
  const int32_t* KL = kmLocal + (size_t)p * stride;
  const int32_t* LI = localIndex + (size_t)p * (size_t)mpStride;
  int32_t* KM = kpMatch + (size_t)p * stride;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int l = KL[i];
    if (l >= 0) KM[i] = LI[l];
  }
}

extern "C" hipError_t orb_k_track_local_merge(int nProblems, int stride, int mpStride,
                                              const int32_t* nkeys, const int32_t* kmLocal,
                                              const int32_t* localIndex, int32_t* kpMatch,
                                              hipStream_t s) {
  hipLaunchKernelGGL(k_track_local_merge, dim3(nProblems), dim3(256), 0, s, stride, mpStride,
                     nkeys, kmLocal, localIndex, kpMatch);
  return hipGetLastError();
}

// src/Tracking.cc:1109-1135 after PoseOptimization: mnMatchesInliers, and
// (nullOutliers: mSensor == System::STEREO) the outliers' points set to NULL.
__global__ __launch_bounds__(256) void k_track_local_finish(
    int stride, long long ptStride, int onlyTracking, int nullOutliers,
    const int32_t* __restrict__ nkeys, int32_t* __restrict__ kpMatch,
    const uint8_t* __restrict__ outlier, const orb_map_point_t* __restrict__ points,
    int32_t* __restrict__ nInliers) {
  __shared__ int cnt;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(nkeys[p], 0), stride);
  int32_t* KM = kpMatch + (size_t)p * stride;
  const uint8_t* OL = outlier + (size_t)p * stride;
  const orb_map_point_t* PTS = points + (size_t)p * (size_t)ptStride;
  if (tid == 0) cnt = 0;
  __syncthreads();
  int inl = 0;
  for (int i = tid; i < n; i += 256) {
    const int pi = KM[i];
    if (pi < 0) continue;
    if (!OL[i]) {
      if (onlyTracking || PTS[pi].has_obs) ++inl;  // :1120-1129
    } else if (nullOutliers) {
      KM[i] = -1;  // :1131-1132
    }
  }
  inl = wave_sum(inl);
  if ((tid & 63) == 0 && inl) atomicAdd(&cnt, inl);
  __syncthreads();
  if (tid == 0) nInliers[p] = cnt;
}

extern "C" hipError_t orb_k_track_local_finish(int nProblems, int stride, long long ptStride,
                                               int onlyTracking, int nullOutliers,
                                               const int32_t* nkeys, int32_t* kpMatch,
                                               const uint8_t* outlier,
                                               const orb_map_point_t* points, int32_t* nInliers,
                                               hipStream_t s) {
  hipLaunchKernelGGL(k_track_local_finish, dim3(nProblems), dim3(256), 0, s, stride, ptStride,
                     onlyTracking, nullOutliers, nkeys, kpMatch, outlier, points, nInliers);
  return hipGetLastError();
}
