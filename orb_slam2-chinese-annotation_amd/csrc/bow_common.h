// bow_common.h -- device helpers shared by the SearchByBoW batches
// (k_bow_batch and k_tri_batch in track_kernels.hip, k_bow_kf_batch in
// sim3chain_kernels.hip): the wave-wide minimum, the 64-bit lane broadcast, the
// FeatureVector checks and the merge-join on node id.
#pragma once
#include "matcher_common.h"

#ifndef BB_T
#define BB_T 512  // eight waves (128, 256 and 1024 measured beside it)
#endif

// Minimum over the 64 lanes (all active), wave-uniform: the DPP steps of
// wave_incl_scan with min; a lane whose source is outside its row keeps v.
__device__ __forceinline__ int wave_min(int v) {
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false));  // row_shr:1
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false));  // row_shr:2
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false));  // row_shr:4
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false));  // row_shr:8
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false));  // row_bcast:15
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false));  // row_bcast:31
  return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ unsigned long long lane_bcast64(unsigned long long v, int srcLane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, srcLane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), srcLane);
  return ((unsigned long long)hi << 32) | lo;
}

// One FeatureVector's offsets: non-negative, non-decreasing, none above count.
__device__ __forceinline__ int bb_bad_offsets(const int32_t* offs, int nNodes, int count, int tid) {
  int bad = 0;
  if (nNodes > 0)
    for (int i = tid; i <= nNodes; i += BB_T) {
      const int o = offs[i];
      bad |= (o < 0 || o > count);
      if (i < nNodes) bad |= (offs[i + 1] < o);
    }
  return bad;
}
// Its feature indices, once the offsets are known to be good.
__device__ __forceinline__ int bb_bad_feats(const int32_t* offs, const uint32_t* feats, int nNodes,
                                            int count, int tid) {
  int bad = 0;
  if (nNodes > 0)
    for (int q = offs[0] + tid; q < offs[nNodes]; q += BB_T) bad |= (feats[q] >= (uint32_t)count);
  return bad;
}
// The merge-join on node id, a node of the first FeatureVector per thread:
// partner[a] = the position in bNodes of the node with aNodes[a]'s id, -1 none.
// Returns this thread's count of common nodes.
__device__ __forceinline__ int bb_join_nodes(const uint32_t* aNodes, int na, const uint32_t* bNodes,
                                             int nb, int* partner, int tid) {
  int common = 0;
  for (int a = tid; a < na; a += BB_T) {
    const uint32_t id = aNodes[a];
    int lo = 0, hi = nb;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (bNodes[mid] < id) lo = mid + 1; else hi = mid;
    }
    const bool found = lo < nb && bNodes[lo] == id;
    partner[a] = found ? lo : -1;
    common += found;
  }
  return common;
}
