// placerec_kernels.hip -- gfx950 kernels of place recognition: DBoW2 BoW
// scoring (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-311) and the keyframe
// database queries (src/KeyFrameDatabase.cc:79-339: DetectLoopCandidates,
// DetectRelocalizationCandidates).
//
// Score.  score(a, b) walks the two std::maps in step and adds one term per
// common word to a double, in ascending word order.  Here a wave takes one
// pair: each lane looks one word of b up in a (binary search, both ascending)
// and evaluates its term, all 64 in parallel; the adds then run as one chain,
// lane by lane in ballot order, chunk after chunk, so every partial sum rounds
// exactly as the reference's `score +=` does.  No tree or wave reduction
// touches a double.
//
// Query.  The reference walks mvInvertedFile[w] for each query word w in
// ascending order and appends a keyframe to lKFsSharingWords the first time it
// meets it (:89-108, :214-236).  A keyframe is met first under its smallest
// shared word, and each inverted list is in add order (erase keeps the order
// of the rest, :51-70), so the list is the sharing keyframes sorted by
// (smallest shared word, add sequence number).  Database slots are handed out
// in add order and never reused, so the slot index is the sequence number:
//   k_db_common      a wave per slot: words shared with the query (ballot +
//                    popcount) = mnRelocWords / mnLoopWords, smallest shared word
//   k_db_list        one workgroup: bitonic sort of (first word << 32 | slot),
//                    maxCommonWords, minCommonWords = (int)(max * 0.8f)
//   k_db_score       a wave per listed keyframe with common > minCommonWords:
//                    si = (float)score(query, kf), stored as the keyframe's
//                    persistent mRelocScore / mLoopScore
//   k_db_accumulate  a thread per scored entry: the float chain over its <= 10
//                    stored covisibility neighbours (:152-178, :281-313)
//   k_db_select      one workgroup: bestAccScore, 0.75f * it, and the ordered
//                    compaction of each kept entry's best keyframe at its first
//                    occurrence (:181-198, :316-336)
#include "orb_device.h"
#include "orb_kernels.h"

#define PR_NONE 0xFFFFFFFFu
#define PR_LDS_KEYS 4096  // list keys sorted in LDS up to this many slots (32 KiB)
#define PR_Q_LDS 8192     // query words staged in LDS up to this many (32 KiB)

// ScoringType (BowVector.h:45-53)
#define PR_L1 0
#define PR_L2 1
#define PR_CHI 2
#define PR_KL 3
#define PR_BHAT 4
#define PR_DOT 5

// Index of w in the ascending words[0, n), or -1.
__device__ __forceinline__ int pr_find(const uint32_t* words, int n, uint32_t w) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (words[mid] < w) lo = mid + 1; else hi = mid;
  }
  return (lo < n && words[lo] == w) ? lo : -1;
}

// score(a, b) by one wave (all 64 lanes active, arguments wave-uniform);
// vi is a's value and wi is b's, as v1 / v2 in ScoringObject.cpp.
__device__ __forceinline__ double pr_score_wave(int type, const uint32_t* __restrict__ aw,
                                                const double* __restrict__ av, int na,
                                                const uint32_t* __restrict__ bw,
                                                const double* __restrict__ bv, int nb) {
  const int lane = lane_id();
  double score = 0;
  for (int base = 0; base < nb; base += ORB_WAVE) {
    const int j = base + lane;
    double term = 0.0;
    bool has = false;
    if (j < nb) {
      const int p = pr_find(aw, na, bw[j]);
      if (p >= 0) {
        const double vi = av[p], wi = bv[j];
        has = true;
        switch (type) {
          case PR_L1: term = fabs(vi - wi) - fabs(vi) - fabs(wi); break;        // :41
          case PR_CHI:                                                          // :148
            if (vi + wi != 0.0) term = vi * wi / (vi + wi); else has = false;
            break;
          case PR_BHAT: term = sqrt(vi * wi); break;                            // :245
          default: term = vi * wi; break;                                       // :91, :290
        }
      }
    }
    // the reference's `score += term`, one word after the other
    unsigned long long m = __ballot(has);
    while (m) {
      const int l = __ffsll((long long)m) - 1;
      m &= m - 1;
      score += __shfl(term, l);
    }
  }
  if (type == PR_L1) score = -score / 2.0;                                      // :65
  else if (type == PR_L2) score = score >= 1 ? 1.0 : 1.0 - sqrt(1.0 - score);   // :114-117
  else if (type == PR_CHI) score = 2. * score;                                  // :167
  return score;
}

// Pair p: a = words/values [aOffs[p], aOffs[p+1]), b likewise.  A wave per pair.
__global__ __launch_bounds__(256) void k_bow_score(
    int type, int nPairs, const int32_t* __restrict__ aOffs, const uint32_t* __restrict__ aWords,
    const double* __restrict__ aValues, const int32_t* __restrict__ bOffs,
    const uint32_t* __restrict__ bWords, const double* __restrict__ bValues,
    double* __restrict__ out) {
  const int p = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (p >= nPairs) return;  // wave-uniform
  const int a0 = aOffs[p], a1 = aOffs[p + 1], b0 = bOffs[p], b1 = bOffs[p + 1];
  const double s = pr_score_wave(type, aWords + a0, aValues + a0, a1 - a0, bWords + b0,
                                 bValues + b0, b1 - b0);
  if (lane_id() == 0) out[p] = s;
}

// Marks the slots of the query's connected keyframes (loop query).
__global__ void k_db_mark(const int32_t* __restrict__ slots, int n, uint8_t* __restrict__ flag) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) flag[slots[i]] = 1;
}

// One wave's pass over a keyframe's words W[0, len) against the ascending
// query words q[0, nq): the count of shared words and the smallest of them.
__device__ __forceinline__ void pr_common_wave(const uint32_t* __restrict__ W, int len,
                                               const uint32_t* q, int nq, int& cnt, uint32_t& fw) {
  const int lane = lane_id();
  for (int base = 0; base < len; base += ORB_WAVE) {
    const int j = base + lane;
    const uint32_t w = j < len ? W[j] : PR_NONE;
    const bool hit = j < len && pr_find(q, nq, w) >= 0;
    const unsigned long long m = __ballot(hit);
    if (m && fw == PR_NONE) fw = (uint32_t)__shfl((int)w, __ffsll((long long)m) - 1);
    cnt += __popcll(m);
  }
}

// A wave per slot: common[slot] = words shared with the query, first[slot] =
// the smallest of them, or PR_NONE when the keyframe does not share (no common
// word, erased, or connected to the query keyframe).  The query's words are
// staged in LDS when they fit (every lane searches them ~log2(nq) deep).
__global__ __launch_bounds__(256) void k_db_common(
    const PrSlot* __restrict__ slots, int nSlots, const uint32_t* __restrict__ words,
    const uint32_t* __restrict__ qWords, int nq, const uint8_t* __restrict__ connected,
    int32_t* __restrict__ common, uint32_t* __restrict__ first, int32_t* __restrict__ firstPos) {
  __shared__ uint32_t sQ[PR_Q_LDS];
  const bool staged = nq <= PR_Q_LDS;
  if (staged) {
    for (int i = threadIdx.x; i < nq; i += blockDim.x) sQ[i] = qWords[i];
    __syncthreads();
  }
  const int slot = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (slot >= nSlots) return;  // wave-uniform
  const PrSlot S = slots[slot];
  int cnt = 0;
  uint32_t fw = PR_NONE;
  if (S.live) {
    if (staged) pr_common_wave(words + S.off, S.len, sQ, nq, cnt, fw);
    else pr_common_wave(words + S.off, S.len, qWords, nq, cnt, fw);
  }
  if (lane_id() == 0) {
    common[slot] = cnt;
    first[slot] = (connected && connected[slot]) ? PR_NONE : fw;
    firstPos[slot] = 0x7FFFFFFF;
  }
}

// Bitonic sort of P (power of two) keys, ascending, by one workgroup: each
// work item owns one compare-exchange of a step.
__device__ __forceinline__ void pr_bitonic(unsigned long long* keys, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const unsigned long long a = keys[lo], b = keys[hi];
        if ((a > b) == ((lo & k) == 0)) {
          keys[lo] = b;
          keys[hi] = a;
        }
      }
      __syncthreads();
    }
  }
}

// Keys of the sharing slots (the others ~0), sorted; `keys` is LDS or global.
__device__ __forceinline__ void pr_list_sort(unsigned long long* keys, int nSlots, int P,
                                             const int32_t* __restrict__ common,
                                             const uint32_t* __restrict__ first, int& mx, int& cnt) {
  for (int i = threadIdx.x; i < P; i += blockDim.x) {
    unsigned long long key = ~0ull;
    if (i < nSlots && first[i] != PR_NONE) {
      key = ((unsigned long long)first[i] << 32) | (uint32_t)i;
      mx = max(mx, common[i]);  // :117-122, :243-249
      ++cnt;
    }
    keys[i] = key;
  }
  __syncthreads();
  pr_bitonic(keys, P);
}

// hdr: [0] list length, [1] maxCommonWords, [2] minCommonWords, [3] candidates.
// One workgroup.  gKeys = global scratch of P keys, used when P > PR_LDS_KEYS.
__global__ __launch_bounds__(1024) void k_db_list(
    int nSlots, int P, const int32_t* __restrict__ common, const uint32_t* __restrict__ first,
    unsigned long long* gKeys, uint32_t* __restrict__ list, int32_t* __restrict__ hdr) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long prKeys[];
  __shared__ int sMax, sCount;
  const bool inLds = P <= PR_LDS_KEYS;
  if (threadIdx.x == 0) { sMax = 0; sCount = 0; }
  __syncthreads();
  int mx = 0, cnt = 0;
  if (inLds) pr_list_sort(prKeys, nSlots, P, common, first, mx, cnt);
  else pr_list_sort(gKeys, nSlots, P, common, first, mx, cnt);
  atomicMax(&sMax, mx);
  atomicAdd(&sCount, cnt);
  __syncthreads();
  const unsigned long long* keys = inLds ? prKeys : gKeys;
  const int n = sCount;
  for (int i = threadIdx.x; i < n; i += blockDim.x) list[i] = (uint32_t)keys[i];
  if (threadIdx.x == 0) {
    hdr[0] = n;
    hdr[1] = sMax;
    hdr[2] = (int)((float)sMax * 0.8f);  // int minCommonWords = maxCommonWords*0.8f (:124, :251)
    hdr[3] = 0;
  }
}

// A wave per list entry: score it if it shares more than minCommonWords words.
__global__ __launch_bounds__(256) void k_db_score(
    int type, int nSlots, const PrSlot* __restrict__ slots, const uint32_t* __restrict__ words,
    const double* __restrict__ values, const uint32_t* __restrict__ qWords,
    const double* __restrict__ qValues, int nq, const int32_t* __restrict__ common,
    const uint32_t* __restrict__ list, const int32_t* __restrict__ hdr,
    float* __restrict__ stored, uint8_t* __restrict__ scored) {
  const int r = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (r >= nSlots || r >= hdr[0]) return;  // wave-uniform
  const uint32_t slot = list[r];
  const bool doit = common[slot] > hdr[2];  // :133, :262
  if (doit) {
    const PrSlot S = slots[slot];
    const double s = pr_score_wave(type, qWords, qValues, nq, words + S.off, values + S.off, S.len);
    if (lane_id() == 0) stored[slot] = (float)s;  // float si = mpVoc->score(...) (:137-139, :267-268)
  }
  if (lane_id() == 0) scored[r] = doit;
}

// A thread per list entry: accScore and pBestKF over the stored neighbours.
__global__ __launch_bounds__(256) void k_db_accumulate(
    int loop, float minScore, int nSlots, const int32_t* __restrict__ common,
    const uint32_t* __restrict__ first, const int32_t* __restrict__ neigh,
    const float* __restrict__ stored, const uint32_t* __restrict__ list,
    const int32_t* __restrict__ hdr, const uint8_t* __restrict__ scored,
    float* __restrict__ acc, uint32_t* __restrict__ best, uint8_t* __restrict__ valid) {
  const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (r >= nSlots || r >= hdr[0]) return;
  const uint32_t slot = list[r];
  const int minCommon = hdr[2];
  const float si = stored[slot];
  const bool ok = scored[r] && (!loop || si >= minScore);  // :140
  float bestScore = si, accScore = si;
  uint32_t bestSlot = slot;
  if (ok) {
    for (int j = 0; j < PR_NEIGH; ++j) {
      const int nb = neigh[(size_t)slot * PR_NEIGH + j];
      if (nb < 0) continue;                   // not in the database
      if (first[nb] == PR_NONE) continue;     // mnRelocQuery / mnLoopQuery != id (:164, :296)
      if (loop && !(common[nb] > minCommon)) continue;  // :164
      const float s2 = stored[nb];  // possibly an earlier query's score, as the reference reads
      accScore += s2;
      if (s2 > bestScore) {
        bestSlot = (uint32_t)nb;
        bestScore = s2;
      }
    }
  }
  acc[r] = accScore;
  best[r] = bestSlot;
  valid[r] = ok;
}

// One workgroup: bestAccScore, the retain threshold and the ordered output.
__global__ __launch_bounds__(1024) void k_db_select(
    float bestInit, const float* __restrict__ acc, const uint32_t* __restrict__ best,
    const uint8_t* __restrict__ valid, int32_t* firstPos, const long long* __restrict__ ids,
    int32_t* hdr, long long* __restrict__ out) {
  __shared__ float sBest[16];
  __shared__ int tmp[17];
  const int n = hdr[0];
  const int lane = lane_id(), wv = (int)(threadIdx.x >> 6);
  float b = bestInit;  // minScore (:149) or 0 (:278)
  for (int r = threadIdx.x; r < n; r += blockDim.x)
    if (valid[r] && acc[r] > b) b = acc[r];  // :176-177, :310-312
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) b = fmaxf(b, __shfl_xor(b, m));
  if (lane == 0) sBest[wv] = b;
  __syncthreads();
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) b = fmaxf(b, sBest[w]);
  const float minRetain = 0.75f * b;  // :181, :316
  // the first kept entry that elects each keyframe (spAlreadyAddedKF)
  for (int r = threadIdx.x; r < n; r += blockDim.x)
    if (valid[r] && acc[r] > minRetain) atomicMin(&firstPos[best[r]], r);
  __syncthreads();
  int emitted = 0;
  for (int base = 0; base < n; base += blockDim.x) {
    const int r = base + (int)threadIdx.x;
    bool emit = false;
    uint32_t slot = 0;
    if (r < n && valid[r] && acc[r] > minRetain) {
      slot = best[r];
      emit = __hip_atomic_load(&firstPos[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == r;
    }
    int total;
    const int pos = block_excl_scan(emit ? 1 : 0, tmp, &total);
    if (emit) out[emitted + pos] = ids[slot];
    emitted += total;
  }
  if (threadIdx.x == 0) hdr[3] = emitted;
}

extern "C" hipError_t orb_k_bow_score(int type, int nPairs, const int32_t* aOffs,
                                      const uint32_t* aWords, const double* aValues,
                                      const int32_t* bOffs, const uint32_t* bWords,
                                      const double* bValues, double* out, hipStream_t s) {
  if (nPairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_bow_score, dim3((unsigned)((nPairs + 3) / 4)), dim3(256), 0, s, type,
                     nPairs, aOffs, aWords, aValues, bOffs, bWords, bValues, out);
  return hipGetLastError();
}

// Scratch keys the list sort needs in global memory for nSlots slots (0: LDS).
extern "C" size_t orb_k_db_key_scratch(int nSlots) {
  size_t P = 1024;
  while (P < (size_t)nSlots) P <<= 1;
  return P <= PR_LDS_KEYS ? 0 : P;
}

extern "C" hipError_t orb_k_db_query(const PrQueryArgs* args, hipStream_t s) {
  const PrQueryArgs& A = *args;
  const int n = A.nSlots;
  if (n <= 0) return hipSuccess;
  const bool all = A.stage < 0;
  const unsigned waveBlocks = (unsigned)((n + 3) / 4);
  if (all && A.loop) {
    hipError_t e = hipMemsetAsync(A.connected, 0, (size_t)n, s);
    if (e != hipSuccess) return e;
    if (A.nConnected > 0)
      hipLaunchKernelGGL(k_db_mark, dim3((unsigned)((A.nConnected + 255) / 256)), dim3(256), 0, s,
                         A.connSlots, A.nConnected, A.connected);
  }
  if (all || A.stage == 0)
    hipLaunchKernelGGL(k_db_common, dim3(waveBlocks), dim3(256), 0, s, A.slots, n,
                       A.words, A.qWords, A.nq, A.loop ? A.connected : nullptr, A.common, A.first,
                       A.firstPos);
  if (all || A.stage == 1) {
    int P = 1024;
    while (P < n) P <<= 1;
    const size_t lds = P <= PR_LDS_KEYS ? (size_t)P * 8 : 0;
    hipLaunchKernelGGL(k_db_list, dim3(1), dim3(1024), lds, s, n, P, A.common, A.first, A.keys,
                       A.list, A.hdr);
  }
  if (all || A.stage == 2)
    hipLaunchKernelGGL(k_db_score, dim3(waveBlocks), dim3(256), 0, s, A.type, n,
                       A.slots, A.words, A.values, A.qWords, A.qValues, A.nq,
                       A.common, A.list, A.hdr, A.stored, A.scored);
  if (all || A.stage == 3)
    hipLaunchKernelGGL(k_db_accumulate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A.loop,
                       A.minScore, n, A.common, A.first, A.neigh, A.stored, A.list, A.hdr,
                       A.scored, A.acc, A.best, A.valid);
  if (all || A.stage == 4)
    hipLaunchKernelGGL(k_db_select, dim3(1), dim3(1024), 0, s, A.loop ? A.minScore : 0.0f, A.acc,
                       A.best, A.valid, A.firstPos, A.ids, A.hdr, A.out);
  return hipGetLastError();
}
