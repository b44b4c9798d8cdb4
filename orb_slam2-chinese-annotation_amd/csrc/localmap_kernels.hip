// localmap_kernels.hip -- Tracking::UpdateLocalMap (src/Tracking.cc:1395-1404)
// as a device-resident batch: UpdateLocalKeyFrames (:1437-1558), then
// UpdateLocalPoints (:1407-1434), with the already-matched marking of
// SearchLocalPoints' first loop (:1333-1354), over a map view that lives in
// device memory (orb_map_view_t).
//
// k_local_map: one workgroup of sixteen waves per problem.
//   vote     a keypoint per thread; a bad point is nulled, every other point
//            adds one to the LDS counter of each keyframe that observes it
//   voted    the counters are read in rank order (kf_by_rank), so the ordered
//            list of voted keyframes is a block scan over rank space, not a
//            sort; pKFmax is the smallest rank among the largest counts
//   stage    what the neighbour pass can read of the first 80 voted keyframes
//            (ten covisibles, sixteen children, the parent: ranks, -1 for a
//            bad or missing one) is loaded by all threads at once into LDS
//   pass     wave 0 replays the serial loop, going straight to the next keyframe
//            that can add anything: per visited keyframe one LDS read per
//            lane, the included bitmap (by rank) and two wave-wide picks;
//            nothing on the chain is loaded from global memory unless a
//            keyframe has more than sixteen children
//   union    a wave per local keyframe: atomicMin of the concatenated slot
//            position into a per-problem table keyed by point id, a count of
//            the first occurrences per keyframe, a block scan, the ordered
//            scatter of the indices, then the 36 B + 32 B gather, a point per
//            thread
// The table is an LDS hash table while the problem's slots name at most
// LM_HASH_CAP distinct points; a problem with more runs the union again on a
// table indexed by point id in the handle's device scratch (LocalMapParams::
// table), which it clears itself for the ids it is about to touch.
#include <algorithm>

#include "orb_device.h"
#include "orb_kernels.h"

#define LM_T 1024
#define LM_NW (LM_T / 64)
#define LM_HASH 12288      // LDS hash entries (key + position word each)
#define LM_HASH_CAP 9216   // distinct ids it takes: the load factor stays <= 3/4, and the
                           // LM_T inserts that may be in flight past the cap still find a slot
#define LM_VISIT 80        // the pass breaks once the list holds more than 80 (:1498)
#define LM_NEIGH 10        // GetBestCovisibilityKeyFrames(10) (:1503)
#define LM_CHILD 16        // children staged per visited keyframe
#define LM_STAGE_WORDS (LM_VISIT * (LM_NEIGH + LM_CHILD + 3))
#define LM_STATIC_LDS ((size_t)512)  // budget for ctl[16], the scan scratch and the block vote
#define LM_U 8             // slots a lane takes per chunk (two chunks are in flight)
#define LM_HELD 0x80000000u
#define LM_OK 0x40000000u
#define LM_POS 0x3FFFFFFFu
static_assert(LM_HASH - LM_HASH_CAP > LM_T, "inserts in flight past the cap must find a slot");

enum { LC_NULLED, LC_NVOTED, LC_MAX, LC_REF, LC_LEN, LC_DISTINCT, LC_OVF, LC_TOTAL };

// per-keyframe slots of the dynamic LDS: kf_stride + 1 offsets, rounded to a bitmap word
static __host__ __device__ inline size_t lm_kr(int kfStride) {
  return ((size_t)kfStride + 32) & ~(size_t)31;
}
// dynamic LDS of one k_local_map workgroup at `kfStride` keyframe slots
static size_t local_map_lds(int kfStride) {
  const size_t KR = lm_kr(kfStride);
  return (size_t)8 * LM_HASH + (size_t)4 * LM_STAGE_WORDS + 12 * KR + KR / 8;
}

__device__ __forceinline__ void lm_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Minimum over the 64 lanes (all active), wave-uniform (track_kernels.hip's
// wave_min: the DPP steps of wave_incl_scan with min).
__device__ __forceinline__ int lm_wave_min(int v) {
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false));  // row_shr:1
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false));  // row_shr:2
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false));  // row_shr:4
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false));  // row_shr:8
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false));  // row_bcast:15
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false));  // row_bcast:31
  return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ uint32_t lm_hash(int id) {
  return __umulhi((uint32_t)id * 2654435761u, (uint32_t)LM_HASH);
}

// The per-problem table "point id -> smallest concatenated slot position":
// SCRATCH false: the LDS hash (keys, pos); true: tab[id] in device memory, read
// and written past this CU's L1 (agent-scope atomics and loads).  A word is
// the position (30 bits, LM_POS when absent) | LM_OK (its first occurrence is
// not bad) | LM_HELD (a keypoint of this frame holds the point).
template <bool SCRATCH>
struct LmTable {
  int* keys;
  uint32_t* pos;
  uint32_t* tab;
  int* ctl;

  __device__ __forceinline__ void insert(int id, uint32_t q) const {
    if constexpr (SCRATCH) {
      atomicMin(&tab[id], q);
    } else {
      uint32_t h = lm_hash(id);
      for (;;) {
        int k = keys[h];
        if (k == -1) {
          k = atomicCAS(&keys[h], -1, id);
          if (k == -1) {
            if (atomicAdd(&ctl[LC_DISTINCT], 1) >= LM_HASH_CAP) ctl[LC_OVF] = 1;
            k = id;
          }
        }
        if (k == id) {
          atomicMin(&pos[h], q);
          return;
        }
        h = h + 1 == LM_HASH ? 0 : h + 1;
      }
    }
  }
  // the word of `id`, null when the table does not have it
  __device__ __forceinline__ uint32_t* find(int id) const {
    if constexpr (SCRATCH) {
      return &tab[id];
    } else {
      uint32_t h = lm_hash(id);
      for (;;) {
        const int k = keys[h];
        if (k == id) return &pos[h];
        if (k == -1) return nullptr;
        h = h + 1 == LM_HASH ? 0 : h + 1;
      }
    }
  }
  __device__ __forceinline__ uint32_t load(const uint32_t* w) const {
    if constexpr (SCRATCH) return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *w;
  }
  // The words of LM_U ids at once (null: id < 0 or absent): the first probes
  // are independent LDS reads, only a collision walks on alone.
  __device__ __forceinline__ void find_all(const int (&id)[LM_U], uint32_t* (&w)[LM_U]) const {
    if constexpr (SCRATCH) {
#pragma unroll
      for (int u = 0; u < LM_U; ++u) w[u] = id[u] >= 0 ? &tab[id[u]] : nullptr;
    } else {
      uint32_t h[LM_U];
      int k[LM_U];
#pragma unroll
      for (int u = 0; u < LM_U; ++u) {
        h[u] = lm_hash(max(id[u], 0));
        k[u] = keys[h[u]];
      }
#pragma unroll
      for (int u = 0; u < LM_U; ++u) {
        while (id[u] >= 0 && k[u] != id[u] && k[u] != -1) {
          h[u] = h[u] + 1 == LM_HASH ? 0 : h[u] + 1;
          k[u] = keys[h[u]];
        }
        w[u] = (id[u] >= 0 && k[u] == id[u]) ? &pos[h[u]] : nullptr;
      }
    }
  }
  // their values (LM_POS for a null word), the reads independent too
  __device__ __forceinline__ void load_all(uint32_t* const (&w)[LM_U], uint32_t (&v)[LM_U]) const {
#pragma unroll
    for (int u = 0; u < LM_U; ++u) v[u] = w[u] ? load(w[u]) : LM_POS;
  }
  __device__ __forceinline__ void hold(int id) const {
    uint32_t* w = find(id);
    if (w && (load(w) & LM_POS) != LM_POS) atomicOr(w, LM_HELD);
  }
};

// Block exclusive scan of v[0..n) in place (LDS), all threads; returns the sum.
// Ends with a barrier: every thread may read any v[i] afterwards.
__device__ __forceinline__ int lm_scan_inplace(int* v, int n, int* tmp) {
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += LM_T) {
    const int i = i0 + (int)threadIdx.x;
    const int x = i < n ? v[i] : 0;
    int tot;
    const int ex = block_excl_scan(x, tmp, &tot);
    if (i < n) v[i] = base + ex;
    base += tot;
  }
  __syncthreads();
  return base;
}

// The local keyframes' slots in chunks of 64 * LM_U, a wave per keyframe
// (keyframe e, e + LM_NW, ...): body(e, q0, c, s0, id) gets the chunk that
// starts at slot s0 of keyframe e (c slots, the first at concatenated position
// q0) with id[u] = the point in slot s0 + 64 u + lane, -1 past the end.  The
// next chunk's ids are loaded before the body runs on this one.  body returns
// false to stop the wave.
template <typename F>
__device__ __forceinline__ void lm_for_chunks(const int32_t* __restrict__ kfMp, int L,
                                              const int* base, const int* offs, F body) {
  const int lane = threadIdx.x & 63;
  int e = threadIdx.x >> 6, s0 = 0;
  if (e >= L) return;
  auto fetch = [&](int fe, int fs, int (&id)[LM_U]) {
    const int lo = base[fe], c = offs[fe + 1] - offs[fe];
#pragma unroll
    for (int u = 0; u < LM_U; ++u) {
      const int s = fs + u * 64 + lane;
      id[u] = s < c ? kfMp[lo + s] : -1;
    }
  };
  int cur[LM_U], nxt[LM_U];
  fetch(e, 0, cur);
  for (;;) {
    const int q0 = offs[e], c = offs[e + 1] - q0;
    int ne = e, ns = s0 + 64 * LM_U;
    if (ns >= c) { ne = e + LM_NW; ns = 0; }
    const bool more = ne < L;
    if (more) fetch(ne, ns, nxt);
    if (!body(e, q0, c, s0, cur) || !more) return;
    e = ne;
    s0 = ns;
#pragma unroll
    for (int u = 0; u < LM_U; ++u) cur[u] = nxt[u];
  }
}

// UpdateLocalPoints over the L local keyframes (:1407-1434) with the `seen`
// marking (:1333-1354); base[e] is keyframe e's first kf_mp slot, offs its
// first concatenated position.  A bad point is never appended and so never
// taken (:1424-1431): the union is the first occurrence of every id whose
// point is not bad.  Returns false (SCRATCH == false only) when the LDS table
// met more than LM_HASH_CAP distinct ids: nothing has been written then.
template <bool SCRATCH>
__device__ bool lm_union(const LocalMapParams& P, int p, int n, int L, const int* base, int* offs,
                         int* cnt, const LmTable<SCRATCH>& T, int* ctl, int* tmp) {
  const orb_map_view_t& V = P.view;
  const int tid = threadIdx.x, lane = tid & 63;
  const int32_t* KM = P.kpMatch + (size_t)p * P.kpStride;

  if constexpr (SCRATCH) {
    // the ids this problem is about to touch start absent
    lm_for_chunks(V.kf_mp, L, base, offs, [&](int, int, int, int, const int (&id)[LM_U]) {
#pragma unroll
      for (int u = 0; u < LM_U; ++u)
        if (id[u] >= 0)
          __hip_atomic_store(&T.tab[id[u]], LM_POS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return true;
    });
    for (int i = tid; i < n; i += LM_T) {
      const int pi = KM[i];
      if (pi >= 0) __hip_atomic_store(&T.tab[pi], LM_POS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  } else {
    for (int i = tid; i < LM_HASH; i += LM_T) {
      T.keys[i] = -1;
      T.pos[i] = LM_POS;
    }
  }
  for (int i = tid; i < L; i += LM_T) cnt[i] = 0;
  __syncthreads();

  // ---- the first occurrence of every id: the smallest concatenated position
  lm_for_chunks(V.kf_mp, L, base, offs, [&](int, int q0, int, int s0, const int (&id)[LM_U]) {
#pragma unroll
    for (int u = 0; u < LM_U; ++u) {  // a thread adds at most one id past the cap
      if (!SCRATCH && *(volatile int*)&ctl[LC_OVF]) return false;
      if (id[u] >= 0) T.insert(id[u], (uint32_t)(q0 + s0 + u * 64 + lane));
    }
    return true;
  });
  __syncthreads();
  if (!SCRATCH && ctl[LC_OVF]) return false;

  // ---- points a keypoint of this frame holds (after the nulling)
  for (int i = tid; i < n; i += LM_T) {
    const int pi = KM[i];
    if (pi >= 0) T.hold(pi);
  }
  __syncthreads();

  // ---- first occurrences that are not bad: marked LM_OK, counted per keyframe
  lm_for_chunks(V.kf_mp, L, base, offs, [&](int e, int q0, int, int s0, const int (&id)[LM_U]) {
    uint32_t* w[LM_U];
    uint32_t v[LM_U];
    uint8_t bad[LM_U];
    T.find_all(id, w);
    T.load_all(w, v);
#pragma unroll
    for (int u = 0; u < LM_U; ++u)
      if ((v[u] & LM_POS) != (uint32_t)(q0 + s0 + u * 64 + lane)) w[u] = nullptr;
#pragma unroll
    for (int u = 0; u < LM_U; ++u) bad[u] = w[u] ? V.points[id[u]].bad : 1;
    int k = 0;
#pragma unroll
    for (int u = 0; u < LM_U; ++u)
      if (!bad[u]) {
        atomicOr(w[u], LM_OK);
        ++k;
      }
    k = wave_sum(k);
    if (lane == 0 && k) cnt[e] += k;  // keyframe e is this wave's alone
    return true;
  });
  __syncthreads();
  const int total = lm_scan_inplace(cnt, L, tmp);
  if (tid == 0) ctl[LC_TOTAL] = total;

  // ---- the ordered scatter of the indices
  const size_t mb = (size_t)p * (size_t)P.mpStride;
  int32_t* LI = P.localIndex + mb;
  uint32_t* REC = (uint32_t*)(P.mps + mb);
  uint4* DSC = (uint4*)(P.mpDesc + mb * 32);
  const unsigned long long below = (1ull << lane) - 1ull;
  int run = 0;
  lm_for_chunks(V.kf_mp, L, base, offs, [&](int e, int q0, int, int s0, const int (&id)[LM_U]) {
    if (s0 == 0) run = cnt[e];
    if (run >= P.mpStride) return true;
    uint32_t* wp[LM_U];
    uint32_t wv[LM_U];
    T.find_all(id, wp);
    T.load_all(wp, wv);
#pragma unroll
    for (int u = 0; u < LM_U; ++u) {
      const uint32_t w = wv[u];
      const bool first = (w & LM_POS) == (uint32_t)(q0 + s0 + u * 64 + lane) && (w & LM_OK);
      const unsigned long long b = __ballot(first);
      const int out = run + __popcll(b & below);
      run += __popcll(b);
      if (first && out < P.mpStride) LI[out] = id[u];
    }
    return true;
  });
  __syncthreads();

  // ---- the gather, a local point per thread: 36 B + 32 B, `seen` from the table
  const int nout = min(total, P.mpStride);
  for (int j = tid; j < nout; j += LM_T) {
    const int id = LI[j];
    const uint32_t w = T.load(T.find(id));
    const uint32_t* src = (const uint32_t*)(V.points + id);
    const uint4* ds = (const uint4*)(V.mp_desc + (size_t)id * 32);
    uint32_t r[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) r[q] = src[q];
    const uint4 d0 = ds[0], d1 = ds[1];
    // bad | seen << 8 | has_obs << 16 | _pad << 24: seen is this frame's own
    r[8] = (r[8] & ~0xFF00u) | ((w & LM_HELD) ? 0x100u : 0u);
    uint32_t* dst = REC + (size_t)j * 9;
#pragma unroll
    for (int q = 0; q < 9; ++q) dst[q] = r[q];
    DSC[(size_t)j * 2] = d0;
    DSC[(size_t)j * 2 + 1] = d1;
  }
  return true;
}

__global__ __launch_bounds__(LM_T) void k_local_map(LocalMapParams P) {
  extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];
  __shared__ int ctl[16];
  __shared__ int tmp[20];
  static_assert(sizeof(ctl) + sizeof(tmp) + 256 <= LM_STATIC_LDS, "capacity rule counts these");
  static_assert(sizeof(orb_map_point_t) == 36, "the gather copies nine words");
  const orb_map_view_t& V = P.view;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int KR = (int)lm_kr(P.kfStride);
  int* hkeys = (int*)dyn;
  uint32_t* hpos = dyn + LM_HASH;
  int* offs = (int*)(dyn + 2 * LM_HASH);  // votes by keyframe, then the list's slot offsets
  int* list = offs + KR;                  // the local keyframes (~rank while the pass appends)
  int* cnt = list + KR;                   // first occurrences per local keyframe, then their scan
  uint32_t* incl = (uint32_t*)(cnt + KR); // mnTrackReferenceForFrame == this frame, by rank
  int* stNb = (int*)(incl + KR / 32);     // [LM_VISIT][LM_NEIGH] covisible ranks
  int* stCh = stNb + LM_VISIT * LM_NEIGH; // [LM_VISIT][LM_CHILD] child ranks
  int* stPar = stCh + LM_VISIT * LM_CHILD;
  int* stChLo = stPar + LM_VISIT;
  int* stChN = stChLo + LM_VISIT;

  const int nKf = P.nKf;
  const int n = min(max(P.nkeys[p], 0), P.kpStride);
  int32_t* KM = P.kpMatch + (size_t)p * P.kpStride;
  uint8_t* LK = P.locked + (size_t)p * P.kpStride;
  int32_t* OUTKF = P.localKf + (size_t)p * P.kfStride;

  for (int i = tid; i < nKf; i += LM_T) offs[i] = 0;
  for (int i = tid; i < KR / 32; i += LM_T) incl[i] = 0u;
  if (tid < 16) ctl[tid] = tid == LC_REF ? 0x7FFFFFFF : 0;
  __syncthreads();

  // ---- the vote (:1441-1460) and the local matcher's locks
  {
    int nulled = 0;
    for (int i = tid; i < n; i += LM_T) {
      const int pi = KM[i];
      uint8_t lk = 0;
      if (pi >= 0) {
        // bad | seen << 8 | has_obs << 16, and the observation list, in one round
        const uint32_t flags = ((const uint32_t*)(V.points + pi))[8];
        const int o0 = V.mp_obs_offs[pi], o1 = V.mp_obs_offs[pi + 1];
        if (flags & 0xFFu) {
          KM[i] = -1;
          ++nulled;
        } else {
          lk = (flags & 0xFF0000u) != 0;
          for (int o = o0; o < o1; o += 8) {
            int kf[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) kf[u] = o + u < o1 ? V.mp_obs[o + u] : -1;
#pragma unroll
            for (int u = 0; u < 8; ++u)
              if (kf[u] >= 0) atomicAdd(&offs[kf[u]], 1);
          }
        }
      }
      LK[i] = lk;
    }
    nulled = wave_sum(nulled);
    if (lane == 0 && nulled) atomicAdd(&ctl[LC_NULLED], nulled);
  }
  __syncthreads();

  // ---- the voted keyframes in rank order (:1472-1489)
  int nv = 0;
  {
    int nVoted = 0, bestV = 0, bestR = 0x7FFFFFFF;
    for (int r0 = 0; r0 < nKf; r0 += LM_T) {
      const int r = r0 + tid;
      int kf = -1, v = 0;
      bool good = false;
      if (r < nKf) {
        kf = V.kf_by_rank[r];
        v = offs[kf];
        if (v > 0) {
          ++nVoted;
          good = !V.kf_bad[kf];
        }
      }
      int tot;
      const int ex = block_excl_scan(good ? 1 : 0, tmp, &tot);
      if (good) {
        list[nv + ex] = kf;
        atomicOr(&incl[r >> 5], 1u << (r & 31));
        if (v > bestV) { bestV = v; bestR = r; }  // ranks ascend per thread: the first of its maxima
      }
      nv += tot;
    }
    nVoted = wave_sum(nVoted);
    if (lane == 0 && nVoted) atomicAdd(&ctl[LC_NVOTED], nVoted);
    if (bestV > 0) atomicMax(&ctl[LC_MAX], bestV);
    __syncthreads();
    if (bestV > 0 && bestV == ctl[LC_MAX]) atomicMin(&ctl[LC_REF], bestR);
    __syncthreads();
  }
  const int nVotedAll = ctl[LC_NVOTED];
  const bool kept = nVotedAll == 0;  // :1462: the list stays as it was
  int L;
  if (kept) {
    L = min(max(P.nLocalKf[p], 0), P.kfStride);
    for (int i = tid; i < L; i += LM_T) list[i] = OUTKF[i];
  } else {
    // ---- what the pass reads of the keyframes it can visit
    const int nvis = min(nv, LM_VISIT);
    for (int idx = tid; idx < nvis * 32; idx += LM_T) {
      const int j = idx >> 5, s = idx & 31, kf = list[j];
      if (s < LM_NEIGH) {
        const int c0 = V.kf_cov_offs[kf], c1 = V.kf_cov_offs[kf + 1];
        int val = -1;
        if (c0 + s < c1) {
          const int nb = V.kf_cov[c0 + s];
          if (!V.kf_bad[nb]) val = V.kf_rank[nb];
        }
        stNb[j * LM_NEIGH + s] = val;
      } else if (s == LM_NEIGH) {
        const int par = V.kf_parent[kf];
        stPar[j] = par >= 0 ? V.kf_rank[par] : -1;  // isBad() is not consulted (:1538-1547)
      } else if (s == LM_NEIGH + 1) {
        const int c0 = V.kf_child_offs[kf];
        stChLo[j] = c0;
        stChN[j] = V.kf_child_offs[kf + 1] - c0;
      } else if (s >= 16) {
        const int c0 = V.kf_child_offs[kf], c1 = V.kf_child_offs[kf + 1], c = s - 16;
        int val = -1;
        if (c0 + c < c1) {
          const int ch = V.kf_child[c0 + c];
          if (!V.kf_bad[ch]) val = V.kf_rank[ch];
        }
        stCh[j * LM_CHILD + c] = val;
      }
    }
    __syncthreads();

    // ---- the neighbour pass (:1494-1550) over the voted keyframes, wave 0:
    // lanes 0-9 hold the covisibles, 16-31 the children, 32 the parent
    if (wave == 0) {
      int len = nv, j = 0;
      while (j < nv && len <= 80) {  // :1498 (len <= 80 here means every j < nv is staged)
        // The included set only grows, so a keyframe none of whose candidates is
        // free now adds nothing later either: go straight to the first one at or
        // after j that can add (slot 11 stands for a child list read from memory).
        int jn = 0x7FFFFFFF;
        for (int idx = j * 32 + lane; idx < nv * 32; idx += 64) {
          const int jj = idx >> 5, sl = idx & 31;
          int c = -1;
          bool hit = false;
          if (sl < LM_NEIGH) c = stNb[jj * LM_NEIGH + sl];
          else if (sl == LM_NEIGH) c = stPar[jj];
          else if (sl == LM_NEIGH + 1) hit = stChN[jj] > LM_CHILD;
          else if (sl >= 16) c = stCh[jj * LM_CHILD + sl - 16];
          if (hit || (c >= 0 && !((incl[c >> 5] >> (c & 31)) & 1u))) {
            jn = jj;
            break;
          }
        }
        jn = lm_wave_min(jn);
        if (jn >= nv) break;
        j = jn;
        const int chN = stChN[j], par = stPar[j];  // with the candidates: one LDS round
        int cand = -1;
        if (lane < LM_NEIGH) cand = stNb[j * LM_NEIGH + lane];
        else if (lane >= 16 && lane < 16 + LM_CHILD) cand = stCh[j * LM_CHILD + lane - 16];
        const bool isFree = cand >= 0 && !((incl[cand >> 5] >> (cand & 31)) & 1u);
        const bool parFree = par >= 0 && !((incl[par >> 5] >> (par & 31)) & 1u);
        const unsigned long long fb = __ballot(isFree);
        // the first covisible that is not bad and not included (:1505-1520)
        int nb = -1;
        if (fb & 0x3FFull)
          nb = __builtin_amdgcn_readlane(cand, (int)__builtin_ctzll(fb & 0x3FFull));
        // std::set<KeyFrame*> order: the child of smallest rank (:1522-1536)
        int key = 0x7FFFFFFF;
        if (chN <= LM_CHILD) {
          if (lane >= 16 && isFree && cand != nb) key = cand;
        } else {
          const int c0 = stChLo[j];
          for (int c = lane; c < chN; c += 64) {
            const int ch = V.kf_child[c0 + c];
            if (V.kf_bad[ch]) continue;
            const int r = V.kf_rank[ch];
            if (r != nb && !((incl[r >> 5] >> (r & 31)) & 1u)) key = min(key, r);
          }
        }
        key = lm_wave_min(key);
        const int child = key == 0x7FFFFFFF ? -1 : key;
        const bool parAdd = parFree && par != nb && par != child;
        if (lane == 0) {
          int at = len;
          if (nb >= 0) { list[at++] = ~nb; incl[nb >> 5] |= 1u << (nb & 31); }
          if (child >= 0) { list[at++] = ~child; incl[child >> 5] |= 1u << (child & 31); }
          if (parAdd) { list[at++] = ~par; incl[par >> 5] |= 1u << (par & 31); }
        }
        len += (nb >= 0) + (child >= 0) + (parAdd ? 1 : 0);
        lm_wave_sync();
        if (parAdd) break;  // :1546 leaves the outer loop
        ++j;
      }
      if (lane == 0) ctl[LC_LEN] = len;
    }
    __syncthreads();
    L = ctl[LC_LEN];
    for (int i = nv + tid; i < L; i += LM_T) list[i] = V.kf_by_rank[~list[i]];
    __syncthreads();
    for (int i = tid; i < L; i += LM_T) OUTKF[i] = list[i];
    if (tid == 0) P.nLocalKf[p] = L;
  }
  __syncthreads();

  // ---- the list's slot offsets (the votes are dead); the list itself has been
  // written out and becomes each keyframe's first kf_mp slot
  for (int i = tid; i < L; i += LM_T) {
    const int kf = list[i];
    const int lo = V.kf_mp_offs[kf];
    offs[i] = V.kf_mp_offs[kf + 1] - lo;
    list[i] = lo;
  }
  __syncthreads();
  {
    const int slots = lm_scan_inplace(offs, L, tmp);
    if (tid == 0) offs[L] = slots;
  }
  __syncthreads();

  const LmTable<false> TL{hkeys, hpos, nullptr, ctl};
  if (!lm_union<false>(P, p, n, L, list, offs, cnt, TL, ctl, tmp)) {
    const LmTable<true> TS{nullptr, nullptr, (uint32_t*)P.table + (size_t)p * (size_t)P.nMp, ctl};
    lm_union<true>(P, p, n, L, list, offs, cnt, TS, ctl, tmp);
  }
  __syncthreads();

  if (tid == 0) {
    const int total = ctl[LC_TOTAL];
    P.nmps[p] = min(total, P.mpStride);
    orb_local_map_info_t o;
    o.n_local_kf = L;
    o.n_voted = nVotedAll;
    o.n_added = kept ? 0 : L - nv;
    o.ref_kf = (kept || ctl[LC_REF] == 0x7FFFFFFF) ? -1 : V.kf_by_rank[ctl[LC_REF]];
    o.max_votes = ctl[LC_MAX];
    o.n_local_points = total;
    o.n_nulled = ctl[LC_NULLED];
    o.kept = kept ? 1 : 0;
    P.info[p] = o;
  }
}

extern "C" int orb_k_local_map_max_keyframes(void) {
  // 12 B and one bit per keyframe slot (+ 1, rounded up to 32) beside the hash
  // table, the staged neighbourhoods and the static part, within 160 KiB
  int k = (int)((ORB_LDS_PER_CU - LM_STATIC_LDS - 8 * LM_HASH - 4 * LM_STAGE_WORDS) / 12);
  while (k > 0 && local_map_lds(k) + LM_STATIC_LDS > ORB_LDS_PER_CU) --k;
  return k;
}

extern "C" int orb_k_local_map_hash_cap(void) { return LM_HASH_CAP; }

extern "C" hipError_t orb_k_local_map(const LocalMapParams* params, hipStream_t s) {
  const LocalMapParams P = *params;
  if (P.kfStride < P.nKf || P.kfStride > orb_k_local_map_max_keyframes())
    return hipErrorInvalidValue;
  const size_t lds = local_map_lds(P.kfStride);
  hipError_t e = hipFuncSetAttribute((const void*)k_local_map,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_local_map, dim3(P.nProblems), dim3(LM_T), lds, s, P);
  return hipGetLastError();
}
