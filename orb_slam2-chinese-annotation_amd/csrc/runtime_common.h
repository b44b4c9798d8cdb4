// runtime_common.h -- what the host runtime's files share (internal; the C ABI
// is include/orb_abi.h): error and profiling macros, the call-order rule
// (CallOrder, MatcherCall), device and pinned buffers, the stage profiler,
// stream helpers, and the handle structs: the stereo entry points read the
// extractor's single-frame state, the keyframe database holds a vocabulary.
// Every helper here has internal linkage (static inline, or the anonymous
// namespace): none of them is an export of the library.
#ifndef ORB_RUNTIME_COMMON_H
#define ORB_RUNTIME_COMMON_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <mutex>
#include <shared_mutex>
#include <cmath>
#include <unordered_map>
#include <vector>

#include "../../include/orb_abi.h"
#include "orb_kernels.h"
#include "orb_resize_tables.h"  // cvRoundF, satShort

namespace {

#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t _e = (expr);                             \
    if (_e != hipSuccess) {                             \
      if (getenv("ORB_AMD_DEBUG"))                      \
        fprintf(stderr, "[orb_amd] %s:%d %s -> %s\n", __FILE__, __LINE__, #expr, \
                hipGetErrorString(_e));                 \
      return _e == hipErrorOutOfMemory ? ORB_ENOMEM : ORB_EDEVICE; \
    }                                                   \
  } while (0)

static inline bool stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &cst) == hipSuccess && cst != hipStreamCaptureStatusNone;
}

// Call order on one handle.  Every call reuses the handle's device scratch
// (the extractor's arena, cell keys and octree tables; the matcher's grid,
// candidate lists and claim buffers), and a batch call runs asynchronously on
// whatever stream its caller passes, so a call on a stream other than the
// previous call's makes its stream wait for that call first (on the device, no
// host synchronisation), and every call records where it ended.  The reference
// has the same rule in host form: an ORBextractor is not reentrant
// (include/ORBextractor.h:85), a Frame drives two instances concurrently
// (src/Frame.cc:81-84).  A stream being captured into a graph is left to the
// caller's ordering of the graph's launches.  (Growing a scratch buffer is
// safe on its own: hipFree synchronises the device.)
#ifndef ORB_CALL_ORDER
#define ORB_CALL_ORDER 1  // 0: no cross-stream waits (the ordering test's negative control only)
#endif
static inline bool must_wait(hipStream_t last, hipStream_t s) {
  return ORB_CALL_ORDER && last && last != s;
}
struct CallOrder {
  hipEvent_t ev;
  hipStream_t* last;
  hipStream_t s;
  bool capture;
  orb_status_t status = ORB_OK;
  CallOrder(hipEvent_t e, hipStream_t* l, hipStream_t st)
      : ev(e), last(l), s(st), capture(stream_capturing(st)) {
    if (!capture && must_wait(*last, s) && hipStreamWaitEvent(s, ev, 0) != hipSuccess)
      status = ORB_EDEVICE;
  }
  // the call synchronised its stream: nothing of it is pending any more
  void settled() {
    if (!capture) *last = nullptr;
    capture = true;
  }
  ~CallOrder() {
    if (!capture && hipEventRecord(ev, s) == hipSuccess) *last = s;
  }
};

// Wait for a stream whose results the caller reads next.  The synchronous
// entry points (one frame, one SearchByProjection) sit on the tracking
// thread's critical path, where hipStreamSynchronize returned 5-13 us after
// the stream's last operation (profiles/r06_dropin_timeline.txt); polling the
// stream returns within a query (~1 us) of it.  Bounded: past 2 ms of polling
// the wait blocks as hipStreamSynchronize does.
static inline hipError_t stream_wait(hipStream_t s) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned i = 1;; ++i) {
    const hipError_t e = hipStreamQuery(s);
    if (e != hipErrorNotReady) return e;
    if ((i & 63) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2))
      return hipStreamSynchronize(s);
  }
}

// Growable device buffer, freed with the handle that owns it (the handle's
// destroy function sets the device and drains its stream first).
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  orb_status_t ensure(size_t n) {
    if (n <= bytes) return ORB_OK;
    if (p) hipFree(p);
    p = nullptr;
    bytes = 0;
    if (hipMalloc(&p, n) != hipSuccess) return ORB_ENOMEM;
    bytes = n;
    return ORB_OK;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <typename T>
  T* as() const { return (T*)p; }
};

// Pinned host staging for the host-buffer API: one contiguous DMA each way
// (a 2-D copy from pageable memory goes row by row, ~7 us per row).
struct HostBuf {
  void* p = nullptr;
  size_t bytes = 0;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { release(); }
  orb_status_t ensure(size_t n) {
    if (n <= bytes) return ORB_OK;
    if (p) hipHostFree(p);
    p = nullptr;
    bytes = 0;
    if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) return ORB_ENOMEM;
    bytes = n;
    return ORB_OK;
  }
  void release() {
    if (p) hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <typename T>
  T* as() const { return (T*)p; }
};

// HIP-event timing of kernel stages on the stream they are launched on.  Each
// profiled call takes a fresh set of events from a pool (no synchronisation in
// the launch path); read() drains every recorded set and accumulates per-stage
// milliseconds, so a timed region of K calls is measured without perturbing it.
struct StageProfiler {
  // Per call: (begin, end) event pairs per stage -- up to maxSeg[stage]
  // segments, e.g. one per level for a stage launched level by level, whose
  // durations are summed -- recorded on whichever stream runs that stage
  // (stages may overlap), plus a (begin, end) pair for the whole call on the
  // caller's stream.
  static constexpr int kMaxStages = 8;
  bool enabled = false;
  bool serial = false;  // isolated timing: every stage on the caller's stream, one after another
  int nStages = 0;
  const char* names[kMaxStages] = {};
  int maxSeg[kMaxStages] = {1, 1, 1, 1, 1, 1, 1, 1};
  std::vector<std::vector<hipEvent_t>> pool;  // each: 2 * sum(maxSeg) + 2 events
  std::vector<std::vector<uint8_t>> segs;     // per call: segments recorded per stage
  size_t used = 0;
  double ms[kMaxStages + 1] = {};
  long launches[kMaxStages + 1] = {};
  int launchesPerCall[kMaxStages] = {};

  int base(int stage) const {
    int o = 0;
    for (int i = 0; i < stage; ++i) o += maxSeg[i];
    return o;
  }
  int total() const { return base(nStages); }
  void reset() {
    used = 0;
    for (int i = 0; i <= kMaxStages; ++i) { ms[i] = 0; launches[i] = 0; }
  }
  std::vector<hipEvent_t>* begin_call() {
    if (!enabled) return nullptr;
    if (used == pool.size()) {
      pool.emplace_back(2 * total() + 2);
      for (hipEvent_t& e : pool.back()) hipEventCreate(&e);
      segs.emplace_back(kMaxStages, 0);
    }
    std::fill(segs[used].begin(), segs[used].end(), (uint8_t)1);
    return &pool[used++];
  }
  // of the current call: stage not run / run as n segments
  void not_run(int stage) { segs[used - 1][stage] = 0; }
  void segments(int stage, int n) { segs[used - 1][stage] = (uint8_t)n; }
  hipEvent_t b(std::vector<hipEvent_t>* ev, int stage, int seg = 0) const {
    return (*ev)[2 * (base(stage) + seg)];
  }
  hipEvent_t e(std::vector<hipEvent_t>* ev, int stage, int seg = 0) const {
    return (*ev)[2 * (base(stage) + seg) + 1];
  }
  hipEvent_t t0(std::vector<hipEvent_t>* ev) const { return (*ev)[2 * total()]; }
  hipEvent_t t1(std::vector<hipEvent_t>* ev) const { return (*ev)[2 * total() + 1]; }
  void drain() {
    for (size_t c = 0; c < used; ++c) {
      std::vector<hipEvent_t>& ev = pool[c];
      if (hipEventSynchronize(t1(&ev)) != hipSuccess) continue;
      for (int i = 0; i < nStages; ++i) {
        if (launchesPerCall[i] == 0 || segs[c][i] == 0) continue;  // stage not run
        bool ok = true;
        double sum = 0;
        for (int g = 0; g < segs[c][i] && ok; ++g) {
          float t = 0.f;
          ok = hipEventElapsedTime(&t, b(&ev, i, g), e(&ev, i, g)) == hipSuccess;
          sum += t;
        }
        if (ok) {
          ms[i] += sum;
          launches[i] += launchesPerCall[i];
        } else {
          (void)hipGetLastError();  // clear it: torch checks the last error after its launches
        }
      }
      float t = 0.f;
      if (hipEventElapsedTime(&t, t0(&ev), t1(&ev)) == hipSuccess) {
        ms[nStages] += t;
        launches[nStages] += 1;
      }
    }
    used = 0;
  }
  void destroy() {
    for (auto& v : pool)
      for (hipEvent_t ev : v) hipEventDestroy(ev);
    pool.clear();
    segs.clear();
    used = 0;
  }
};

#define PROF_REC(ev, evt, strm) \
  do {                                            \
    if (ev) HIP_TRY(hipEventRecord((evt), (strm))); \
  } while (0)

inline orb_status_t check_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ORB_ENODEV;
  if (device < 0 || device >= n) return ORB_EINVAL;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ORB_EDEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    if (getenv("ORB_AMD_DEBUG")) fprintf(stderr, "[orb_amd] device %d is %s, need gfx950\n", device, prop.gcnArchName);
    return ORB_ENODEV;
  }
  return ORB_OK;
}

// The device's least stream priority: the handles' own streams take it (see
// create_own_stream).
static inline int least_stream_prio() {
  int lo = 0, hi = 0;
  hipDeviceGetStreamPriorityRange(&lo, &hi);
  return lo;
}

// A handle's own stream (single-frame calls, host-buffer matchers, readbacks,
// graph capture) at the device's least priority.  HIP backs the streams of a
// process by a few HSA queues per priority level and maps a new stream onto
// the least-used queue of its level; normal-priority streams a library
// creates early (ORB-SLAM2 builds its extractors and matchers at start-up)
// take normal queues the caller's own streams then share: a caller's
// high-priority stream ran 2x slower beside busy normal-priority streams
// after three idle normal streams had been created first, with or without
// this library (tools/probe/contention_probe.py, profiles/r05_contention.txt).
// The least priority keeps the library out of the pools the caller's streams
// use (the side stream has a queue of its own, a full-CU-mask stream).
static inline hipError_t create_own_stream(hipStream_t* s) {
  return hipStreamCreateWithPriority(s, hipStreamNonBlocking, least_stream_prio());
}

// Row pitch of the one-frame path's staged image (pinned and device): the
// width itself (the kernels take any stride), so a contiguous caller image is
// staged with one memcpy instead of one per row
static inline size_t one_stride(int width) {
  return (size_t)width;
}

static inline orb_status_t upload(DevBuf& b, const void* src, size_t n, hipStream_t s) {
  orb_status_t st = b.ensure(std::max<size_t>(n, 16));
  if (st) return st;
  if (n) HIP_TRY(hipMemcpyAsync(b.p, src, n, hipMemcpyHostToDevice, s));
  return ORB_OK;
}

}  // namespace

// ================================================================ extractor
struct orb_extractor {
  int device = 0;
  int nfeatures = 0, nlevels = 0, iniTh = 0, minTh = 0;
  float scaleFactorF = 1.2f;
  double scaleFactor = 1.2;
  std::vector<float> scale, invScale, sigma2, invSigma2;
  std::vector<int> quota;
  int umax[16];
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // the device's shared side stream: FAST beside the resize chain
  hipStream_t privSide = nullptr; // this handle's side stream while its caller's stream is captured
  hipEvent_t evL0Fork = nullptr, evL0Join = nullptr;  // level-0 FAST beside the resize chain
  hipEvent_t evLvl = nullptr;  // the resize chain has written level FAST_SIDE_LEVELS
  hipEvent_t evBatch = nullptr;  // recorded at the end of every run_batch on its stream
  hipStream_t lastStream = nullptr;  // the stream evBatch was last recorded on (null: none pending)
  bool ownStream = false;
  std::mutex mu;

  // plan for the current image size
  int planW = -1, planH = -1;
  OrbPlanDesc plan;
  std::vector<OrbCellDesc> cells;
  size_t cellClassOff = 0;  // byte offset of the OrbCellClass table inside dCells
  long long arenaBytes = 0, blurBytes = 0;
  int maxCellsPerLevel = 0, nodeCapMax = 0, ldsKeyCap = 0;
  int nResizePairs = 0;  // resize launches per call with the level pairs (PYR_PAIR_MAX_IMAGES)
  DevBuf dCells, dRtab, dTiles, dBands;

  // batch scratch
  int batchCap = 0;
  DevBuf dBlur;  // one image's blurred levels (orb_extractor_blurred_level, on demand)
  DevBuf dArena, dCellKeys, dCellCount, dGKeys, dGNid, dOutKeys, dOutCount, dErr;
  DevBuf dOctNodes;            // octree node tables in global memory (large nfeatures)
  long long octNodeBytes = 0;  // per (image, level) slice; 0: node tables in LDS
  // single-image API scratch
  // single-image API: dImg (the image at a 64-B row pitch) and dOne = [count,
  // pad x3 | cap keypoints | cap x 32 descriptors], mirrored by the pinned
  // hImg / hOut so each call is one DMA in and one DMA out
  DevBuf dImg, dOne;
  HostBuf hImg, hOut, hLvl;  // hLvl: staging of orb_extractor_pyramid_level / _blurred_level
  // host mirror of the single-frame call's levels 1.. (orb_extractor_host_pyramid):
  // once asked for, the arena's D2H joins every later call's graph
  HostBuf hPyr;
  bool pyrReadback = false, hPyrValid = false;
  int oneCap = 0;            // capacity of the dOne layout
  bool lastSingle = false;   // the last call was orb_extractor_extract (dOne is current)
  // the whole single-image call (H2D, every kernel, D2H) as one hipGraph per
  // plan; keyed by the buffers it captured (any reallocation re-captures)
  hipGraphExec_t oneExec = nullptr;
  std::vector<const void*> oneKey;
  int lastW = 0, lastH = 0;
  size_t lastImgStride = 0;
  const uint8_t* lastImg0 = nullptr;  // level 0 of the last batch (device)
  size_t lastImg0Pitch = 0;
  int lastImg0Stride = 0;

  // profiling: stages k_pyr_resize (x nlevels-1), k_blur_levels, k_fast_band, k_octree,
  // k_orient_desc
  StageProfiler prof;
};

// ================================================================== matcher
// orb_matcher::sx, the scratch of the projection-window variants (PP_*), of
// KF-KF SearchByBoW (BW_*) and of SearchForTriangulation (TR_*): three calls
// that never overlap name the same buffers.
enum MatcherSlot {
  PP_FRAME0 = 0, PP_FRAME1 = 4,  // two searched (key)frames: keys, desc, n, grid (PPFrame)
  PP_MPS = 8, PP_MPDESC, PP_VALID, PP_SKIP, PP_ANGLE, PP_URIGHT, PP_RECS, PP_TOPK, PP_NCAND,
  PP_BEST, PP_LOCKED, PP_KPMATCH, PP_COUNT, PP_BEST12, PP_BEST21, PP_MUTUAL, SX_COUNT,
  BW_DESC1 = 0, BW_ANGLE1, BW_MP1, BW_BAD1, BW_IDS1, BW_OFFS1, BW_FEATS1,
  BW_DESC2, BW_ANGLE2, BW_MP2, BW_BAD2, BW_IDS2, BW_OFFS2, BW_FEATS2, BW_MATCH, BW_ACC, BW_COUNT,
  TR_KEYS1 = 0, TR_DESC1, TR_UR1, TR_HASMP1, TR_IDS1, TR_OFFS1, TR_FEATS1,
  TR_KEYS2, TR_DESC2, TR_UR2, TR_HASMP2, TR_IDS2, TR_OFFS2, TR_FEATS2, TR_MATCH, TR_ACC, TR_COUNT
};

struct orb_matcher {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t evLast = nullptr;        // recorded where the last call ended (CallOrder)
  hipStream_t lastStream = nullptr;   // its stream (null: nothing pending)
  std::mutex mu;
  // profiling: stages k_grid_build, k_proj_candidates + k_proj_resolve
  StageProfiler prof;
  DevBuf dKeys, dDesc, dUr, dLocked, dNKeys, dMps, dMpDesc, dNMps, dCellStart, dCellIdx, dTopk,
      dNcand, dKpMatch, dNMatch, dA, dB, dOut;
  DevBuf dJac;  // Jacobi-resolve scratch (ORB_RESOLVE_JACOBI)
  DevBuf dCpKeys;  // k_close_points' key scratch for frames above CP_LDS_KEYS slots
  DevBuf dPoKeys, dPoUr, dPoIdx, dPoPts, dPoOut;  // orb_pose_optimization's staged frame
  DevBuf dPoRecs;  // k_pose_optimization's edge records for frames above PO_LDS_EDGES slots
  DevBuf dLmTable;  // k_local_map's first-occurrence table by point id (the scratch tier)
  DevBuf dOvf, dOvfCtr;  // candidate lists of SearchByProjection(F, localMap) (ProjParams.ovf)
  uint32_t ovfGen = 0;
  int stagedN = -1, stagedM = -1;  // orb_match_projection_local_stage's layout
  bool begun = false, begunStereo = false, begunLocked = false;  // _begin sent the frame's part
  int resolveSchedule = ORB_RESOLVE_AUTO;  // orb_matcher_set_resolve
  int jacobiRounds = 6;
  // stereo / frame / BoW scratch
  DevBuf dStRowStart, dStRowIdx;  // stereo vRowIndices (CSR per pair)
  DevBuf dProjStage;              // cell-ordered keypoints for k_proj_candidates (16 B per slot)
  DevBuf dRKeys, dRDesc, dNR, dPyr, dPairLv, dDepth, dSad, dBowA, dBowB, dBowC, dBowD, dBowE,
      dBowF, dBowG, dBowH, dBowI, dBowJ, dBowK;
  HostBuf hPyr;  // pinned staging of the host stereo pyramids (one DMA)
  // orb_match_projection_local: every input in one pinned block / one DMA, and
  // the matches + count back in one
  HostBuf hIn, hOutM;
  DevBuf dIn;
  // frustum scratch
  DevBuf dMapPts, dPose, dTracks, dNInView;
  // SearchForInitialization / ComputeDistinctiveDescriptors scratch
  DevBuf dK1, dD1, dK2, dD2, dN1, dN2, dPrev, dList, dM12, dOffs, dObsDesc, dBest, dBestDesc,
      dInitQ, dInitStage, dInitCounts;
  DevBuf sx[SX_COUNT];  // projection / triangulation / KF-KF BoW scratch (MatcherSlot)
  std::vector<uint8_t> hostScratch;
};

namespace {
// One call on a matcher handle that uses the handle's scratch: the handle's
// lock, its device, the stream the call runs on (the caller's, or the handle's
// own) and the call-order rule (CallOrder), in that order.  Members are
// destroyed in reverse, so the call's end is recorded before the lock is
// released.  An entry point that touches no handle scratch takes neither (the
// device-resident batches over caller-owned buffers only).
struct MatcherCall {
  std::lock_guard<std::mutex> lock;
  const hipStream_t s;
  CallOrder order;
  const orb_status_t status;  // not ORB_OK: the call must return it at once
  // (runs between taking the lock and the call-order wait)
  static hipStream_t on_device(orb_matcher* m, void* stream) {
    hipSetDevice(m->device);
    return stream ? (hipStream_t)stream : m->stream;
  }
  explicit MatcherCall(orb_matcher* m, void* stream = nullptr)
      : lock(m->mu),
        s(on_device(m, stream)),
        order(m->evLast, &m->lastStream, s),
        status(order.status) {}
  void settled() { order.settled(); }
  // the end of a synchronous call: its results are on the host when it returns
  orb_status_t finish() {
    HIP_TRY(stream_wait(s));
    settled();
    return ORB_OK;
  }
};
}  // namespace

// ------------------------------------------------------- DBoW2 vocabulary
// TemplatedVocabulary<FORB::TDescriptor, FORB> as loaded by loadFromTextFile
// (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1362-1448) and its transform
// (:1128-1283), the producer of Frame/KeyFrame::mBowVec and mFeatVec
// (src/Frame.cc:439-449, src/KeyFrame.cc:60-71).  The tree lives on the
// device, renumbered breadth-first (vocab_kernels.hip).  (Hidden: its implicit
// destructor, which frees the buffers, is no export of the library.)
struct __attribute__((visibility("hidden"))) orb_vocabulary {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  int k = 0, L = 0, scoring = 0, weighting = 0, nNodes = 0, nWords = 0;
  DevBuf dInfo, dDesc, dWord, dWeight, dOrig;
  DevBuf dIn, dCounts, dFWord, dFWeight, dFNode, dBowW, dBowV, dNW, dFvN, dFvO, dFvF, dNFv;
  DevBuf dScore[7];  // orb_vocabulary_score: a offs / words / values, b likewise, out
};

#endif  // ORB_RUNTIME_COMMON_H
