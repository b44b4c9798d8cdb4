// orb_kernel_params.h -- the parameter blocks and records the host runtime
// fills and the matcher / mapping / vocabulary / place-recognition / camera /
// depth kernels read: one definition for both sides, as orb_plan.h is for the
// extractor.  Plain C++ (no HIP): a host and a device compile both include it.
// The blocks marked "by value" are kernel arguments, so their names are part
// of the kernels' mangled symbols.
#pragma once
#include <stdint.h>

#include "../../include/orb_abi.h"

#ifndef ORB_MAX_LEVELS
#define ORB_MAX_LEVELS 16  // as orb_plan.h, orb_device.h
#endif

// ------------------------------------------------------ matcher_kernels.hip
// SearchByProjection(F, vpMapPoints) (by value).  ovf: the candidate lists of
// the map points with more than TOPK candidates (OVF_SLOTS, OVF_CAP:
// matcher_common.h).
struct ProjParams {
  float minX, minY, invW, invH;
  float th, nnratio;
  int nLevels;
  float scale[ORB_MAX_LEVELS];
  uint32_t* ovf;     // OVF_SLOTS x OVF_CAP entries per problem, or null (no lists)
  uint32_t* ovfCtr;  // per problem: the call's gen << 20 | slots taken
  uint32_t gen;      // 1..4095, a new value per call (no reset of ovfCtr needed)
};

// Frame::ComputeStereoMatches (by value)
struct StereoParams {
  int nLevels;
  float bf, fx;
  int w[ORB_MAX_LEVELS], h[ORB_MAX_LEVELS];
  int strideL[ORB_MAX_LEVELS], strideR[ORB_MAX_LEVELS];
  float scale[ORB_MAX_LEVELS], invScale[ORB_MAX_LEVELS];
};

// the pyramid levels of one stereo pair (device pointers; an array per call)
struct StereoPairLevels {
  const uint8_t* L[ORB_MAX_LEVELS];
  const uint8_t* R[ORB_MAX_LEVELS];
};

// SearchByProjection(CurrentFrame, LastFrame) (by value)
struct FrameProjParams {
  float minX, maxX, minY, maxY, invW, invH;
  float fx, fy, cx, cy, bf;
  float th;
  int fwd, bwd, checkOri;
  float scale[ORB_MAX_LEVELS];
};

// k_frustum (by value)
struct FrustumParams {
  float fx, fy, cx, cy, bf;
  float minX, maxX, minY, maxY;
  float cosLimit, logScale;
  int nLevels;
};

// --------------------------------------------------- projection_kernels.hip
// the projection-window variants (by value)
struct PPParams {
  float R[9], t[3], Ow[3];  // world -> camera of the searched frame (first stage)
  float R2[9], t2[3];       // SearchBySim3: camera A -> camera B (sR, t)
  float fx, fy, cx, cy, bf;
  float minX, maxX, minY, maxY, invW, invH;
  float th, logScale;
  int nLevels, thr, checkOri;
  float scale[ORB_MAX_LEVELS], invSigma2[ORB_MAX_LEVELS];
};

// projected point: position, predicted window and levels; valid = 0 when the
// reference skips the point before its window scan
struct PPRec {
  float u, v, ur, radius;
  int minL, maxL, valid, pad;
};

// SearchForTriangulation (by value)
struct TriParams {
  float F[9];
  float ex, ey;
  int onlyStereo, checkOri;
  float scale[ORB_MAX_LEVELS], sigma2[ORB_MAX_LEVELS];
};

// ------------------------------------------------------ mapping_kernels.hip
// SearchForInitialization (by value)
struct InitParams {
  float minX, minY, invW, invH;
  float r, nnratio;
  int checkOri;
};

// staged F2 keypoint: position, grid cell (ix << 16 | iy), original index
struct InitKey {
  float x, y;
  uint32_t cell;
  int32_t idx;
};

// -------------------------------------------------------- vocab_kernels.hip
struct VocNodeInfo {
  int32_t first;  // device position of the first child
  int32_t count;  // number of children (0 = Node::isLeaf)
};

// ------------------------------------------------------- camera_kernels.hip
// cv::undistortPoints' double parameter block (by value): cvConvert of the
// CV_32F matrices, ifx = 1./fx, RR = mK * I
struct UndistortParams {
  double fx, fy, cx, cy, ifx, ify;  // A = mK (double), ifx = 1./fx
  double rr[9];                     // RR = mK * I
  double k[12];                     // k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4
};
static_assert(sizeof(UndistortParams) == 27 * 8, "parameter block layout");

// -------------------------------------------------------- depth_kernels.hip
// Frame::ComputeStereoFromRGBD over n_frames x stride keypoint slots (by value)
struct RgbdParams {
  int nFrames, stride;
  int depthType;  // ORB_DEPTH_U16 / ORB_DEPTH_F32
  int convert;    // GrabImageRGBD's condition (src/Tracking.cc:229), evaluated on the host
  int cols, rows;
  long long rowBytes, imageBytes;
  float factor;  // mDepthMapFactor
  float bf;
};

// Frame::UnprojectStereo (by value): invfx = 1.0f / fx as src/Frame.cc:115
struct UnprojectParams {
  int nFrames, stride;
  float cx, cy, invfx, invfy;
};

// k_close_points sorts up to this many 8-byte keys in LDS (32 KiB; the next
// power of two, 64 KiB of keys plus the counters, exceeds the 64 KiB a
// workgroup gets without opting in)
#define CP_LDS_KEYS 4096

// ----------------------------------------------------- placerec_kernels.hip
#define PR_NEIGH 10  // covisibility neighbours stored per keyframe

struct PrSlot {
  long long off;  // first entry of the keyframe's BowVector in words / values
  int32_t len;    // its word count
  int32_t live;   // 0 once erased
};

// one keyframe database query: the database, the query, its scratch
struct PrQueryArgs {
  int type, loop;
  float minScore;
  int nSlots, nq, nConnected;
  const PrSlot* slots;
  const uint32_t* words;
  const double* values;
  const int32_t* neigh;
  const long long* ids;
  float* stored;
  const uint32_t* qWords;
  const double* qValues;
  const int32_t* connSlots;
  uint8_t* connected;
  int32_t* common;
  uint32_t* first;
  int32_t* firstPos;
  unsigned long long* keys;
  uint32_t* list;
  int32_t* hdr;
  uint8_t* scored;
  float* acc;
  uint32_t* best;
  uint8_t* valid;
  long long* out;
  int stage;  // -1: the whole query; 0..4: that kernel alone (isolated timing)
};

// --------------------------------------------------------- pose_kernels.hip
// k_pose_optimization keeps up to this many 32-byte edge records in LDS (32 KiB
// beside the 7.2 KiB term tile and 256 B for the sums: four workgroups per CU
// at 1,000 slots); frames with more keypoint slots keep them in the handle's
// device scratch
#define PO_LDS_EDGES 1024

// Optimizer::PoseOptimization over nProblems x stride keypoint slots (by value)
struct PoseOptParams {
  int nProblems, stride;
  int nSingle;             // the keypoint count when there is no count array
  int pointStrideBytes;    // bytes between two points (three floats each)
  long long ptStride;      // points between two problems' point arrays
  int nLevels;
  float invLevelSigma2[ORB_MAX_LEVELS];  // mvInvLevelSigma2
  float fx, fy, cx, cy, bf;
};

// -------------------------------------------------------- track_kernels.hip
// SearchByProjection(CurrentFrame, LastFrame) over nProblems x stride keypoint
// slots, poses and map points read on the device (by value)
struct FrameBatchParams {
  int nProblems, stride;
  long long mpStride;  // map points between two problems' arrays (0: one shared array)
  float minX, maxX, minY, maxY, invW, invH;
  float fx, fy, cx, cy, bf, mb;
  float th;
  int nLevels, mono, checkOri, retryBelow;
  float scale[ORB_MAX_LEVELS];
};

// One side's slot arrays of SearchByBoW(KF, F) as a batch: what
// orb_extractor_extract_batch and orb_vocabulary_transform_batch write, slot k
// at k * stride (desc x 32, fvOffs at k * (stride + 1))
struct BowSlots {
  const orb_keypoint_t* keys;
  const uint8_t* desc;
  const int32_t* nkeys;
  const uint32_t* fvNodes;
  const int32_t* fvOffs;
  const uint32_t* fvFeats;
  const int32_t* nFvNodes;
};

// SearchByBoW(pKF, F, vpMapPointMatches) over nProblems (by value)
struct BowBatchParams {
  int nProblems, stride;
  long long mpStride;          // map points between two problems' arrays (0: one shared array)
  const int32_t* kfIndex;      // keyframe / frame slot of problem p (null: p)
  const int32_t* fIndex;
  BowSlots kf, f;
  const int32_t* kfPointIndex; // mvpMapPoints per keyframe keypoint (< 0: NULL)
  const orb_map_point_t* points;  // null: no point is bad
  float nnratio;
  int checkOri, minMatches;
};

// SearchForTriangulation over nProblems (KF1, KF2) pairs of keyframe slots (by
// value): one set of slot arrays serves both sides
struct TriBatchParams {
  int nProblems, stride;
  const int32_t* kf1Slot;
  const int32_t* kf2Slot;
  BowSlots kf;
  const int32_t* pointIndex;   // mvpMapPoints per keypoint (>= 0: the keypoint is skipped)
  const float* uRight;         // null: every keypoint is monocular
  const orb_pose_t* pose;
  const float* f12;            // ComputeF12, nine floats per problem, row-major
  float fx, fy, cx, cy;        // pKF2
  int nLevels, onlyStereo, checkOri;
  float scale[ORB_MAX_LEVELS], sigma2[ORB_MAX_LEVELS];  // pKF2
};

// ----------------------------------------------------- localmap_kernels.hip
// Tracking::UpdateLocalMap over nProblems frames against one map view (by
// value): the view's device pointers, the per-problem arrays and strides
struct LocalMapParams {
  int nProblems;
  int nKf, nMp;
  int kpStride, kfStride, mpStride;
  orb_map_view_t view;
  const int32_t* nkeys;
  int32_t* kpMatch;       // in/out
  int32_t* localKf;       // in/out
  int32_t* nLocalKf;      // in/out
  int32_t* localIndex;
  orb_map_point_t* mps;
  uint8_t* mpDesc;
  int32_t* nmps;
  uint8_t* locked;
  orb_local_map_info_t* info;
  int32_t* table;         // the scratch tier's per-problem table, nMp entries each
};

// --------------------------------------------------------- sim3_kernels.hip
// Sim3Solver's constructor and SetRansacParameters over nProblems (by value)
struct Sim3SetupParams {
  int nProblems, stride;
  const int32_t* kf1Slot;  // null: p
  const int32_t* kf2Slot;
  const orb_keypoint_t* keys;
  const int32_t* nkeys;
  const int32_t* pointIndex;
  const orb_pose_t* pose;
  const orb_map_point_t* points;
  const int32_t* match12;
  const int32_t* index1;   // null: i1
  const int32_t* index2;
  int nLevels;
  float maxErr[ORB_MAX_LEVELS];  // (float)(uint64_t)(9.210 * sigma2) per level
  float k1[4], k2[4];            // fx, fy, cx, cy
  int fixScale, minInliers, maxIterations;
  double probability;            // mRansacProb (pinned_log(1 - p) is evaluated on the device)
  orb_sim3_state_t* state;
  orb_sim3_corr_t* corr;
};

// Sim3Solver::iterate over nProblems (by value)
struct Sim3IterParams {
  int nProblems, stride;
  orb_sim3_state_t* state;
  orb_sim3_corr_t* corr;
  const uint32_t* draws;
  int drawStride;
  uint32_t randMax;
  int maxIterations, nIterations;
  const uint8_t* active;  // null: every problem
  uint8_t* inliers12;
  orb_sim3_result_t* result;
};

// ------------------------------------------------------ sim3opt_kernels.hip
// Optimizer::OptimizeSim3 over nProblems (by value)
struct Sim3OptParams {
  int nProblems, stride;
  const int32_t* kf1Slot;  // null: p
  const int32_t* kf2Slot;
  const orb_keypoint_t* keys;
  const int32_t* nkeys;
  const int32_t* pointIndex;
  const orb_pose_t* pose;
  const orb_map_point_t* points;
  int32_t* match12;        // in/out
  const int32_t* index2;
  const orb_sim3_result_t* start;
  const uint8_t* active;   // null: every problem
  int nLevels;
  float invLevelSigma2[ORB_MAX_LEVELS];
  float k1[4], k2[4];      // fx, fy, cx, cy
  float th2;
  int fixScale;
  orb_sim3_opt_result_t* out;
};

// ----------------------------------------------------- newpoints_kernels.hip
// KeyFrame::ComputeSceneMedianDepth over nProblems keyframe slots (by value)
struct MedianDepthParams {
  int nProblems, stride, q;
  const int32_t* slot;          // null: p
  const int32_t* nkeys;
  const int32_t* pointIndex;
  const orb_pose_t* pose;
  const orb_map_point_t* points;
  float* median;
  int32_t* count;
};

// LocalMapping::CreateNewMapPoints' gate and loop body over nProblems
// (current keyframe, neighbour) pairs (by value)
struct NewPointsParams {
  int nProblems, stride;
  const int32_t* kf1Slot;
  const int32_t* kf2Slot;
  const orb_keypoint_t* keys;
  const int32_t* nkeys;
  int32_t* pointIndex;          // in/out: the two AddMapPoint calls
  const orb_pose_t* pose;
  const float* uRight;          // null (with depth): monocular keyframes, all -1
  const float* depth;
  const int32_t* match12;
  const float* medianDepth;     // read only when monocular
  orb_map_point_t* points;
  int pointCapacity;
  int32_t* pointCursor;
  const int32_t* cursorIndex;
  float k1[4], inv1[2], bf1, mb1;  // fx fy cx cy, invfx invfy (1.0f / f on the host), mbf, mb
  float k2[4], inv2[2], mb2;
  int nLevels;
  float scaleFactors[ORB_MAX_LEVELS], sigma2[ORB_MAX_LEVELS];
  float ratioFactor;            // 1.5f * mfScaleFactor
  int monocular;
  uint8_t* status;
  float* x3d;
  int32_t* newPairs;
  orb_new_point_info_t* info;
};

// ---------------------------------------------------- sim3chain_kernels.hip
// SearchByBoW(pKF1, pKF2, vpMatches12) over nProblems pairs of keyframe slots
// (by value): one set of slot arrays serves both sides
struct BowKfBatchParams {
  int nProblems, stride;
  const int32_t* kf1Slot;  // null: p
  const int32_t* kf2Slot;
  BowSlots kf;
  const int32_t* pointIndex;      // mvpMapPoints per keypoint (< 0: NULL)
  const orb_map_point_t* points;  // null: no point is bad
  float nnratio;
  int checkOri, minMatches;
};

// SearchBySim3 over nProblems pairs of keyframe slots (by value).  base: the
// camera, the image bounds with invW / invH, th, logScale, the levels and
// thr = 100; the kernel adds each direction's R, t, R2, t2.
struct Sim3SearchParams {
  int nProblems, stride;
  const int32_t* kf1Slot;  // null: p
  const int32_t* kf2Slot;
  const orb_keypoint_t* keys;
  const uint8_t* desc;
  const int32_t* nkeys;
  const int32_t* pointIndex;
  const orb_pose_t* pose;
  const orb_map_point_t* points;
  const uint8_t* mpDesc;
  int32_t* match12;           // in/out
  int32_t* index2;            // in/out
  const uint8_t* inliers12;   // null: no filter
  const orb_sim3_result_t* sim3;
  const uint8_t* active;      // null: every problem
  PPParams base;
  int32_t* new12;             // null: not wanted
  orb_sim3_search_info_t* info;
};
