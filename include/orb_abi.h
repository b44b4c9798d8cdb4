/*
 * orb_abi.h -- C ABI of the MI355X-native ORB front-end (extractor + Hamming matcher).
 *
 * This is the drop-in boundary.  Plain C: pointers, sizes, status codes; no
 * OpenCV, no torch, no HIP types in any signature (streams are passed as
 * `void*`, a hipStream_t, NULL = the handle's own stream).
 *
 * Streams and call order.  A handle's calls are serialised on the host (a
 * mutex per handle) and on the device: every call reuses the handle's device
 * scratch, so a call issued on a different stream from the previous call on
 * the same handle first makes its stream wait for that call (an event wait,
 * no host synchronisation), and a frame-size change, which rewrites the
 * extractor's plan tables, waits on the host for the previous call.  One
 * handle may therefore be driven from any mix of streams (the reference's
 * ORBextractor is not reentrant at all, include/ORBextractor.h:85).  The
 * caller still orders its own data: a batch call's inputs must be ready on
 * the stream passed, and its outputs are ready on that stream only.  Calls
 * issued on a stream being captured into a graph record no event; the caller
 * orders the graph's launches.  The extractor's batch calls also use one
 * device-wide side stream that HIP creates blocking, so work on the legacy
 * null stream waits for its FAST kernels in flight (INTEGRATION.md "Streams").
 *
 * Reference interfaces each entry point replaces (paths relative to the
 * reference tree, yg838457845/ORB_SLAM2-Chinese-annotation):
 *
 *   orb_extractor_create/destroy   ORBextractor::ORBextractor  include/ORBextractor.h:51-54,
 *                                  src/ORBextractor.cc:428-489
 *   orb_extractor_get_*            ORBextractor::Get*          include/ORBextractor.h:63-83
 *   orb_extractor_extract          ORBextractor::operator()    include/ORBextractor.h:59-61,
 *                                  src/ORBextractor.cc:1091-1169
 *   orb_extractor_pyramid_level    ORBextractor::mvImagePyramid include/ORBextractor.h:85
 *   orb_extractor_extract_batch    (throughput form of operator(), many frames per launch)
 *   orb_descriptor_distance        ORBmatcher::DescriptorDistance src/ORBmatcher.cc:1814-1830
 *   orb_hamming_batch              batched DescriptorDistance (device)
 *   orb_match_projection_local     ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, float)
 *                                  src/ORBmatcher.cc:47-133 (+ Frame::GetFeaturesInArea
 *                                  src/Frame.cc:368-424, AssignFeaturesToGrid :261-276)
 *   orb_match_projection_local_batch  device-batched form of the above
 *   orb_stereo_match               Frame::ComputeStereoMatches src/Frame.cc:516-704
 *   orb_match_projection_frame     ORBmatcher::SearchByProjection(Frame&, const Frame&, float, bool)
 *                                  src/ORBmatcher.cc:1460-1619
 *   orb_match_bow                  ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)
 *                                  src/ORBmatcher.cc:164-306
 *   orb_frustum(_batch)            Frame::isInFrustum src/Frame.cc:303-366 over the local map
 *                                  (Tracking::SearchLocalPoints src/Tracking.cc:1360-1377,
 *                                  MapPoint::PredictScale src/MapPoint.cc:435-450)
 *   orb_stereo_match_batch         device-batched ComputeStereoMatches (pairs from two extractors)
 *   orb_search_for_initialization(_batch)  ORBmatcher::SearchForInitialization
 *                                  src/ORBmatcher.cc:429-577
 *   orb_distinctive_descriptors(_batch)    MapPoint::ComputeDistinctiveDescriptors
 *                                  src/MapPoint.cc:250-326
 *   orb_search_by_projection_reloc SearchByProjection(Frame&, KeyFrame*, set, th, ORBdist)
 *                                  src/ORBmatcher.cc:1622-1759
 *   orb_search_by_projection_sim3  SearchByProjection(KeyFrame*, Scw, ...) src/ORBmatcher.cc:311-425
 *   orb_fuse / orb_fuse_sim3       Fuse(KeyFrame*, ...) x2   src/ORBmatcher.cc:903-1210
 *   orb_search_by_sim3             SearchBySim3              src/ORBmatcher.cc:1212-1458
 *   orb_match_bow_kf               SearchByBoW(KeyFrame*, KeyFrame*, ...) src/ORBmatcher.cc:581-716
 *   orb_search_for_triangulation   SearchForTriangulation    src/ORBmatcher.cc:718-901
 *   orb_undistort_points / orb_undistort_keypoints(_batch) / orb_compute_image_bounds
 *                                  cv::undistortPoints in Frame::UndistortKeyPoints
 *                                  src/Frame.cc:452-482 and ComputeImageBounds :484-514
 *   orb_match_projection_local_batch_stereo  the batched SearchByProjection(F, localMap)
 *                                  with mvuRight (src/ORBmatcher.cc:95-100)
 *   orb_stereo_from_rgbd(_batch)   Frame::ComputeStereoFromRGBD src/Frame.cc:707-728 with
 *                                  Tracking::GrabImageRGBD's convertTo src/Tracking.cc:229-230
 *   orb_unproject_stereo(_batch)   Frame::UnprojectStereo src/Frame.cc:730-744
 *   orb_close_points(_batch)       the closest-point selection of Tracking::UpdateLastFrame
 *                                  src/Tracking.cc:969-1021 and CreateNewKeyFrame :1263-1318,
 *                                  the counts of NeedNewKeyFrame :1181-1197
 *   orb_match_projection_frame_batch  device-batched SearchByProjection(CurrentFrame, LastFrame)
 *                                  src/ORBmatcher.cc:1460-1619 with TrackWithMotionModel's
 *                                  2 * th retry src/Tracking.cc:1044-1052; pins: twc as mOw,
 *                                  3x3 * vector as ((r0 x + r1 y) + r2 z) + t, invzc = 1.0f / z
 *   orb_track_discard_outliers_batch  "Discard outliers" src/Tracking.cc:1060-1083 and the
 *                                  already-matched marking of SearchLocalPoints :1333-1354
 *   orb_match_bow_batch            device-batched SearchByBoW(KeyFrame*, Frame&, ...)
 *                                  src/ORBmatcher.cc:164-306 as TrackReferenceKeyFrame
 *                                  src/Tracking.cc:904-954 and Relocalization :1592-1616 call it
 *   orb_track_discard_outliers_batch_n  the discard loop with the match count read through a
 *                                  strided pointer (src/Tracking.cc:928-951 after SearchByBoW)
 *   orb_update_local_map_batch     Tracking::UpdateLocalMap src/Tracking.cc:1395-1404:
 *                                  UpdateLocalKeyFrames :1437-1558 and UpdateLocalPoints
 *                                  :1407-1434 over a device-resident map view, with the
 *                                  already-matched marking of SearchLocalPoints :1333-1354
 *   orb_track_local_merge_batch    F.mvpMapPoints[bestIdx] = pMP (src/ORBmatcher.cc:127) of the
 *                                  local matcher, as global point indices
 *   orb_track_local_map_finish_batch  mnMatchesInliers and the stereo outlier reset of
 *                                  Tracking::TrackLocalMap src/Tracking.cc:1109-1135
 *   orb_sim3_solver_setup_batch    Sim3Solver's constructor and SetRansacParameters
 *                                  src/Sim3Solver.cc:37-141 (LoopClosing::ComputeSim3
 *                                  src/LoopClosing.cc)
 *   orb_sim3_solver_iterate_batch  Sim3Solver::iterate / find :144-220 with ComputeSim3
 *                                  :237-351, CheckInliers :354-378 and Project :396-417
 *   orb_scene_median_depth(_batch) KeyFrame::ComputeSceneMedianDepth src/KeyFrame.cc:658-694
 *   orb_create_new_map_points(_batch)  LocalMapping::CreateNewMapPoints: the neighbour
 *                                  loop's gate src/LocalMapping.cc:289-311 and body :338-535
 *                                  (parallax test, linear triangulation, both reprojection
 *                                  checks, scale consistency) with the new point's
 *                                  MapPoint::UpdateNormalAndDepth src/MapPoint.cc:349-402
 *   orb_search_for_triangulation_batch  device-batched SearchForTriangulation
 *                                  src/ORBmatcher.cc:718-901 as the neighbour loop of
 *                                  CreateNewMapPoints calls it src/LocalMapping.cc:313-318,
 *                                  on the slot arrays of orb_create_new_map_points_batch
 *   orb_match_bow_kf_batch         device-batched SearchByBoW(pKF1, pKF2, vpMatches12)
 *                                  src/ORBmatcher.cc:581-716 with ComputeSim3's 20-match
 *                                  gate src/LoopClosing.cc:282-293, on the solver's slots
 *   orb_search_by_sim3_batch       device-batched SearchBySim3 src/ORBmatcher.cc:1212-1458
 *                                  with the inlier filter of src/LoopClosing.cc:338-343, on
 *                                  the solver's slots, rows, result and inlier flags
 *   orb_vocabulary_create / _load_text / _destroy
 *                                  DBoW2 TemplatedVocabulary ctor + loadFromTextFile
 *                                  Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1362-1448
 *                                  (ORBVocabulary, include/ORBVocabulary.h; loaded by
 *                                  System::System src/System.cc)
 *   orb_vocabulary_transform(_batch)  Frame::ComputeBoW src/Frame.cc:439-449,
 *                                  KeyFrame::ComputeBoW src/KeyFrame.cc:60-71 ->
 *                                  TemplatedVocabulary::transform(features, BowVector&,
 *                                  FeatureVector&, levelsup) TemplatedVocabulary.h:1128-1283
 *   orb_vocabulary_score(_batch)   TemplatedVocabulary::score TemplatedVocabulary.h ->
 *                                  L1/L2/ChiSquare/Bhattacharyya/DotProduct Scoring::score
 *                                  Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-311
 *   orb_kf_database_create / _add / _erase / _clear
 *                                  KeyFrameDatabase ctor, add, erase, clear
 *                                  src/KeyFrameDatabase.cc:34-76
 *   orb_kf_database_detect_relocalization
 *                                  KeyFrameDatabase::DetectRelocalizationCandidates
 *                                  src/KeyFrameDatabase.cc:205-339 (src/Tracking.cc:1569)
 *   orb_kf_database_detect_loop    KeyFrameDatabase::DetectLoopCandidates
 *                                  src/KeyFrameDatabase.cc:79-202 (src/LoopClosing.cc:125-158)
 *   orb_kf_database_set_covisibility  KeyFrame::GetBestCovisibilityKeyFrames(10) as read at
 *                                  src/KeyFrameDatabase.cc:155,286
 *
 * Error behaviour: the reference has no status codes (an empty image returns
 * silently with outputs untouched, src/ORBextractor.cc:1095-1096; a non-8UC1
 * image asserts, :1100).  Here every call returns an orb_status_t; the C++
 * wrapper (orb_slam2-chinese-annotation_amd/host/orb_amd.hpp) maps
 * ORB_EEMPTY to "return, outputs untouched" and ORB_EINVAL to an assert.
 */
#ifndef ORB_ABI_H
#define ORB_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORB_ABI_VERSION 1
#define ORB_DESC_BYTES 32
#define ORB_GRID_COLS 64 /* FRAME_GRID_COLS, include/Frame.h:39 */
#define ORB_GRID_ROWS 48 /* FRAME_GRID_ROWS, include/Frame.h:40 */

typedef enum orb_status {
  ORB_OK = 0,
  ORB_EEMPTY = 1,     /* empty input: reference returns silently, outputs untouched */
  ORB_EINVAL = -1,    /* bad argument (reference: assert) */
  ORB_ENOMEM = -2,    /* device allocation failed */
  ORB_EDEVICE = -3,   /* HIP runtime / kernel error */
  ORB_ECAPACITY = -4, /* caller buffer too small; *n set to the required size */
  ORB_ENODEV = -5     /* no gfx950 device visible */
} orb_status_t;

/* Mirrors cv::KeyPoint field-for-field (28 bytes). */
typedef struct orb_keypoint {
  float x, y;      /* pt */
  float size;      /* int(31 * scale[octave]) */
  float angle;     /* degrees, [0, 360] */
  float response;  /* FAST-9/16 corner score */
  int32_t octave;  /* pyramid level */
  int32_t class_id;/* always -1 */
} orb_keypoint_t;

typedef struct orb_extractor orb_extractor_t;
typedef struct orb_matcher orb_matcher_t;

/* ---------------------------------------------------------------- extractor */

/* Limits (the reference states none; these are where this build stops, each
 * a status, never a silent change of results):
 *   create: nfeatures >= 0, 1 <= nlevels <= 16, scale_factor > 1 (finite)
 *     (ORB_EINVAL otherwise: at 1 the reference's quota series is 0 / 0,
 *     src/ORBextractor.cc:453-455).  Every scale factor takes the same
 *     integer resize taps; levels whose downscale the staged tiles cannot
 *     hold (beyond ~1.9) take an untiled kernel.
 *   extract: every pyramid level between 33 and 4095 px in each dimension
 *     (at 32 px or less the reference's DistributeOctTree divides by zero or
 *     sizes its root vector negatively, :562-569; keys pack x and y in 12
 *     bits), a level's quota + 4 at most 65,534 (16-bit node labels: nfeatures
 *     up to ~300,000 at 1.2 / 8 levels), FAST cells at most 64 x 64 interior
 *     pixels: ORB_EINVAL from the call (and orb_extractor_capacity < 0).
 *   DistributeOctTree (src/ORBextractor.cc:558-782): node tables hold
 *     quota + 4 nodes per level (the reference's list never exceeds quota + 3,
 *     or 4 x its root count after the first pass), at most 512 passes (distinct
 *     keys separate in about 12; the final phase adds a few) and 2^24 created
 *     nodes.  Exceeding any of them is not reachable with keys the FAST stage
 *     emits; if it happened the image fails as a whole: orb_extractor_extract
 *     returns ORB_EDEVICE and the batch form writes d_counts[i] = ORB_EDEVICE
 *     (negative).  A test-only build of the library with the pass bound
 *     lowered drives that path (tests/test_gpu_extractor.py); the product
 *     reads no environment variable that changes results. */
orb_status_t orb_extractor_create(int nfeatures, float scale_factor, int nlevels,
                                  int ini_th_fast, int min_th_fast, int device,
                                  orb_extractor_t** out);
void orb_extractor_destroy(orb_extractor_t* h);

int orb_extractor_get_levels(const orb_extractor_t* h);
float orb_extractor_get_scale_factor(const orb_extractor_t* h);
/* Each writes nlevels floats. */
void orb_extractor_get_scale_factors(const orb_extractor_t* h, float* out);
void orb_extractor_get_inverse_scale_factors(const orb_extractor_t* h, float* out);
void orb_extractor_get_scale_sigma_squares(const orb_extractor_t* h, float* out);
void orb_extractor_get_inverse_scale_sigma_squares(const orb_extractor_t* h, float* out);
/* Per-level keypoint quotas (mnFeaturesPerLevel, src/ORBextractor.cc:453-464). */
void orb_extractor_get_features_per_level(const orb_extractor_t* h, int32_t* out);
/* Upper bound on keypoints one image of this size can produce. */
int orb_extractor_capacity(const orb_extractor_t* h, int width, int height);

/* ORBextractor::operator(): host image in, host keypoints + N x 32 descriptors out.
 * Synchronous.  `capacity` = rows available in keypoints/descriptors; on
 * ORB_ECAPACITY *n_keypoints holds the required count. */
orb_status_t orb_extractor_extract(orb_extractor_t* h, const uint8_t* image, int width,
                                   int height, size_t stride, orb_keypoint_t* keypoints,
                                   uint8_t* descriptors, int capacity, int* n_keypoints);

/* Host copy of mvImagePyramid[level] of the first image of the last call
 * (orb_extractor_extract, or image 0 of orb_extractor_extract_batch, whose
 * level 0 is read from the caller's d_images: keep it alive until then).
 * The copy waits for the last call's stream.  dst may be NULL to query the size. */
orb_status_t orb_extractor_pyramid_level(orb_extractor_t* h, int level, uint8_t* dst,
                                         size_t dst_stride, int* width, int* height);
/* mvImagePyramid[level] of the last orb_extractor_extract call without a copy
 * out: a pointer into pinned host memory the library owns, valid until the
 * next call on this handle (the reference rebuilds mvImagePyramid on every
 * call too, src/ORBextractor.cc:1172-1207; its only reader is
 * Frame::ComputeStereoMatches, src/Frame.cc:524,619,633,639, right after the
 * extraction).  Level 0 is the call's pinned staging of the image; levels 1..
 * come from one DMA of the device pyramid, which the first request makes
 * synchronously and which from then on rides in every call's graph after the
 * keypoint copy.  ORB_EINVAL after a batch call. */
orb_status_t orb_extractor_host_pyramid(orb_extractor_t* h, int level, const uint8_t** data,
                                        int* width, int* height, size_t* stride);
/* Stops the per-call DMA of levels 1.. that orb_extractor_host_pyramid turned
 * on (for a caller that no longer reads the mirror): later calls move no
 * pyramid bytes until the next request, which again copies once and turns the
 * per-call copy back on. */
orb_status_t orb_extractor_host_pyramid_off(orb_extractor_t* h);
/* The 7x7 Gaussian-blurred copy of level `level` of the first image of the
 * last call (the image computeDescriptors samples, src/ORBextractor.cc:1143-1145);
 * same conventions as orb_extractor_pyramid_level. */
orb_status_t orb_extractor_blurred_level(orb_extractor_t* h, int level, uint8_t* dst,
                                         size_t dst_stride, int* width, int* height);

/* Throughput form: n_images device-resident images (image i at
 * d_images + i*image_pitch, rows `stride` apart), all width x height.
 * Outputs per image i: d_keypoints[i*capacity ...], d_descriptors[(i*capacity) * 32 ...],
 * d_counts[i].  Asynchronous on `stream` (NULL = handle stream). */
orb_status_t orb_extractor_extract_batch(orb_extractor_t* h, const uint8_t* d_images,
                                         int n_images, int width, int height, size_t stride,
                                         size_t image_pitch, orb_keypoint_t* d_keypoints,
                                         uint8_t* d_descriptors, int capacity,
                                         int32_t* d_counts, void* stream);

/* Device pointer to pyramid level `level` of batch image `image` after
 * orb_extractor_extract_batch (valid until the next call on this handle).
 * Level 0 is the caller's own image memory (d_images of that call): it is
 * valid only while the caller keeps it.  Readers on another stream must order
 * themselves after the batch's stream. */
orb_status_t orb_extractor_batch_level(orb_extractor_t* h, int image, int level,
                                       const uint8_t** d_level, int* width, int* height,
                                       size_t* stride);

/* Stream the handle launches on (a hipStream_t). */
void* orb_extractor_stream(orb_extractor_t* h);

/* Kernel timing with HIP events recorded on the stream each stage is launched
 * on (no synchronisation in the launch path).  profile(h, 1) resets and
 * enables; profile_read drains the recorded events and returns the summed
 * milliseconds, launch count and kernel name of `stage`:
 * 0 k_pyr_resize (nlevels-1 launches per call), 1 k_blur_levels (split mode
 * only), 2 FAST (k_fast_cells on the levels the main stream runs, or
 * k_fast_band on all levels), 3 k_octree, 4 k_orient_desc,
 * 5 k_fast_cells_side (the cells of level 0, then of levels 1-2, on the
 * handle's side stream beside the resize chain; durations summed; 0 launches
 * when not split off), 6 = the whole extraction call.
 * enable = 2 times every stage alone: while it is set the batch form runs all
 * stages one after another on the caller's stream (no side stream), so each
 * stage's events bracket its own kernels only (bench.py's isolated table). */
orb_status_t orb_extractor_profile(orb_extractor_t* h, int enable);
orb_status_t orb_extractor_profile_read(orb_extractor_t* h, int stage, double* total_ms,
                                        int* launches, const char** name);

/* ------------------------------------------------------------------ matcher */

/* A frame as the matcher sees it (Frame members used by ORBmatcher). */
typedef struct orb_frame {
  int32_t n;                     /* N */
  const orb_keypoint_t* keys;    /* mvKeysUn (== mvKeys at zero distortion) */
  const uint8_t* descriptors;    /* mDescriptors, N x 32 */
  const float* u_right;          /* mvuRight (N) or NULL for monocular (-1) */
  float min_x, max_x, min_y, max_y; /* mnMinX, mnMaxX, mnMinY, mnMaxY */
  int32_t n_levels;
  const float* scale_factors;    /* mvScaleFactors */
} orb_frame_t;

/* MapPoint fields written by Frame::isInFrustum (include/MapPoint.h:92-97). */
typedef struct orb_mp_track {
  float proj_x, proj_y, proj_xr;  /* mTrackProjX, mTrackProjY, mTrackProjXR */
  float view_cos;                 /* mTrackViewCos */
  int32_t level;                  /* mnTrackScaleLevel */
  uint8_t in_view;                /* mbTrackInView */
  uint8_t bad;                    /* isBad() */
  uint8_t has_obs;                /* Observations() > 0 (a claim by it locks the keypoint) */
  uint8_t _pad;
} orb_mp_track_t;

/* MapPoint state read by Frame::isInFrustum and Tracking::SearchLocalPoints
 * (src/Frame.cc:303-366, src/Tracking.cc:1360-1377, src/MapPoint.cc:404-450). */
typedef struct orb_map_point {
  float pos[3];        /* GetWorldPos() */
  float normal[3];     /* GetNormal() */
  float min_distance;  /* mfMinDistance (GetMinDistanceInvariance = 0.8f * it) */
  float max_distance;  /* mfMaxDistance (GetMaxDistanceInvariance = 1.2f * it) */
  uint8_t bad;         /* isBad() */
  uint8_t seen;        /* mnLastFrameSeen == mCurrentFrame.mnId (already matched) */
  uint8_t has_obs;     /* Observations() > 0 */
  uint8_t _pad;
} orb_map_point_t;     /* 36 bytes */

/* Pinhole camera (Frame::fx, fy, cx, cy, mbf, mb). */
typedef struct orb_camera {
  float fx, fy, cx, cy, bf, mb;
} orb_camera_t;

/* Frame pose (Frame::UpdatePoseMatrices, src/Frame.cc:294-300). */
typedef struct orb_pose {
  float rcw[9];        /* mRcw, row-major */
  float tcw[3];        /* mtcw */
  float ow[3];         /* mOw = -mRcw^T * mtcw (camera centre) */
} orb_pose_t;

int orb_descriptor_distance(const uint8_t* a, const uint8_t* b);

orb_status_t orb_matcher_create(int device, orb_matcher_t** out);
void orb_matcher_destroy(orb_matcher_t* m);
void* orb_matcher_stream(orb_matcher_t* m);
/* Same scheme for the batched local-map matcher: stage 0 k_grid_build,
 * 1 k_proj_candidates, 2 k_proj_resolve, 3 = whole call. */
orb_status_t orb_matcher_profile(orb_matcher_t* m, int enable);
orb_status_t orb_matcher_profile_read(orb_matcher_t* m, int stage, double* total_ms,
                                      int* launches, const char** name);

/* Resolve schedule of SearchByProjection(F, vpMapPoints)'s first-come claims
 * (src/ORBmatcher.cc:90-93,127: a keypoint claimed by an earlier MapPoint of
 * the same call is skipped).  Every schedule returns the reference's result;
 * they differ in how the ordered resolve is spread over the chip (DESIGN.md
 * §4.2).  AUTO (the default) picks by problem count and map size; JACOBI runs
 * `jacobi_rounds` (1-48) chip-wide rounds first, then the fixed-point windows
 * for any problem not yet settled.  Schedules that need more LDS than the
 * frame's keypoint count allows fall back to the prefix windows. */
#define ORB_RESOLVE_AUTO 0
#define ORB_RESOLVE_PREFIX 1      /* speculative windows, longest conflict-free prefix kept */
#define ORB_RESOLVE_FIXED_POINT 2 /* 1024-point windows iterated to their fixed point */
#define ORB_RESOLVE_JACOBI 3      /* chip-wide rounds + fixed-point windows */
orb_status_t orb_matcher_set_resolve(orb_matcher_t* m, int schedule, int jacobi_rounds);
/* The resolve kernel the local-map matcher launches for a call of n_problems
 * problems at these strides under the handle's schedule. */
#define ORB_RESOLVE_KERNEL_PREFIX_W1 1   /* k_proj_resolve<1>: one wave per problem */
#define ORB_RESOLVE_KERNEL_PREFIX_W4 4   /* k_proj_resolve<4> */
#define ORB_RESOLVE_KERNEL_PREFIX_W8 8   /* k_proj_resolve<8> */
#define ORB_RESOLVE_KERNEL_FIXED_POINT 16 /* k_proj_resolve_fp<1024> */
#define ORB_RESOLVE_KERNEL_JACOBI 32     /* k_proj_jacobi rounds + k_proj_resolve_fp */
orb_status_t orb_matcher_resolve_kernel(orb_matcher_t* m, int n_problems, int kp_stride,
                                        int mp_stride, int* kernel);

/* dist[i] = DescriptorDistance(a + 32 i, b + 32 i), device pointers. */
orb_status_t orb_hamming_batch(orb_matcher_t* m, const uint8_t* d_a, const uint8_t* d_b,
                               int n, int32_t* d_dist, void* stream);

/* SearchByProjection(F, vpMapPoints, th) with ORBmatcher(nnratio).
 * kp_locked[i] != 0  <=>  F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() > 0
 * on entry.  Output kp_match[i] = index of the MapPoint assigned to keypoint i
 * by THIS call (last writer wins, as F.mvpMapPoints[bestIdx]=pMP), or -1.
 * Returns the reference's nmatches. Host buffers. */
orb_status_t orb_match_projection_local(orb_matcher_t* m, const orb_frame_t* frame,
                                        const uint8_t* kp_locked, int n_mp,
                                        const orb_mp_track_t* mps, const uint8_t* mp_desc,
                                        float th, float nnratio, int32_t* kp_match,
                                        int32_t* nmatches);

/* Zero-copy form of orb_match_projection_local, for a caller that flattens its
 * Frame and MapPoints anyway (the reference-typed drop-in's SearchByProjection,
 * integration/ORBmatcher.cc): _stage returns pointers into the handle's pinned
 * input block laid out for n_keys keypoints and n_mp map points, the caller
 * writes keys, descriptors, the map-point tracks and descriptors there (and
 * u_right / kp_locked when it passes stereo / locked), and _staged runs the
 * match on them: one DMA in, no library-side copy.  `frame` supplies n (==
 * n_keys), the bounds, levels and scale factors; its keys / descriptors /
 * u_right pointers are not read.  The pointers are valid until the next call
 * on this handle; the pair must not interleave with other calls on it (one
 * handle per thread, as the reference's per-call-site ORBmatcher objects).
 * Optional _begin, between _stage and _staged, once the frame's part (keys,
 * descriptors, u_right, kp_locked) is written and before the map points are:
 * it sends that part and builds the keypoint grid on the device while the
 * caller flattens its map; stereo / locked must equal _staged's.  A _stage
 * after a _begin without its _staged waits for the _begin's work first. */
typedef struct orb_local_stage {
  orb_keypoint_t* keys;        /* n_keys */
  uint8_t* descriptors;        /* n_keys x 32 */
  float* u_right;              /* n_keys (read only with stereo != 0) */
  uint8_t* kp_locked;          /* n_keys (read only with locked != 0) */
  orb_mp_track_t* mps;         /* n_mp */
  uint8_t* mp_desc;            /* n_mp x 32 */
} orb_local_stage_t;
orb_status_t orb_match_projection_local_stage(orb_matcher_t* m, int n_keys, int n_mp,
                                              orb_local_stage_t* out);
orb_status_t orb_match_projection_local_begin(orb_matcher_t* m, const orb_frame_t* frame,
                                              int stereo, int locked);
orb_status_t orb_match_projection_local_staged(orb_matcher_t* m, const orb_frame_t* frame,
                                               int n_mp, int stereo, int locked, float th,
                                               float nnratio, int32_t* kp_match,
                                               int32_t* nmatches);

/* Device-batched form: P independent (frame, local map) problems.
 * Problem p: keypoints d_keys + p*kp_stride (count d_nkeys[p]), descriptors
 * d_desc + p*kp_stride*32, locks d_locked + p*kp_stride (may be NULL),
 * map points d_mps + p*mp_stride (count d_nmps[p]), their descriptors
 * d_mp_desc + p*mp_stride*32.  Monocular (u_right = -1).  Frame bounds and
 * scale factors are shared.  Outputs d_kp_match + p*kp_stride, d_nmatches[p]. */
orb_status_t orb_match_projection_local_batch(
    orb_matcher_t* m, int n_problems, const orb_keypoint_t* d_keys, const uint8_t* d_desc,
    const int32_t* d_nkeys, const uint8_t* d_locked, int kp_stride,
    const orb_mp_track_t* d_mps, const uint8_t* d_mp_desc, const int32_t* d_nmps,
    int mp_stride, float min_x, float max_x, float min_y, float max_y, int n_levels,
    const float* scale_factors, float th, float nnratio, int32_t* d_kp_match,
    int32_t* d_nmatches, void* stream);

/* The same for stereo / RGB-D frames: d_u_right + p*kp_stride is problem p's
 * mvuRight (-1 = no right coordinate; e.g. orb_stereo_from_rgbd_batch's or
 * orb_stereo_match_batch's output), read by the staged grid build, the
 * candidate scan and every resolve, which apply the reference's check
 * (src/ORBmatcher.cc:95-100: a keypoint with mvuRight > 0 is skipped when
 * |mTrackProjXR - mvuRight| > r * scale[octave]).  Every other argument as
 * above; every resolve schedule and routed kernel is supported. */
orb_status_t orb_match_projection_local_batch_stereo(
    orb_matcher_t* m, int n_problems, const orb_keypoint_t* d_keys, const uint8_t* d_desc,
    const float* d_u_right, const int32_t* d_nkeys, const uint8_t* d_locked, int kp_stride,
    const orb_mp_track_t* d_mps, const uint8_t* d_mp_desc, const int32_t* d_nmps,
    int mp_stride, float min_x, float max_x, float min_y, float max_y, int n_levels,
    const float* scale_factors, float th, float nnratio, int32_t* d_kp_match,
    int32_t* d_nmatches, void* stream);

/* Tracking::SearchLocalPoints' frustum pass: for each local MapPoint in order,
 * skip it if seen or bad, else Frame::isInFrustum(pMP, viewing_cos_limit)
 * (src/Tracking.cc:1360-1377, src/Frame.cc:303-366, MapPoint::PredictScale
 * src/MapPoint.cc:435-450).  Writes tracks[i] (proj_x, proj_y, proj_xr,
 * view_cos, level, in_view; bad and has_obs copied through; all-zero
 * projection fields when not in view) and n_in_view = nToMatch.  The tracks
 * feed orb_match_projection_local unchanged.  log_scale_factor =
 * Frame::mfLogScaleFactor.  Host buffers. */
orb_status_t orb_frustum(orb_matcher_t* m, int n_mp, const orb_map_point_t* mps,
                         const orb_pose_t* pose, const orb_camera_t* cam, float min_x,
                         float max_x, float min_y, float max_y, float viewing_cos_limit,
                         float log_scale_factor, int n_levels, orb_mp_track_t* tracks,
                         int32_t* n_in_view);

/* Device-batched form: problem p uses d_poses[p], map points d_mps + p*mp_stride
 * (count d_nmps[p]); writes d_tracks + p*mp_stride and d_n_in_view[p]. */
orb_status_t orb_frustum_batch(orb_matcher_t* m, int n_problems, const orb_map_point_t* d_mps,
                               const int32_t* d_nmps, int mp_stride, const orb_pose_t* d_poses,
                               const orb_camera_t* cam, float min_x, float max_x, float min_y,
                               float max_y, float viewing_cos_limit, float log_scale_factor,
                               int n_levels, orb_mp_track_t* d_tracks, int32_t* d_n_in_view,
                               void* stream);

/* Frame::ComputeStereoMatches for one rectified pair.  Left/right keypoints
 * and descriptors as produced by the two extractors, plus both pyramids
 * (level l of side s at pyr[s][l] with the given stride/size).  Writes
 * mvuRight / mvDepth (-1 = no match). Host buffers.
 *
 * Defined input domain (this entry, _batch and _extracted alike).  The
 * reference indexes vRowIndices and cuts its 11x11 windows without a bounds
 * check (src/Frame.cc:543,565,619,639), so it is defined only where
 *   - every octave lies in [0, n_levels);
 *   - every right keypoint's row band [floor(y - 2 s), ceil(y + 2 s)], s its
 *     octave's scale factor, lies in [0, H - 1], H = level_height[0], and every
 *     left keypoint's (int)y does;
 *   - every left keypoint's window fits its level: 5 <= roundf(x * inv) <=
 *     width - 6 and 5 <= roundf(y * inv) <= height - 6 at its octave;
 *   - every right keypoint that can be a left keypoint's best candidate has
 *     roundf(uR * inv) >= 10 at the LEFT keypoint's octave: the 11 shifts reach
 *     10 columns left of it (the right side is guarded, :633).
 * Keypoints of the extractors satisfy all four (EDGE_THRESHOLD = 19).  Inside
 * the domain the outputs equal the reference's bit for bit.  Outside it the
 * device code clamps the row bands to the image and skips a left keypoint
 * whose row is outside it, but the windows are read as given: the result is
 * unspecified and the reads may leave the level.
 * With no match at all (the reference then indexes an empty vector, :691)
 * every output is -1. */
typedef struct orb_stereo_input {
  const orb_frame_t* left;       /* mvKeys, mDescriptors (u_right ignored) */
  int32_t n_right;
  const orb_keypoint_t* right_keys;
  const uint8_t* right_desc;
  int32_t n_levels;
  const uint8_t* const* left_levels;   /* n_levels host pointers */
  const uint8_t* const* right_levels;
  const int32_t* level_width;    /* n_levels */
  const int32_t* level_height;
  const int64_t* level_stride;
  const float* inv_scale_factors;/* mvInvScaleFactors */
  float bf;                      /* mbf */
  float fx;                      /* fx; mb = bf / fx */
} orb_stereo_input_t;

orb_status_t orb_stereo_match(orb_matcher_t* m, const orb_stereo_input_t* in,
                              float* u_right, float* depth);

/* Device-batched ComputeStereoMatches for n_pairs rectified pairs whose left
 * and right images went through orb_extractor_extract_batch on left_ext and
 * right_ext (pyramids are read from those handles).  Keypoints/descriptors as
 * written by the two batches (pair i at i*kp_stride), counts d_left_n/d_right_n.
 * Writes, for i < d_left_n[pair] only (slots past the count are not touched):
 * d_u_right / d_depth (-1 = none), and d_sad = the best SAD (vDistIdx's first
 * member, src/Frame.cc:685) of every match found, INCLUDING those the median
 * test of :690-703 then resets to -1 in d_u_right / d_depth; -1 where no match
 * was found.  So d_sad[i] >= 0 with d_u_right[i] == -1 marks a pruned match.
 * The match kernel reads right-image rows in aligned 16-byte spans, of which
 * it uses the 11 bytes inside the level: a span may end up to 4 bytes past
 * its row, so past the last row of the right batch's last image (level 0 is
 * the caller's d_images) up to 4 bytes may be read and ignored. */
orb_status_t orb_stereo_match_batch(orb_matcher_t* m, int n_pairs, orb_extractor_t* left_ext,
                                    orb_extractor_t* right_ext, const orb_keypoint_t* d_left_keys,
                                    const uint8_t* d_left_desc, const int32_t* d_left_n,
                                    const orb_keypoint_t* d_right_keys,
                                    const uint8_t* d_right_desc, const int32_t* d_right_n,
                                    int kp_stride, float bf, float fx, float* d_u_right,
                                    float* d_depth, int32_t* d_sad, void* stream);

/* Frame::ComputeStereoMatches (src/Frame.cc:516-704) for the pair whose left
 * and right images were extracted last by orb_extractor_extract on left_ext and
 * right_ext (the stereo Frame constructor's two ExtractORB calls,
 * src/Frame.cc:81-93): keypoints, descriptors and both pyramids are read where
 * the extractions left them in device memory, so only mvuRight / mvDepth
 * (-1 = no match) are copied back.  *n_left = the left keypoint count; the
 * outputs need n_left entries (ORB_ECAPACITY if capacity is smaller; both
 * outputs NULL = size query).
 * ORB_EINVAL if either handle's last call was not orb_extractor_extract, or
 * if the matcher and the two extractors were not created on one device.
 * Synchronous. */
orb_status_t orb_stereo_match_extracted(orb_matcher_t* m, orb_extractor_t* left_ext,
                                        orb_extractor_t* right_ext, float bf, float fx,
                                        float* u_right, float* depth, int capacity,
                                        int* n_left);

/* SearchByProjection(CurrentFrame, LastFrame, th, bMono) with ORBmatcher(nnratio, checkOri).
 * The last frame's map points are given already projected with the current
 * pose (the float camera-space coordinates xc, yc and invzc computed exactly
 * as src/ORBmatcher.cc:1500-1505).  valid[i]=0 for NULL or outlier entries.
 * kp_match[i] (out) = MapPoint id assigned to current keypoint i by this call,
 * -1 untouched, -2 reset to NULL by the rotation-consistency filter
 * (src/ORBmatcher.cc:1597-1616).
 * Capacity: the replay runs in one workgroup, whose LDS (160 KiB of one CU)
 * holds, with N = current->n and W = ceil(N / 32), both rounded up to a
 * multiple of 4,
 *   4 * (W + 2 * N + max(n_last, 1)) + 128 bytes <= 163840,
 * else ORB_ECAPACITY, returned before anything is launched (outputs: all -1,
 * *nmatches 0).  E.g. N = 12000 admits n_last <= 16552. */
typedef struct orb_last_mp {
  float xc, yc, invzc;          /* Rcw*x3Dw + tcw, 1/z */
  int32_t last_octave;          /* LastFrame.mvKeys[i].octave */
  float last_angle;             /* LastFrame.mvKeysUn[i].angle */
  uint8_t valid;                /* pMP && !mvbOutlier[i] */
  uint8_t has_obs;              /* pMP->Observations() > 0 */
  uint8_t _pad[2];
  int32_t mp_id;                /* identity of pMP (same id => same MapPoint) */
} orb_last_mp_t;


orb_status_t orb_match_projection_frame(orb_matcher_t* m, const orb_frame_t* current,
                                        const uint8_t* kp_locked, int n_last,
                                        const orb_last_mp_t* last, const uint8_t* last_desc,
                                        const orb_camera_t* cam, float tlc_z, float th,
                                        int mono, int check_orientation,
                                        int32_t* kp_match, int32_t* nmatches);

/* SearchByBoW(pKF, F, vpMapPointMatches) with ORBmatcher(nnratio, checkOri).
 * FeatureVectors are CSR: node ids ascending (nodes_*), feature lists
 * offs_*[k]..offs_*[k+1] in feats_*.  kf_mp[i] = MapPoint id of KF keypoint i
 * or -1 (NULL); kf_mp_bad[i] = isBad().  Output f_match[j] = MapPoint id or -1. */
orb_status_t orb_match_bow(orb_matcher_t* m, int n_kf, const uint8_t* kf_desc,
                           const float* kf_angle, const int32_t* kf_mp,
                           const uint8_t* kf_mp_bad, int kf_nodes, const uint32_t* kf_node_ids,
                           const int32_t* kf_offs, const uint32_t* kf_feats, int n_f,
                           const uint8_t* f_desc, const float* f_angle, int f_nodes,
                           const uint32_t* f_node_ids, const int32_t* f_offs,
                           const uint32_t* f_feats, float nnratio, int check_orientation,
                           int32_t* f_match, int32_t* nmatches);

/* ORBmatcher(nnratio, checkOri).SearchForInitialization(F1, F2, vbPrevMatched,
 * vnMatches12, windowSize), src/ORBmatcher.cc:429-577 (called from
 * Tracking::MonocularInitialization, src/Tracking.cc:698-701).  Level-0
 * keypoints of f1 are matched to level-0 keypoints of f2 within windowSize of
 * prev_matched[i] (x, y pairs); f2's grid bounds are min_x..max_y.
 * matches12[i] = F2 index or -1; prev_matched is updated in place for matched
 * keypoints (:571-574); *nmatches = the reference's return value.  Host buffers;
 * 4 * 4 * max(N1, N2) bytes (N rounded up to a multiple of 4) and the kernel's
 * 128 static bytes must fit the 160 KiB LDS of one CU (N <= 10232), else
 * ORB_ECAPACITY. */
orb_status_t orb_search_for_initialization(orb_matcher_t* m, const orb_frame_t* f1,
                                           const orb_frame_t* f2, float* prev_matched,
                                           int window_size, float nnratio,
                                           int check_orientation, int32_t* matches12,
                                           int32_t* nmatches);

/* Device-batched form: problem p uses d_keys1/d_desc1/d_prev_matched/d_matches12
 * at offset p*kp_stride (keypoints; x2 floats, x32 bytes as applicable), counts
 * d_n1[p], d_n2[p] <= kp_stride, shared frame bounds. */
orb_status_t orb_search_for_initialization_batch(
    orb_matcher_t* m, int n_problems, const orb_keypoint_t* d_keys1, const uint8_t* d_desc1,
    const int32_t* d_n1, const orb_keypoint_t* d_keys2, const uint8_t* d_desc2,
    const int32_t* d_n2, int kp_stride, float min_x, float max_x, float min_y, float max_y,
    int window_size, float nnratio, int check_orientation, float* d_prev_matched,
    int32_t* d_matches12, int32_t* d_nmatches, void* stream);

/* MapPoint::ComputeDistinctiveDescriptors, src/MapPoint.cc:250-326, for n_mp
 * points at once.  Point p's candidate descriptors are obs_desc rows
 * obs_offs[p] .. obs_offs[p+1]-1: its observations in mObservations (map) order,
 * bad KeyFrames left out (:279-283).  best_idx[p] = BestIdx within that list,
 * -1 for an empty list (the reference returns without touching mDescriptor).
 * If descriptors != NULL, row p is overwritten with the chosen descriptor
 * (left untouched for empty lists).  Host buffers. */
orb_status_t orb_distinctive_descriptors(orb_matcher_t* m, int n_mp, const int32_t* obs_offs,
                                         const uint8_t* obs_desc, int32_t* best_idx,
                                         uint8_t* descriptors);

/* Device-batched form (device pointers, asynchronous on `stream`). */
orb_status_t orb_distinctive_descriptors_batch(orb_matcher_t* m, int n_mp,
                                               const int32_t* d_obs_offs,
                                               const uint8_t* d_obs_desc, int32_t* d_best_idx,
                                               uint8_t* d_descriptors, void* stream);

/* ---- projection-window ORBmatcher variants.  Map points use
 * orb_map_point_t; its `seen` flag marks the variant's "already found" set
 * (documented per call).  Host buffers; log_scale_factor = mfLogScaleFactor;
 * KeyFrame bounds come from the orb_frame_t (KeyFrame::IsInImage is
 * half-open, Frame bounds closed, as in the reference).
 * Capacity of the two variants that claim keypoints
 * (orb_search_by_projection_reloc, orb_search_by_projection_sim3): their
 * first-come replay runs in one workgroup, whose LDS (160 KiB of one CU)
 * holds, with N = the frame's keypoints and W = ceil(N / 32), both rounded up
 * to a multiple of 4,
 *   4 * (W + N + max(n_mp, 1)) + 128 bytes <= 163840,
 * else ORB_ECAPACITY, returned before anything is launched (kp_match all -1,
 * kp_matched as on entry, *nmatches 0).  E.g. N = 20000 admits n_mp <= 20300. */

/* SearchByProjection(Frame& F, KeyFrame* pKF, sAlreadyFound, th, ORBdist),
 * src/ORBmatcher.cc:1622-1759 (Tracking::Relocalization).  Point i = the
 * MapPoint of KF keypoint i (NULL -> bad = 1; seen = in sAlreadyFound),
 * kf_angle[i] = pKF->mvKeysUn[i].angle, pose = F.mTcw (+ mOw).
 * kp_locked[j] = F.mvpMapPoints[j] != NULL on entry.  kp_match[j] (out) = point
 * assigned to frame keypoint j by this call, -1 none, -2 reset by the rotation
 * filter.  *nmatches = the reference's return value. */
orb_status_t orb_search_by_projection_reloc(orb_matcher_t* m, const orb_frame_t* frame,
                                            const uint8_t* kp_locked, const orb_pose_t* pose,
                                            const orb_camera_t* cam, float log_scale_factor,
                                            int n_mp, const orb_map_point_t* mps,
                                            const uint8_t* mp_desc, const float* kf_angle,
                                            float th, int orb_dist, int check_orientation,
                                            int32_t* kp_match, int32_t* nmatches);

/* SearchByProjection(KeyFrame* pKF, Scw, vpPoints, vpMatched, th),
 * src/ORBmatcher.cc:311-425 (LoopClosing::ComputeSim3).  scw = the top 3 rows of
 * Scw, row-major.  seen = in spAlreadyFound (vpMatched's points).
 * kp_matched[j] (in/out) = index into vpPoints of vpMatched[j], -1 = NULL. */
orb_status_t orb_search_by_projection_sim3(orb_matcher_t* m, const orb_frame_t* kf,
                                           const float* scw, const orb_camera_t* cam,
                                           float log_scale_factor, int n_mp,
                                           const orb_map_point_t* mps, const uint8_t* mp_desc,
                                           float th, int32_t* kp_matched, int32_t* nmatches);

/* Fuse(KeyFrame* pKF, vpMapPoints, th), src/ORBmatcher.cc:903-1077: the match
 * half.  fuse_idx[i] (out) = keypoint of pKF point i fuses into (bestIdx) or
 * -1; seen = pMP->IsInKeyFrame(pKF); pose = pKF's Tcw with Ow = camera centre;
 * kf->u_right = mvuRight.  The caller applies Replace / AddObservation in
 * point order (:1048-1070), re-checking isBad() / IsInKeyFrame() first: the
 * targets only depend on entry state for points the reference still visits. */
orb_status_t orb_fuse(orb_matcher_t* m, const orb_frame_t* kf, const float* inv_level_sigma2,
                      const orb_pose_t* pose, const orb_camera_t* cam, float log_scale_factor,
                      int n_mp, const orb_map_point_t* mps, const uint8_t* mp_desc, float th,
                      int32_t* fuse_idx, int32_t* n_fuse);

/* Fuse(KeyFrame* pKF, Scw, vpPoints, th, vpReplacePoint),
 * src/ORBmatcher.cc:1079-1210: fuse_idx[i] = bestIdx or -1 (seen = in
 * pKF->GetMapPoints() at entry); vpReplacePoint / AddMapPoint stay with the
 * caller. */
orb_status_t orb_fuse_sim3(orb_matcher_t* m, const orb_frame_t* kf, const float* scw,
                           const orb_camera_t* cam, float log_scale_factor, int n_mp,
                           const orb_map_point_t* mps, const uint8_t* mp_desc, float th,
                           int32_t* fuse_idx, int32_t* n_fuse);

/* SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th),
 * src/ORBmatcher.cc:1212-1458.  mpsX[i] / mp_descX[i] = the MapPoint of
 * keypoint i of KF X (validX[i] = non-NULL), alreadyX = vbAlreadyMatchedX
 * (:1240-1252).  rXw / tXw = KF rotations (row-major) and translations.
 * match12[i1] (out) = idx2 with vpMatches12[i1] = vpMapPoints2[idx2], or -1. */
orb_status_t orb_search_by_sim3(orb_matcher_t* m, const orb_frame_t* kf1, const orb_frame_t* kf2,
                                float log_scale_factor, const orb_camera_t* cam,
                                const float* r1w, const float* t1w, const float* r2w,
                                const float* t2w, const orb_map_point_t* mps1,
                                const uint8_t* valid1, const uint8_t* already1,
                                const uint8_t* mp_desc1, const orb_map_point_t* mps2,
                                const uint8_t* valid2, const uint8_t* already2,
                                const uint8_t* mp_desc2, float s12, const float* r12,
                                const float* t12, float th, int32_t* match12, int32_t* nfound);

/* SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12),
 * src/ORBmatcher.cc:581-716 (FeatureVectors as in orb_match_bow).
 * match12[i] (out) = MapPoint id of the KF2 keypoint matched to KF1 keypoint i,
 * or -1. */
orb_status_t orb_match_bow_kf(orb_matcher_t* m, int n1, const uint8_t* desc1,
                              const float* angle1, const int32_t* mp1, const uint8_t* mp1_bad,
                              int nodes1, const uint32_t* node_ids1, const int32_t* offs1,
                              const uint32_t* feats1, int n2, const uint8_t* desc2,
                              const float* angle2, const int32_t* mp2, const uint8_t* mp2_bad,
                              int nodes2, const uint32_t* node_ids2, const int32_t* offs2,
                              const uint32_t* feats2, float nnratio, int check_orientation,
                              int32_t* match12, int32_t* nmatches);

/* SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo),
 * src/ORBmatcher.cc:718-901.  has_mpX[i] = GetMapPoint(i) != NULL;
 * level_sigma2 = pKF2->mvLevelSigma2; f12 row-major; cw = pKF1 camera centre,
 * r2w/t2w = pKF2 pose.  match12[i] (out) = KF2 index or -1; vMatchedPairs =
 * the (i, match12[i]) with match12[i] >= 0 in ascending i. */
orb_status_t orb_search_for_triangulation(
    orb_matcher_t* m, const orb_frame_t* kf1, const uint8_t* has_mp1, const orb_frame_t* kf2,
    const uint8_t* has_mp2, const float* level_sigma2, const float* f12,
    const orb_camera_t* cam, const float* cw, const float* r2w, const float* t2w, int nodes1,
    const uint32_t* node_ids1, const int32_t* offs1, const uint32_t* feats1, int nodes2,
    const uint32_t* node_ids2, const int32_t* offs2, const uint32_t* feats2, int only_stereo,
    int check_orientation, int32_t* match12, int32_t* nmatches);

/* -------------------------------------------------------- undistortion */

/* cv::undistortPoints(src, dst, mK, mDistCoef, cv::Mat(), mK), the call in
 * Frame::UndistortKeyPoints and Frame::ComputeImageBounds (src/Frame.cc:452-514),
 * with OpenCV's cvUndistortPoints arithmetic (double, 5 fixed iterations,
 * RR = mK): K = mK as 9 floats row-major, dist = mDistCoef (n_dist 4, 5, 8 or
 * 12: k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]]; the tilted 14-term model is
 * not supported).  Points as (x, y) float pairs.  Host buffers. */
orb_status_t orb_undistort_points(orb_matcher_t* m, int n, const float* xy, const float* K,
                                  const float* dist, int n_dist, float* out_xy);
/* Frame::UndistortKeyPoints: mvKeysUn from mvKeys (dist[0] == 0 -> copy,
 * :454-458); every field but pt is copied.  keys_un may equal keys. */
orb_status_t orb_undistort_keypoints(orb_matcher_t* m, int n, const orb_keypoint_t* keys,
                                     const float* K, const float* dist, int n_dist,
                                     orb_keypoint_t* keys_un);
/* Frame::ComputeImageBounds: bounds = {mnMinX, mnMaxX, mnMinY, mnMaxY}. */
orb_status_t orb_compute_image_bounds(orb_matcher_t* m, int cols, int rows, const float* K,
                                      const float* dist, int n_dist, float* bounds);
/* Device-batched UndistortKeyPoints: frame f has d_n[f] keypoints at
 * d_keys + f * stride (e.g. the output of orb_extractor_extract_batch);
 * writes d_keys_un at the same offsets.  Asynchronous on `stream`. */
orb_status_t orb_undistort_keypoints_batch(orb_matcher_t* m, int n_frames, const int32_t* d_n,
                                           const orb_keypoint_t* d_keys, int stride,
                                           const float* K, const float* dist, int n_dist,
                                           orb_keypoint_t* d_keys_un, void* stream);

/* ------------------------------------------------------------- RGB-D depth */

/* Frame::ComputeStereoFromRGBD (src/Frame.cc:707-728) on the depth image as
 * the caller holds it, with Tracking::GrabImageRGBD's conversion
 * (src/Tracking.cc:229-230) applied to the sampled element only; no converted
 * image is written.
 *   Conversion.  The host evaluates the reference's condition exactly,
 *     fabs(depth_map_factor - 1.0f) > 1e-5 || depth_type != ORB_DEPTH_F32.
 *     False: the F32 element's bits are used as they are.  True:
 *     d = (float)src * depth_map_factor, OpenCV's cvtScale_<T, float, float>
 *     with scale and shift narrowed to float (the + 0.0f shift cannot change a
 *     value that passes d > 0).  depth_map_factor is Tracking::mDepthMapFactor
 *     as Tracking holds it, i.e. already inverted (src/Tracking.cc:143-147).
 *   Sample position.  imDepth.at<float>(v, u) takes float arguments: row =
 *     (int)mvKeys[i].pt.y, column = (int)mvKeys[i].pt.x, truncated toward zero
 *     (both are fractional on levels >= 1).
 *   Outputs.  d > 0: mvDepth = d, mvuRight = mvKeysUn[i].pt.x - bf / d (one
 *     correctly rounded float divide, one subtract).  Anything else (0,
 *     negative, NaN): -1 / -1.
 *   Outside the image.  A keypoint whose truncated position lies outside
 *     cols x rows (or is NaN / beyond int range) is undefined behaviour in the
 *     reference; here it yields -1 / -1 and nothing is read.
 * depth: rows of `row_bytes` bytes (any pitch >= cols x element size that is
 * a multiple of the element size; the pointer aligned to the element size).
 * Both conversion pins are unpinned against a real OpenCV.  Host buffers. */
#define ORB_DEPTH_U16 0 /* CV_16U */
#define ORB_DEPTH_F32 1 /* CV_32F */
orb_status_t orb_stereo_from_rgbd(orb_matcher_t* m, int n, const orb_keypoint_t* keys,
                                  const orb_keypoint_t* keys_un, const void* depth,
                                  int depth_type, int cols, int rows, size_t row_bytes,
                                  float depth_map_factor, float bf, float* u_right,
                                  float* depth_out);
/* Device-batched form: frame f has d_n[f] keypoints, mvKeys at d_keys +
 * f * kp_stride and mvKeysUn at d_keys_un + f * kp_stride, and its depth image
 * at d_depth + f * image_bytes; writes d_u_right / d_depth_out at
 * f * kp_stride (slots past d_n[f] are left untouched).  Asynchronous on
 * `stream`; uses no handle scratch. */
orb_status_t orb_stereo_from_rgbd_batch(orb_matcher_t* m, int n_frames, const int32_t* d_n,
                                        const orb_keypoint_t* d_keys,
                                        const orb_keypoint_t* d_keys_un, int kp_stride,
                                        const void* d_depth, int depth_type, int cols, int rows,
                                        size_t row_bytes, size_t image_bytes,
                                        float depth_map_factor, float bf, float* d_u_right,
                                        float* d_depth_out, void* stream);

/* Frame::UnprojectStereo (src/Frame.cc:730-744; KeyFrame::UnprojectStereo,
 * src/KeyFrame.cc:640, is the same arithmetic) for every keypoint of a frame.
 * z = depth[i] <= 0 (or NaN): valid[i] = 0, x3d = 0 (the reference returns an
 * empty Mat).  Otherwise valid[i] = 1, x = (u - cx) * z * invfx,
 * y = (v - cy) * z * invfy with invfx = 1.0f / fx computed on the host
 * (src/Frame.cc:115), and mRwc * x3Dc + mOw with mRwc = rcw transposed, each
 * component float products summed left to right, then + ow:
 * X = ((rcw[0]*x + rcw[3]*y) + rcw[6]*z) + ow[0] (the product order is
 * unpinned against a real OpenCV).  x3d: 3 floats per keypoint.  Host buffers. */
orb_status_t orb_unproject_stereo(orb_matcher_t* m, int n, const orb_keypoint_t* keys_un,
                                  const float* depth, const orb_pose_t* pose,
                                  const orb_camera_t* cam, float* x3d, uint8_t* valid);
/* Device-batched form: frame f uses d_poses[f]; keypoints, depths, x3d
 * (3 floats per slot) and valid at f * kp_stride.  Asynchronous on `stream`. */
orb_status_t orb_unproject_stereo_batch(orb_matcher_t* m, int n_frames, const int32_t* d_n,
                                        const orb_keypoint_t* d_keys_un, const float* d_depth,
                                        int kp_stride, const orb_pose_t* d_poses,
                                        const orb_camera_t* cam, float* d_x3d, uint8_t* d_valid,
                                        void* stream);

/* The closest-point selection of Tracking::UpdateLastFrame (src/Tracking.cc:
 * 969-1021) and Tracking::CreateNewKeyFrame (:1263-1318) and the close-point
 * counts of Tracking::NeedNewKeyFrame (:1181-1197) for one frame.
 * In: depth = mvDepth; mp_state[i] = 0 mvpMapPoints[i] is NULL, 1 non-NULL
 * with Observations() < 1, 2 non-NULL with observations (NULL: all 0);
 * outlier = mvbOutlier (NULL: all false); th_depth = mThDepth.
 * Out: counts->n_sorted = vDepthIdx.size() (keypoints with z > 0);
 * order[0 .. n_sorted) = the keypoint index at each position of the sorted
 * vector<pair<float,int>> (ascending z, ties by ascending index; +inf sorts
 * last), -1 beyond; counts->n_visit = the positions the loop processes before
 * its break (it breaks after position j when z_j > th_depth && nPoints > 100,
 * nPoints counting every processed position); create[j] = 1 for j < n_visit
 * where mp_state is 0 or 1 (bCreateNew), 0 elsewhere; n_tracked_close /
 * n_non_tracked_close over z > 0 && z < th_depth (strict: z == th_depth is
 * neither close nor a reason to break), tracked = mp_state != 0 && !outlier.
 * The caller applies the side effects in `order` (new MapPoint,
 * AddObservation, the NULL reset at :1294).  order and create hold n entries.
 * Frames of up to orb_close_points_lds_keys() keypoint slots sort in LDS,
 * larger ones in the handle's device scratch.  Host buffers. */
typedef struct orb_close_counts {
  int32_t n_sorted, n_visit, n_tracked_close, n_non_tracked_close;
} orb_close_counts_t;
orb_status_t orb_close_points(orb_matcher_t* m, int n, const float* depth,
                              const uint8_t* mp_state, const uint8_t* outlier, float th_depth,
                              int32_t* order, uint8_t* create, orb_close_counts_t* counts);
/* Device-batched form: everything per frame at f * kp_stride (order and create
 * are written for all kp_stride slots), counts at d_counts[f].  kp_stride <
 * 2^19.  Asynchronous on `stream`. */
orb_status_t orb_close_points_batch(orb_matcher_t* m, int n_frames, const int32_t* d_n,
                                    const float* d_depth, const uint8_t* d_mp_state,
                                    const uint8_t* d_outlier, int kp_stride, float th_depth,
                                    int32_t* d_order, uint8_t* d_create,
                                    orb_close_counts_t* d_counts, void* stream);
/* Largest keypoint-slot count (n, kp_stride) whose keys sort in LDS. */
int orb_close_points_lds_keys(void);

/* Optimizer::PoseOptimization (src/Optimizer.cc:243-477): the motion-only
 * optimisation Tracking runs after each SearchByProjection and in
 * Relocalization, one SE3 vertex and one unary edge per matched keypoint,
 * with the g2o parts it reaches restated literally (four rounds that each
 * restart from pose_in, Levenberg-Marquardt exactly as
 * OptimizationAlgorithmLevenberg::solve writes it, the dense pivoted LDLT,
 * Huber for the first three rounds, classification from the edges' last
 * computed error).  k_pose_optimization, one launch.
 * In: keys_un = mvKeysUn (pt and octave are read), u_right = mvuRight (NULL:
 * monocular, every edge is a mono edge), point_index[i] >= 0 when
 * mvpMapPoints[i] is non-null, its GetWorldPos() being the three floats at
 * points + point_index[i] * point_stride_bytes (12 for packed float3, sizeof(
 * orb_map_point_t) for the matchers' map points); inv_level_sigma2 =
 * mvInvLevelSigma2 (n_levels <= 16 host floats); pose_in = mTcw.
 * Out: pose_out = the pose SetPose receives, with ow as
 * Frame::UpdatePoseMatrices computes it; outlier[i] = mvbOutlier[i] for the
 * keypoints that have an edge, the other slots are left as they are;
 * info->n_inliers = the return value (nInitialCorrespondences - nBad),
 * n_edges = nInitialCorrespondences, lm_iterations = solve() calls,
 * rejected_trials = the trials pop() undid.  Fewer than 3 edges: n_inliers = 0,
 * pose_out = pose_in (the edges' flags are cleared).  An edge whose octave is
 * outside [0, n_levels): n_edges = -1, n_inliers = 0, pose_out = pose_in,
 * outlier untouched.  pose_out may be pose_in.
 * Pinned arithmetic (double unless the reference says float; the numpy
 * restatement tests/poseopt_ref.py states the same list): sin / cos of
 * SE3Quat::exp by the double form of DESIGN.md App. A.6; pow(x, 3) = (x*x)*x;
 * IEEE sqrt and division; every Eigen operation by its documented closed form
 * with sums left to right (Quaterniond(Matrix3d), normalize, quaternion
 * products, toRotationMatrix, 3x3 products, (A^T Omega) A and
 * ((rho1 A^T) Omega) e with the zero terms of the diagonal Omega dropped,
 * LDLT on the lower triangle with symmetric pivoting on the first largest
 * |diagonal|); sums over edges in ascending keypoint order.  Unpinned against
 * Eigen / g2o binaries.  Host buffers. */
typedef struct orb_pose_opt_info {
  int32_t n_inliers, n_edges, lm_iterations, rejected_trials;
} orb_pose_opt_info_t;
orb_status_t orb_pose_optimization(orb_matcher_t* m, int n, const orb_keypoint_t* keys_un,
                                   const float* u_right, const int32_t* point_index,
                                   const void* points, int point_stride_bytes,
                                   const float* inv_level_sigma2, int n_levels,
                                   const orb_camera_t* cam, const orb_pose_t* pose_in,
                                   orb_pose_t* pose_out, uint8_t* outlier,
                                   orb_pose_opt_info_t* info);
/* Device-batched form: problem p reads d_nkeys[p] keypoints, u_right (NULL:
 * monocular), point_index and outlier at p * kp_stride, its points at
 * d_points + p * pt_stride * point_stride_bytes (pt_stride 0: the problems
 * share one array), d_pose_in[p], and writes d_pose_out[p], d_info[p].
 * orb_match_projection_local_batch[_stereo]'s d_kp_match, with the
 * orb_map_point_t array orb_frustum_batch read for it (point_stride_bytes =
 * sizeof(orb_map_point_t), pt_stride = mp_stride), feeds it unchanged.  inv_level_sigma2 and cam are host pointers.  kp_stride < 2^19;
 * above orb_pose_optimization_lds_edges() slots the edge records live in the
 * handle's device scratch.  Asynchronous on `stream`. */
orb_status_t orb_pose_optimization_batch(orb_matcher_t* m, int n_problems,
                                         const int32_t* d_nkeys,
                                         const orb_keypoint_t* d_keys_un,
                                         const float* d_u_right, int kp_stride,
                                         const int32_t* d_point_index, const void* d_points,
                                         int point_stride_bytes, long long pt_stride,
                                         const float* inv_level_sigma2, int n_levels,
                                         const orb_camera_t* cam, const orb_pose_t* d_pose_in,
                                         orb_pose_t* d_pose_out, uint8_t* d_outlier,
                                         orb_pose_opt_info_t* d_info, void* stream);
/* Largest keypoint-slot count (n, kp_stride) whose edge records stay in LDS. */
int orb_pose_optimization_lds_edges(void);

/* Device-batched SearchByProjection(CurrentFrame, LastFrame, th, bMono)
 * (src/ORBmatcher.cc:1460-1619) as Tracking::TrackWithMotionModel calls it
 * (src/Tracking.cc:1044-1052): n_problems independent problems, every input a
 * device pointer, asynchronous on `stream`, no host synchronisation.
 * Problem p reads
 *   the current frame: d_keys, d_desc (x 32), d_u_right (NULL: monocular, every
 *     mvuRight = -1) and d_locked (NULL: none; != 0 <=> mvpMapPoints[i] &&
 *     Observations() > 0 on entry) at p * kp_stride, d_nkeys[p] keypoints;
 *   d_pose_cur[p] (the predicted mVelocity * mLastFrame.mTcw) and
 *     d_pose_last[p]: rcw and tcw only, ow is not read;
 *   the last frame: d_last_keys at p * kp_stride (octave and angle),
 *     d_last_nkeys[p], d_last_point_index at p * kp_stride (>= 0: the index of
 *     mvpMapPoints[i]; any negative value, this family's -2 included, = NULL),
 *     d_last_outlier (NULL: none);
 *   the map points d_points + p * mp_stride (mp_stride 0: one array shared by
 *     all problems; pos and has_obs are read; the caller keeps every index
 *     inside the array), their descriptors d_mp_desc + (p * mp_stride + index) * 32.
 * cam, scale_factors (n_levels floats) and the rest are host values.
 * Pinned arithmetic: twc[i] = -((R[i] t0 + R[3+i] t1) + R[6+i] t2) with R, t of
 * the current pose; every other float 3x3 * vector product, tlc = Rlw twc + tlw
 * and x3Dc = Rcw x3Dw + tcw, is ((r0 x + r1 y) + r2 z) + t without contraction;
 * invzc = 1.0f / z (the reference's double division narrowed is the same float).
 * bForward = tlc.z > cam->mb && !mono, bBackward = -tlc.z > cam->mb && !mono.
 * Retry: with retry_below > 0 a problem whose first pass returns fewer than
 * retry_below matches is run again from cleared outputs with 2.0f * th, on the
 * device, that problem alone (Tracking: retry_below = 20).
 * Out: d_kp_match + p * kp_stride (the first d_nkeys[p] entries): the map-point
 * index assigned to the keypoint, -1 untouched, -2 reset by the rotation
 * filter: orb_pose_optimization_batch's d_point_index (with d_points,
 * sizeof(orb_map_point_t), mp_stride); d_info[p].
 * A last-frame keypoint that holds a non-outlier map point and whose octave is
 * outside [0, n_levels) is found on the device: that problem's n_matches and
 * n_matches_first_pass are -1, its kp_match all -1, nothing is read out of
 * bounds.  kp_stride above orb_match_projection_frame_batch_max_stride() (the
 * replay state of one problem lives in the LDS of one CU): ORB_ECAPACITY
 * before anything is launched. */
typedef struct orb_frame_match_info {
  int32_t n_matches;            /* the return value (of the second pass when retried) */
  int32_t n_matches_first_pass; /* the first pass's return value */
  int32_t retried;              /* 1 when the 2 * th pass ran */
  int32_t forward, backward;    /* bForward, bBackward */
} orb_frame_match_info_t;
orb_status_t orb_match_projection_frame_batch(
    orb_matcher_t* m, int n_problems, const orb_keypoint_t* d_keys, const uint8_t* d_desc,
    const float* d_u_right, const uint8_t* d_locked, const int32_t* d_nkeys, int kp_stride,
    const orb_pose_t* d_pose_cur, const orb_pose_t* d_pose_last,
    const orb_keypoint_t* d_last_keys, const int32_t* d_last_nkeys,
    const int32_t* d_last_point_index, const uint8_t* d_last_outlier,
    const orb_map_point_t* d_points, const uint8_t* d_mp_desc, int mp_stride,
    const orb_camera_t* cam, float min_x, float max_x, float min_y, float max_y, int n_levels,
    const float* scale_factors, float th, int mono, int check_orientation, int retry_below,
    int32_t* d_kp_match, orb_frame_match_info_t* d_info, void* stream);
int orb_match_projection_frame_batch_max_stride(void);

/* TrackWithMotionModel's "Discard outliers" loop (src/Tracking.cc:1060-1083)
 * after orb_pose_optimization_batch, per problem, in place on d_kp_match and
 * d_outlier (both at p * kp_stride, d_nkeys[p] entries): a matched keypoint
 * flagged outlier gets kp_match = -1 and outlier = 0.  d_out[p]: n_discarded,
 * n_matches_map = the kept matches whose point has has_obs (nmatchesMap),
 * n_matches = d_info[p].n_matches - n_discarded.
 * mark_seen != 0 (needs mp_stride > 0, else ORB_EINVAL) also marks, in the
 * problem's own records d_points + p * mp_stride, what orb_frustum_batch must
 * skip: a kept match whose point is bad becomes -1 (SearchLocalPoints' first
 * loop, src/Tracking.cc:1333-1354), every other kept point and every discarded
 * point (:1076) gets seen = 1.  IncreaseVisible and the other MapPoint side
 * effects stay with the caller.  mp_stride as above.  Asynchronous on `stream`. */
typedef struct orb_track_discard_info {
  int32_t n_matches, n_matches_map, n_discarded;
} orb_track_discard_info_t;
orb_status_t orb_track_discard_outliers_batch(orb_matcher_t* m, int n_problems,
                                              const int32_t* d_nkeys, int kp_stride,
                                              int32_t* d_kp_match, uint8_t* d_outlier,
                                              orb_map_point_t* d_points, int mp_stride,
                                              int mark_seen,
                                              const orb_frame_match_info_t* d_info,
                                              orb_track_discard_info_t* d_out, void* stream);
/* The same with the match counts read from d_n_matches[p * n_matches_stride]
 * (int32 units, >= 1): the first field of either matcher's info array, stride
 * 5 for orb_frame_match_info_t and orb_bow_match_info_t alike
 * (TrackReferenceKeyFrame's loop, src/Tracking.cc:928-951, takes its count from
 * SearchByBoW).  orb_track_discard_outliers_batch is this entry with
 * &d_info->n_matches and 5. */
orb_status_t orb_track_discard_outliers_batch_n(orb_matcher_t* m, int n_problems,
                                                const int32_t* d_nkeys, int kp_stride,
                                                int32_t* d_kp_match, uint8_t* d_outlier,
                                                orb_map_point_t* d_points, int mp_stride,
                                                int mark_seen, const int32_t* d_n_matches,
                                                int n_matches_stride,
                                                orb_track_discard_info_t* d_out, void* stream);

/* Device-batched SearchByBoW(pKF, F, vpMapPointMatches) (src/ORBmatcher.cc:
 * 164-306) as Tracking::TrackReferenceKeyFrame (src/Tracking.cc:904-954) and
 * Relocalization's candidate loop (:1592-1616) call it: n_problems independent
 * problems in one launch, every array a device pointer, asynchronous on
 * `stream`, no host synchronisation, upload or download.
 * Slots: slot k of the keyframe side (d_kf_*) and of the frame side (d_f_*) is
 * what orb_extractor_extract_batch and orb_vocabulary_transform_batch write
 * with stride kp_stride: keys, point_index, fv_nodes and fv_feats at
 * k * kp_stride, descriptors at 32 * k * kp_stride, fv_offs at
 * k * (kp_stride + 1), the counts nkeys[k] and n_fv_nodes[k].  Of the keys only
 * `angle` is read.  The two sides may be the same allocation.
 * Problem p matches keyframe slot d_kf_index[p] against frame slot
 * d_f_index[p] (either NULL: slot p; a slot may serve many problems; the
 * caller keeps the slot numbers inside the arrays).  d_kf_point_index[i] >= 0
 * names mvpMapPoints[i] in d_points + p * mp_stride (mp_stride 0: one array
 * shared by all problems), any negative value is NULL; isBad() is that
 * record's `bad` byte (d_points NULL: no point is bad); the caller keeps the
 * indices inside the array.
 * Out: d_kp_match + p * kp_stride, the first d_f_nkeys[slot] entries (the rest
 * is not written): the point index assigned to the frame keypoint or -1;
 * matches removed by the rotation filter are -1, as in orb_match_bow.  With
 * identity frame indices this is orb_pose_optimization_batch's d_point_index
 * (with d_points, sizeof(orb_map_point_t), mp_stride).  d_info[p] as below.
 * Per problem the result is orb_match_bow's on the same inputs.
 * min_matches (Tracking: 15; 0: no gate): a problem with fewer matches keeps
 * its counts, gets enough = 0 and every kp_match entry -1 (Tracking returns
 * before it assigns mvpMapPoints).
 * Malformed slots are found on the device: counts are clamped to
 * [0, kp_stride] and n_fv_nodes to [0, count]; an offset that decreases (or a
 * negative first one), an offset above the slot's count or a feature index >=
 * the slot's count in either FeatureVector gives n_matches = -1, the other
 * fields 0 and kp_match all -1 over the clamped count, and nothing is indexed
 * with the bad value.  Ascending node ids are the caller's promise and are
 * NOT checked (the merge-join is a binary search over them).
 * Capacity: one workgroup per problem keeps 8 bytes per keypoint slot in LDS
 * (the match word per frame keypoint and the partner node per keyframe node):
 * 8 * ((kp_stride + 3) & ~3) + 512 bytes must fit the 160 KiB of one CU;
 * orb_match_bow_batch_max_stride() is the largest such kp_stride (a pure
 * function, callable without a device; every stride
 * orb_vocabulary_transform_batch accepts is below it).  Above it:
 * ORB_ECAPACITY before anything is launched, nothing is written.
 * ORB_EINVAL: a null required pointer, n_problems < 0, kp_stride <= 0,
 * mp_stride < 0, nnratio not finite.  n_problems == 0: ORB_OK, no launch.
 * The call takes the handle's mutex; its kernel keeps all state in LDS and the
 * caller's arrays and uses none of the handle's scratch, so it is ordered by
 * `stream` alone. */
typedef struct orb_bow_match_info {
  int32_t n_matches;      /* the return value (after the rotation filter); -1: malformed slot */
  int32_t n_accepted;     /* nmatches before the filter (src/ORBmatcher.cc:262) */
  int32_t n_common_nodes; /* node ids present in both FeatureVectors */
  int32_t n_tried;        /* KF keypoints of common nodes with a non-NULL, non-bad MapPoint */
  int32_t enough;         /* n_matches >= min_matches */
} orb_bow_match_info_t;   /* 20 bytes */
orb_status_t orb_match_bow_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_kf_index, const int32_t* d_f_index,
    const orb_keypoint_t* d_kf_keys, const uint8_t* d_kf_desc, const int32_t* d_kf_nkeys,
    const int32_t* d_kf_point_index, const uint32_t* d_kf_fv_nodes, const int32_t* d_kf_fv_offs,
    const uint32_t* d_kf_fv_feats, const int32_t* d_kf_n_fv_nodes,
    const orb_keypoint_t* d_f_keys, const uint8_t* d_f_desc, const int32_t* d_f_nkeys,
    const uint32_t* d_f_fv_nodes, const int32_t* d_f_fv_offs, const uint32_t* d_f_fv_feats,
    const int32_t* d_f_n_fv_nodes, int kp_stride, const orb_map_point_t* d_points,
    long long mp_stride, float nnratio, int check_orientation, int min_matches,
    int32_t* d_kp_match, orb_bow_match_info_t* d_info, void* stream);
int orb_match_bow_batch_max_stride(void);

/* ------------------------------------------------ UpdateLocalMap on the device */

/* The map as Tracking::UpdateLocalMap reads it: a host struct of device
 * pointers that the caller owns, keeps resident and keeps well-formed (the
 * integrator updates it where LocalMapping inserts or culls keyframes and
 * points).  Keyframes are numbered 0..n_kf-1 and map points
 * 0..n_mp-1; a `*_offs` array has n + 1 ascending entries and list i is
 * [offs[i], offs[i+1]).  Nothing of it is validated: an index outside its
 * array, a decreasing offset or a kf_rank that is not a permutation is the
 * caller's promise and is NOT checked, as the point indices of
 * orb_match_projection_frame_batch are not.  Every pointer is required (an
 * empty list array may be any valid device pointer). */
typedef struct orb_map_view {
  int32_t n_kf, n_mp;
  const int32_t* kf_rank;      /* n_kf: position of keyframe k in the iteration order of
                                  std::map<KeyFrame*,..> / std::set<KeyFrame*> (pointer order in
                                  the drop-in); a permutation of 0..n_kf-1, NOT checked */
  const int32_t* kf_by_rank;   /* its inverse */
  const uint8_t* kf_bad;       /* KeyFrame::isBad() (src/KeyFrame.cc:572) */
  const int32_t* kf_parent;    /* GetParent() (:431), -1 none */
  const int32_t* kf_cov_offs;   const int32_t* kf_cov;   /* mvpOrderedConnectedKeyFrames, best first (:141-187) */
  const int32_t* kf_child_offs; const int32_t* kf_child; /* mspChildrens, any order (:425) */
  const int32_t* kf_mp_offs;    const int32_t* kf_mp;    /* GetMapPointMatches() by keypoint index, <0 = NULL (:283) */
  const int32_t* mp_obs_offs;   const int32_t* mp_obs;   /* keyframes of GetObservations(), any order (src/MapPoint.cc:142) */
  const orb_map_point_t* points;  /* n_mp; bad and has_obs are read and copied through */
  const uint8_t* mp_desc;         /* n_mp x 32 */
} orb_map_view_t;

typedef struct orb_local_map_info {
  int32_t n_local_kf;     /* mvpLocalKeyFrames.size() on return */
  int32_t n_voted;        /* keyframeCounter.size(), bad keyframes included */
  int32_t n_added;        /* keyframes the neighbour pass appended */
  int32_t ref_kf;         /* pKFmax, -1 when none (mpReferenceKF is then left as it is) */
  int32_t max_votes;      /* max */
  int32_t n_local_points; /* mvpLocalMapPoints.size(): the full count, may exceed mp_stride */
  int32_t n_nulled;       /* matched points found bad and set to NULL (:1457) */
  int32_t kept;           /* 1: the counter was empty, the list was kept (:1462) */
} orb_local_map_info_t;   /* 32 bytes */

/* Tracking::UpdateLocalMap (src/Tracking.cc:1395-1404) for n_problems
 * independent frames against one map view, every per-problem array a device
 * pointer, asynchronous on `stream`, no host synchronisation, upload or
 * download.  `view` is a host pointer, read during the call.
 * In: problem p reads d_nkeys[p] (clamped to [0, kp_stride]) and its matches
 * d_kp_match + p * kp_stride (in/out): global point indices as the tracking
 * batches write them with mp_stride 0; any negative value is NULL and is left
 * as it is.  It also reads the list it left for the previous frame,
 * d_local_kf + p * kf_stride with the count d_n_local_kf[p] (both in/out, the
 * count clamped to [0, kf_stride] on entry): when no keyframe gets a vote the
 * reference returns before it clears mvpLocalKeyFrames (:1462), so the list
 * stays exactly as on entry and the points are gathered from it (info.kept =
 * 1; its keyframes are not re-checked for isBad(), as there).  kf_stride >=
 * view->n_kf.
 * Semantics, the reference restated:
 *   vote (:1441-1460): per keypoint, a matched point that is bad becomes -1 in
 *     d_kp_match (n_nulled); every other matched point gives one vote to each
 *     keyframe of its observation list.
 *   voted keyframes in kf_rank order (:1472-1489): bad ones are skipped, the
 *     first whose count is strictly greater than the running maximum is pKFmax
 *     (ref_kf, max_votes), every one that is not bad is appended.  All bad:
 *     the list is empty, ref_kf = -1, there are no local points.
 *   neighbour pass (:1494-1550) over the voted, appended keyframes only: stop
 *     when the list holds more than 80; of the first min(10, size) covisibles
 *     append the first that is not bad and not yet included; append the child
 *     of smallest kf_rank that is not bad and not yet included; a parent that
 *     is not yet included is appended whatever its isBad() and ends the whole
 *     pass (the break at :1546 leaves the outer loop).
 *   UpdateLocalPoints (:1407-1434): the final list in order, each keyframe's
 *     kf_mp in keypoint order; negatives, points already taken for this
 *     problem and bad points are skipped, the rest appended.
 *   SearchLocalPoints' first loop (:1333-1354): a local point that a keypoint
 *     of this frame holds (after the nulling) gets seen = 1 in its gathered
 *     record, every other local point seen = 0, whatever the map's own byte.
 *   IncreaseVisible and the other MapPoint side effects stay with the caller.
 * Out, per problem: the keyframe list and its count; d_local_index +
 * p * mp_stride, the global index of each local point in order; d_mps +
 * p * mp_stride, the gathered records; d_mp_desc + 32 * p * mp_stride, their
 * descriptors; d_nmps[p] = min(n_local_points, mp_stride), only that many
 * entries are written; d_locked + p * kp_stride (d_nkeys[p] entries) =
 * kp_match >= 0 && has_obs; d_info[p].  d_mps, d_mp_desc and d_nmps are
 * orb_frustum_batch's inputs and d_locked is
 * orb_match_projection_local_batch[_stereo]'s, unchanged.
 * Capacity: one workgroup per problem keeps 12 bytes and one bit per keyframe
 * slot in LDS, over K = (kf_stride + 32) & ~31 slots, beside a 12,288-entry
 * hash table (8 bytes each), 2,320 words of staged neighbourhoods and 512
 * static bytes: 98,304 + 9,280 + 12 K + K / 8 + 512 <= 163,840.
 * orb_update_local_map_max_keyframes() is the largest kf_stride that fits (a
 * pure function, callable without a device); view->n_kf or kf_stride above it:
 * ORB_ECAPACITY before anything is launched, nothing is written.
 * The slots of one problem's local keyframes total fewer than 2^30.
 * Tiers: the union's first-occurrence table is that LDS hash table while the
 * local keyframes' slots name at most 9,216 distinct points; a problem that
 * names more runs the union on a table indexed by point id in the handle's
 * device scratch (4 * n_mp bytes per problem, allocated only when n_mp >
 * 9,216).  Because of that scratch the call follows the handle's call-order
 * rule: on a stream other than the previous call's it first makes its stream
 * wait for that call (on the device).
 * ORB_EINVAL: a null required pointer, a negative count, kp_stride <= 0,
 * mp_stride <= 0, kf_stride < view->n_kf.  n_problems == 0: ORB_OK, no launch.
 * The caller's promises, NOT checked: view->mp_desc and d_mp_desc are 16-byte
 * aligned (the gather moves descriptors as two 16-byte words; the records are
 * moved as 4-byte words); the entries of a list that is kept (the first
 * d_n_local_kf[p] of d_local_kf + p * kf_stride on entry) are keyframe numbers
 * in [0, view->n_kf); every non-negative d_kp_match entry is below view->n_mp. */
orb_status_t orb_update_local_map_batch(
    orb_matcher_t* m, int n_problems, const orb_map_view_t* view, const int32_t* d_nkeys,
    int32_t* d_kp_match, int kp_stride, int32_t* d_local_kf, int32_t* d_n_local_kf,
    int kf_stride, int32_t* d_local_index, orb_map_point_t* d_mps, uint8_t* d_mp_desc,
    int32_t* d_nmps, int mp_stride, uint8_t* d_locked, orb_local_map_info_t* d_info,
    void* stream);
int orb_update_local_map_max_keyframes(void);

/* After orb_match_projection_local_batch[_stereo] on the local map above: per
 * problem and keypoint i < d_nkeys[p], d_kp_match[i] = d_local_index[d_km_local[i]]
 * where d_km_local[i] >= 0 (both match arrays at p * kp_stride, d_local_index at
 * p * mp_stride); other entries are unchanged.  The local matcher's last writer
 * has already won inside d_km_local (F.mvpMapPoints[bestIdx] = pMP).  The
 * result is orb_pose_optimization_batch's d_point_index over the view's shared
 * `points` (pt_stride 0).  Every non-negative d_km_local entry is below d_nmps[p]
 * (and so below mp_stride), as the local matcher writes it: the caller's
 * promise, NOT checked.  ORB_EINVAL: a null pointer, a negative count,
 * kp_stride <= 0, mp_stride <= 0.  Asynchronous on `stream`. */
orb_status_t orb_track_local_merge_batch(orb_matcher_t* m, int n_problems,
                                         const int32_t* d_nkeys, int kp_stride,
                                         const int32_t* d_km_local,
                                         const int32_t* d_local_index, int mp_stride,
                                         int32_t* d_kp_match, void* stream);

/* Tracking::TrackLocalMap after PoseOptimization (src/Tracking.cc:1109-1135):
 * d_n_inliers[p] (mnMatchesInliers) counts the keypoints that hold a point
 * (d_kp_match >= 0, an index into d_points + p * pt_stride; pt_stride 0: one
 * shared array), are not flagged in d_outlier and for which only_tracking ||
 * has_obs holds.  null_outliers != 0 (mSensor == System::STEREO only) sets an
 * outlier's d_kp_match to -1.  IncreaseFound and the < 30 / < 50 decision stay
 * with the caller.  ORB_EINVAL: a null pointer, a negative count or stride,
 * kp_stride <= 0.  Asynchronous on `stream`. */
orb_status_t orb_track_local_map_finish_batch(orb_matcher_t* m, int n_problems,
                                              const int32_t* d_nkeys, int kp_stride,
                                              int32_t* d_kp_match, const uint8_t* d_outlier,
                                              const orb_map_point_t* d_points,
                                              long long pt_stride, int only_tracking,
                                              int null_outliers, int32_t* d_n_inliers,
                                              void* stream);

/* ------------------------------------------------- Sim3Solver on the device */

/* Sim3Solver (src/Sim3Solver.cc, include/Sim3Solver.h) for n_problems
 * independent (pKF1, pKF2, vpMatched12) problems as LoopClosing::ComputeSim3
 * runs them: one call builds the solvers (the constructor and
 * SetRansacParameters), one runs iterate(n) on every solver that is still
 * active.  Every per-problem array is a device pointer, both calls are
 * asynchronous on `stream`, neither synchronises with the host, and neither
 * uses the handle's scratch, so both are ordered by `stream` alone.  The
 * caller owns the state and correspondence arrays; they are the solver's
 * members between calls.
 *
 * One correspondence the constructor's loop (:62-105) keeps, in ascending i1. */
typedef struct orb_sim3_corr {
  int32_t index1;      /* mvnIndices1: i1 */
  float x1[3];         /* mvX3Dc1 = Rcw1 * pos(pMP1) + tcw1 */
  float x2[3];         /* mvX3Dc2 = Rcw2 * pos(pMP2) + tcw2 */
  float p1[2];         /* mvP1im1 (FromCameraToImage, mK1) */
  float p2[2];         /* mvP2im2 (mK2) */
  float max_err1;      /* mvnMaxError1: the size_t (9.210 * sigma2, truncated) as the float */
  float max_err2;      /*   the comparison err < maxError converts it to; mvnMaxError2 */
  uint8_t best_inlier; /* mvbBestInliers */
  uint8_t _pad[3];     /* written as 0 */
} orb_sim3_corr_t;     /* 56 bytes */

typedef struct orb_sim3_state {
  int32_t status;         /* 0; -1: malformed slot or draw, every later iterate returns "no more" */
  int32_t n1;             /* mN1 = vpMatched12.size() (keyframe 1's clamped count) */
  int32_t n;              /* N = mvpMapPoints1.size() */
  int32_t max_its;        /* mRansacMaxIts after SetRansacParameters (0 when N < min_inliers) */
  int32_t iterations;     /* mnIterations */
  int32_t best_inliers;   /* mnBestInliers */
  int32_t best_iteration; /* the 1-based lifetime iteration that produced the best (0: none) */
  int32_t min_inliers;    /* mRansacMinInliers */
  int32_t fix_scale;      /* mbFixScale */
  float best_scale;       /* mBestScale (0 until an iteration is taken) */
  float best_R[9];        /* mBestRotation, row-major */
  float best_t[3];        /* mBestTranslation */
  float best_T12[16];     /* mBestT12, row-major */
  float k1[4], k2[4];     /* fx, fy, cx, cy of mK1 and mK2 */
} orb_sim3_state_t;       /* 184 bytes */

typedef struct orb_sim3_result {
  int32_t has_sim3;       /* iterate returned a non-empty Mat */
  int32_t no_more;        /* bNoMore */
  int32_t n_inliers;      /* nInliers (0 unless has_sim3) */
  int32_t iterations_run; /* nCurrentIterations of this call */
  float T12[16];          /* the returned mBestT12; the four below: zeros unless has_sim3 */
  float R[9];             /* GetEstimatedRotation() */
  float t[3];             /* GetEstimatedTranslation() */
  float scale;            /* GetEstimatedScale() */
} orb_sim3_result_t;      /* 132 bytes */

/* The constructor and SetRansacParameters (:37-141).
 * Slots, as orb_match_bow_batch lays keyframes out: slot k has mvKeysUn at
 * d_kf_keys + k * kp_stride, GetMapPointMatches() as indices into d_points at
 * d_kf_point_index + k * kp_stride (any negative value is NULL), its count
 * d_kf_nkeys[k] (clamped to [0, kp_stride]) and its pose d_kf_pose[k] (rcw and
 * tcw are read).  Problem p uses slots d_kf1_slot[p] and d_kf2_slot[p] (either
 * NULL: slot p; a slot may serve many problems).  d_points is one array shared
 * by all problems (pos and bad are read); the caller keeps every non-negative
 * point index inside it and every slot number inside the slot arrays (NOT
 * checked).
 * Matches: d_match12 + p * kp_stride holds, per i1 < mN1, the global point
 * index of vpMatched12[i1] (negative: NULL); d_index2 + p * kp_stride holds
 * pMP2->GetIndexInKeyFrame(pKF2) (the matchers' bestIdx2); d_index1 is optional
 * (NULL: i1), else pMP1->GetIndexInKeyFrame(pKF1).
 * Skips, in the reference's order: NULL match, NULL pMP1, either point bad,
 * either index negative.  A kept correspondence whose index is at or above its
 * keyframe's clamped count, or whose keypoint's octave is outside
 * [0, n_levels), makes the problem malformed: status = -1, n1 as usual, every
 * other state field 0, no correspondence written, and nothing is indexed with
 * the bad value.
 * Host values: level_sigma2[n_levels] (mvLevelSigma2; 1 <= n_levels <= 16, each
 * finite and in [0, 1e15]), cam1 / cam2 (fx, fy, cx, cy are read), fix_scale,
 * probability (strictly between 0 and 1), min_inliers (>= 3: below it the
 * reference would call RandomInt(0, -1)), max_iterations (>= 1).
 * Out: d_state[p]; d_corr + p * kp_stride, the first `n` records (the rest is
 * not written), best_inlier 0.  max_its: N < min_inliers stores 0 (iterate
 * never reads it); N == min_inliers gives 1; otherwise epsilon =
 * (float)min_inliers / N and ceil(log(1 - p) / log(1 - pow(epsilon, 3))),
 * clamped to [1, max_iterations].
 * Capacity: iterate keeps 48 bytes per correspondence slot and (SIM3_CHUNK +
 * 1) bits per slot in LDS over kp_stride rounded up to 64, beside 8 KiB of
 * static state; orb_sim3_solver_max_stride() is the largest kp_stride that
 * fits the 160 KiB of one CU (a pure function, callable without a device).
 * Above it both calls return ORB_ECAPACITY before anything is launched, and
 * nothing is written.
 * ORB_EINVAL: a null required pointer, n_problems < 0, kp_stride <= 0, a host
 * value outside the ranges above.  n_problems == 0: ORB_OK, no launch. */
orb_status_t orb_sim3_solver_setup_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
    const orb_keypoint_t* d_kf_keys, const int32_t* d_kf_nkeys, const int32_t* d_kf_point_index,
    const orb_pose_t* d_kf_pose, int kp_stride, const orb_map_point_t* d_points,
    const int32_t* d_match12, const int32_t* d_index1, const int32_t* d_index2,
    const float* level_sigma2, int n_levels, const orb_camera_t* cam1, const orb_camera_t* cam2,
    int fix_scale, double probability, int min_inliers, int max_iterations,
    orb_sim3_state_t* d_state, orb_sim3_corr_t* d_corr, void* stream);
int orb_sim3_solver_max_stride(void);

/* iterate(n_iterations) (:144-214) on every problem (find(): n_iterations =
 * max_iterations).  d_active is optional (vbDiscarded inverted): a problem with
 * d_active[p] == 0 is skipped and nothing of it is read or written.
 * Draws: d_draws + p * draw_stride, raw rand() values.  Entry 3 * it + j
 * serves lifetime iteration `it` (mnIterations before its increment), draw j.
 * The device evaluates DUtils::Random::RandomInt(0, size - 1)
 * (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) as
 * (int)(((double)r / ((double)rand_max + 1.0)) * size) with size = N, N - 1,
 * N - 2 and removes each pick by the swap with the back of :175-183.  One draw
 * stream per solver: the reference's single global rand() sequence interleaves
 * the solvers of ComputeSim3's round-robin, and its order is the integrator's
 * to reproduce.  A consumed r > rand_max makes the problem
 * malformed: the iteration that reads it is not run and not counted, status
 * becomes -1, the best of the earlier iterations stays, and the call returns
 * "no more" without a Sim3.  max_iterations is the value given to setup (the
 * device clamps the state's max_its to it); draw_stride < 3 * max_iterations
 * is ORB_EINVAL.
 * Per iteration ComputeSim3 (:237-351) and CheckInliers (:354-378), IEEE
 * throughout with nothing special-cased (identical points: den = 0; a zero
 * imaginary part: vec / 0; z = 0), then the acceptance rule in iteration order
 * (:190-207): the best is taken on >=, the call returns on the first
 * mnInliersi > mRansacMinInliers (strict), vbInliers is indexed through
 * mvnIndices1; on success bNoMore stays false even at the last allowed
 * iteration, and the next call runs nothing and returns bNoMore.  N <
 * min_inliers, or status < 0, returns bNoMore at once.  The hypotheses of a
 * call are evaluated side by side and the rule is replayed over them in order;
 * work past a return is never visible, and the state after k calls of
 * iterate(5) equals, bit for bit, the state after one call that runs the same
 * iterations.
 * Out: d_inliers12 + p * kp_stride, n1 bytes (vbInliers; all 0 unless a Sim3
 * is returned); d_result[p]; the updated d_state[p] and the best_inlier bytes
 * of d_corr.  ORB_EINVAL: a null required pointer, a negative count, kp_stride
 * <= 0, max_iterations < 1, draw_stride < 3 * max_iterations.  n_problems ==
 * 0: ORB_OK, no launch.
 *
 * Pins (the same list stands in tests/sim3_ref.py and DESIGN.md 4.9; OpenCV
 * itself is not available to the project: unpinned against a real OpenCV).
 * Float expressions are evaluated as written, no contraction.
 *  P1  Rcw * X + tcw (constructor, Project): ((r0 x + r1 y) + r2 z) + t in
 *      float, the project's existing pin; 1 / z, x * invz, fx * x + cx in float.
 *  P2  scalar * Mat and Mat / scalar: the double scalar narrowed to float, then
 *      v * s + 0.0f per element (cvtScale_).  C / P.cols is
 *      c * (float)(1.0 / 3) + 0.0f; 2 * ang * vec / norm(vec) has
 *      s = (float)((2.0 * ang) * (1.0 / norm)); sR = R * ms12i;
 *      sRinv = R^T * (float)(1.0 / (double)ms12i).
 *  P3  cv::reduce(P, C, 1, CV_REDUCE_SUM) over three columns:
 *      (p0 + p2) + p1 in float (reduceC_'s two accumulators).
 *  P4  A * B.t() (M = Pr2 * Pr1.t()): per element a double accumulator from 0,
 *      k ascending, exact double products, narrowed once to float.
 *  P5  A * B of 3 x 3 floats without a transpose (P3 = R * Pr2):
 *      (a0 b0 + a1 b1) + a2 b2 in float.
 *  P6  N11..N44: the float expressions as written, left to right (the doubles
 *      that hold them narrow back to the same floats).
 *  P7  cv::eigen on the symmetric 4 x 4 float matrix: OpenCV 3.x's
 *      JacobiImpl_<float>, step by step: V = I, W = diag(A); indR[k] = the first
 *      largest |A[k][m]|, m > k; indC[k] = the first largest |A[i][k]|, i < k;
 *      up to 30 n^2 = 480 sweeps of: the pivot (k, l) = the first largest of
 *      |A[i][indR[i]]|, i = 0..n-2, then of |A[indC[i]][i]|, i = 1..n-1
 *      (strictly larger replaces); p = A[k][l]; stop when |p| <= FLT_EPSILON;
 *      y = (float)((W[l] - W[k]) * 0.5); t = |y| + hypot(p, y); s = hypot(p, t);
 *      c = t / s; s = p / s; t = (p / t) * p; y < 0 negates s and t;
 *      A[k][l] = 0; W[k] -= t; W[l] += t; rotate(a, b) = (a c - b s, a s + b c)
 *      over (A[i][k], A[i][l]) i < k, (A[k][i], A[i][l]) k < i < l,
 *      (A[k][i], A[l][i]) i > l, and (V[k][i], V[l][i]) all i; indR and indC
 *      recomputed for k and l only.  Then a selection sort, descending (swap
 *      with the first largest remaining, strict <), eigenvectors as rows.
 *      hypot(a, b) = (float)sqrt((double)a * a + (double)b * b).
 *  P8  cv::norm(vec): sqrt(((0 + v0 v0) + v1 v1) + v2 v2), products and sums in
 *      double; cv::norm returns that double.
 *  P9  atan2 on doubles: fdlibm's e_atan2.c over s_atan.c, built from IEEE
 *      operations alone (pinned_atan2), no libm call on either side.
 *  P10 cv::Rodrigues, vector to matrix, in double: theta = sqrt((rx rx + ry ry)
 *      + rz rz); theta < DBL_EPSILON gives I; else c, s = pinned_sincos_d(theta),
 *      c1 = 1 - c, r *= 1 / theta, R_ij = (c I_ij + c1 r_i r_j) + s [r]x_ij,
 *      each narrowed to float.
 *  P11 Mat::dot: a double accumulator over the elements row-major, unrolled by
 *      four: r += ((p0 + p1) + p2) + p3 per group, then r += p one at a time,
 *      with exact double products (nom over nine elements, err over two).
 *  P12 cv::pow(P3, 2): x * x in float; den adds those floats into a double,
 *      row-major; ms12i = (float)(nom / den).
 *  P13 the folded O1 - ms12i * mR12i * O2 (one gemm): u_k = (R_k0 o0 + R_k1 o1)
 *      + R_k2 o2 in float, t_k = (float)((double)u_k * -(double)ms12i +
 *      (double)O1_k).
 *  P14 tinv = -sRinv * mt12i: 0.0f - ((a0 t0 + a1 t1) + a2 t2) in float.
 *  P15 pow(epsilon, 3) = (x * x) * x in double; log = pinned_log; sin and cos =
 *      pinned_sincos_d; sqrt and / are IEEE.
 *  P16 thresholds: (float)(uint64_t)(9.210 * (double)sigma2). */
orb_status_t orb_sim3_solver_iterate_batch(
    orb_matcher_t* m, int n_problems, int kp_stride, orb_sim3_state_t* d_state,
    orb_sim3_corr_t* d_corr, const uint32_t* d_draws, int draw_stride, uint32_t rand_max,
    int max_iterations, int n_iterations, const uint8_t* d_active, uint8_t* d_inliers12,
    orb_sim3_result_t* d_result, void* stream);

/* ------------------------------- LocalMapping::CreateNewMapPoints on the device */

/* KeyFrame::ComputeSceneMedianDepth(q) (src/KeyFrame.cc:658-694) for n_problems
 * keyframe slots in the slot layout of orb_match_bow_batch /
 * orb_sim3_solver_setup_batch: problem p names slot d_slot[p] (NULL: slot p),
 * whose count d_kf_nkeys[k] is clamped to [0, kp_stride], whose
 * GetMapPointMatches() are indices into d_points at d_kf_point_index + k *
 * kp_stride (any negative value is NULL; the reference does not ask isBad) and
 * whose pose is d_kf_pose[k] (rcw row 2 and tcw[2] are read).  pos of d_points
 * is read; the caller keeps every non-negative index inside it (NOT checked).
 * Out: d_count[p] = vDepths.size(); d_median[p] = vDepths[(size - 1) / q] of
 * the ascending depths, NaN when the keyframe has no point (the reference
 * indexes an empty vector there).  The order statistic is found by rank
 * counting over keys staged in LDS; "ascending" is the total order of the float
 * bit patterns (-0 before +0, a NaN depth past the infinity of its sign), which
 * is std::sort's order on everything the reference defines.
 * Pin N1 below is the depth.  kp_stride above
 * orb_scene_median_depth_max_stride() (4 bytes of LDS per slot in the 160 KiB of
 * one CU; a pure function): ORB_ECAPACITY before any launch.  ORB_EINVAL: a null
 * required pointer, n_problems < 0, kp_stride <= 0, q < 1.  n_problems == 0:
 * ORB_OK, no launch.  Asynchronous on `stream`, no handle scratch. */
orb_status_t orb_scene_median_depth_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_slot, const int32_t* d_kf_nkeys,
    const int32_t* d_kf_point_index, const orb_pose_t* d_kf_pose, int kp_stride,
    const orb_map_point_t* d_points, int q, float* d_median, int32_t* d_count, void* stream);
int orb_scene_median_depth_max_stride(void);
/* One keyframe, host buffers: point_index[n] into points[n_points] (a
 * non-negative index at or above n_points is ORB_EINVAL). */
orb_status_t orb_scene_median_depth(orb_matcher_t* m, int n, const int32_t* point_index,
                                    const orb_pose_t* pose, const orb_map_point_t* points,
                                    int n_points, int q, float* median, int32_t* count);

/* One status byte per keypoint of the current keyframe: one code per `continue`
 * of the loop body (src/LocalMapping.cc:341-512). */
#define ORB_NP_NOT_TRIED 0     /* the pair was gated (or the slot is past the count) */
#define ORB_NP_NO_MATCH 1      /* match12[i1] < 0: not in vMatchedIndices */
#define ORB_NP_ACCEPTED 2      /* a map point was created */
#define ORB_NP_LOW_PARALLAX 3  /* :412-414 no stereo and very low parallax */
#define ORB_NP_W_ZERO 4        /* :395 x3D.at<float>(3) == 0 */
#define ORB_NP_Z1 5            /* :421 z1 <= 0 */
#define ORB_NP_Z2 6            /* :425 z2 <= 0 */
#define ORB_NP_REPROJ1 7       /* :447 / :458 */
#define ORB_NP_REPROJ2 8       /* :474 / :485 */
#define ORB_NP_ZERO_DIST 9     /* :498 dist1 == 0 || dist2 == 0 */
#define ORB_NP_SCALE_RATIO 10  /* :511 */
#define ORB_NP_UNDEFINED 11    /* undefined in the reference; rejected, see below */
#define ORB_NP_NSTATUS 12

typedef struct orb_new_point_info {
  int32_t gated;        /* the pair was skipped at :299 / :309 */
  int32_t overflow;     /* cursor + n_new > point_capacity: nothing else was written */
  int32_t n_new;        /* nnew of this pair */
  int32_t first_point;  /* the cursor before the call: point i is first_point + i */
  int32_t counts[ORB_NP_NSTATUS]; /* keypoints per status; [ORB_NP_NOT_TRIED] stays 0 */
} orb_new_point_info_t;  /* 64 bytes */

/* The neighbour loop's gate (src/LocalMapping.cc:289-311) and body (:338-535)
 * for n_problems (current keyframe, neighbour) pairs.  Problem p reads slots
 * d_kf1_slot[p] (mpCurrentKeyFrame) and d_kf2_slot[p] (pKF2) of the slot arrays
 * above plus d_kf_keys (mvKeysUn), d_kf_u_right (mvuRight) and d_kf_depth
 * (mvDepth) at k * kp_stride (both NULL: monocular keyframes, every mvuRight
 * is -1).  d_match12 + p * kp_stride holds what orb_search_for_triangulation
 * (or orb_search_for_triangulation_batch, on the device) writes: per keypoint
 * of KF1 the index in KF2, or a negative value; vMatchedIndices is its
 * non-negative entries in ascending index.  An index of KF2 may repeat: the
 * matcher never sets vbMatched2 (src/ORBmatcher.cc:744-797), so several
 * keypoints of KF1 can take one keypoint of KF2.  Every accepted match still
 * creates its point and its pair, and KF2's d_kf_point_index entry ends as the
 * id of the largest accepted i1 that names it, as the reference's sequential
 * AddMapPoint calls leave it: ids ascend with i1 and the store is an atomic
 * maximum, which is that id whenever the entry's previous value is below the
 * cursor (always so for an entry the matcher can return: it is negative).
 * ComputeF12 and the matcher are not part of this call, and neither is
 * ComputeDistinctiveDescriptors (orb_distinctive_descriptors_batch).
 * Host values: cam1, cam2 (all six fields; invfx = 1.0f / fx on the host as
 * src/Frame.cc:115), scale_factors[n_levels] (mvScaleFactors; mfScaleFactor is
 * read as scale_factors[1], which is 1.0f * scaleFactor exactly, so 2 <=
 * n_levels <= 16), level_sigma2[n_levels] (mvLevelSigma2), monocular
 * (mbMonocular).  d_median_depth[p] = ComputeSceneMedianDepth(2) of the
 * neighbour (orb_scene_median_depth_batch), read only when monocular.
 * Gate: baseline = (float)cv::norm(Ow2 - Ow1) (N3).  Stereo: baseline <
 * cam2->mb skips the pair.  Monocular: (double)(baseline / median) < 0.01 skips
 * it, and so does a NaN median.  A skipped pair writes info.gated = 1,
 * first_point, zero counts and ORB_NP_NOT_TRIED for every keypoint below KF1's
 * count; nothing else.
 * Per match the reference's tests in its order, its two quirks included:
 * cosParallaxStereo2 is evaluated only when KF1's keypoint is not stereo (the
 * `else if` of :372), and KF2's right-image reprojection uses the current
 * keyframe's mbf (:480).  bStereo = mvuRight >= 0.  The three branches are the
 * linear triangulation (:383-399), UnprojectStereo(idx1) and
 * UnprojectStereo(idx2) with the arithmetic of orb_unproject_stereo over
 * d_kf_keys (KeyFrame::UnprojectStereo reads mvKeys; the stereo keyframes of
 * this library are rectified, mvKeys == mvKeysUn).
 * ORB_NP_UNDEFINED, tested before any arithmetic: idx2 at or above KF2's
 * clamped count, an octave of either keypoint outside [0, n_levels), or a
 * stereo flag on either keypoint whose depth is not > 0 (UnprojectStereo would
 * return an empty Mat).  Nothing is indexed with the bad value.
 * Out, per keypoint i1 below KF1's clamped count: d_status[p * kp_stride + i1];
 * d_x3d + 3 * (p * kp_stride + i1) = x3D for every status that has one
 * (ACCEPTED and Z1 .. SCALE_RATIO), untouched otherwise.
 * Accepted matches in ascending i1 (the reference's creation order): the i-th
 * becomes point c + i of d_points with c = d_point_cursor[d_cursor_index[p]]
 * (a complete record: pos; normal, min_distance, max_distance as
 * MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:349-402) gives them for the
 * observations {KF1, KF2} with reference keyframe KF1 -- with two observations
 * the sum 0 + a + b of unit vectors does not depend on the std::map<KeyFrame*>
 * order, float addition being commutative --; bad = 0, seen = 0, has_obs = 1,
 * _pad = 0); d_new_pairs + 2 * (p * kp_stride + i) = (i1, idx2); c + i is
 * stored at i1 of KF1's and at idx2 of KF2's d_kf_point_index row (the two
 * AddMapPoint calls: the next neighbour's orb_search_for_triangulation must see
 * them); the cursor advances by n_new.  d_info[p] as above.  If c < 0 or c +
 * n_new > point_capacity the problem writes d_info[p] = {overflow = 1, rest 0}
 * and nothing else.
 * The caller's promises, NOT checked: the problems of one call share no cursor
 * and no keyframe slot, and every slot number is inside the slot arrays.  The
 * neighbours of one keyframe go in successive calls on one stream, as the
 * reference runs them in sequence; the batch is independent keyframes / maps.
 * Capacity: 16 bytes of LDS per slot (a problem's statuses and points wait
 * there until its count is known); kp_stride above
 * orb_create_new_map_points_max_stride() is ORB_ECAPACITY before any launch.
 * ORB_EINVAL: a null required pointer (d_kf_u_right and d_kf_depth both or
 * neither; d_median_depth required when monocular), n_problems < 0, kp_stride
 * <= 0, point_capacity < 0, n_levels outside [2, 16], a scale factor or sigma2
 * that is not finite and positive.  n_problems == 0: ORB_OK, no launch.
 * Asynchronous on `stream`, no handle scratch, ordered by `stream` alone.
 *
 * Pins (the same list stands in tests/newpoints_ref.py and DESIGN.md 4.10;
 * all unpinned against a real OpenCV).  Float expressions as written, no
 * contraction; P-numbers are the Sim3 solver's pins above.
 *  N1  Mat::dot of two 3-vectors (P11 below four elements): ((0 + p0) + p1) +
 *      p2 with exact double products; row.dot(x) + t adds the float t widened,
 *      in double, and narrows once: z of the median, x1 y1 z1 x2 y2 z2.
 *  N2  xn = ((u - cx) * invfx, (v - cy) * invfy, 1); ray = Rwc * xn as 3 x 3 by
 *      3 x 1 float products summed left to right: (rcw[i] x + rcw[3 + i] y) +
 *      rcw[6 + i] * 1.0f.
 *  N3  cv::norm (P8): the sqrt of a double sum, returned as a double.
 *      cosParallaxRays = (float)(dot / (norm1 * norm2)), all in double (N1).
 *  N4  cos(2 * atan2(mb / 2, depth)) on floats: a = (float)pinned_atan2 of the
 *      widened mb / 2.0f and depth; (float) of pinned_sincos_d's cosine of the
 *      widened 2.0f * a.  profiles/newpoints_libm.json counts how often glibc's
 *      atan2f / cosf differ.
 *  N5  A.row(r) = xn * T.row(2) - T.row(r) (addWeighted, beta = -1, gamma = 0):
 *      (xn * T2k + Trk * -1.0f) + 0.0f per element, in float.
 *  N6  cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) on 4 x 4 float: OpenCV
 *      3.x JacobiSVDImpl_<float> on At (row i of At = column i of A).  W[i] = the
 *      double sum of squares of row i, k ascending from 0; Vt = I.  At most
 *      max(m, 30) = 30 sweeps over the pairs i < j in order; p = the double dot
 *      of rows i and j; the pair is skipped when |p| <= eps * sqrt(a * b), eps =
 *      (double)(2 * FLT_EPSILON), a = W[i], b = W[j]; p *= 2; beta = a - b;
 *      gamma = hypot(p, beta) = sqrt(p * p + beta * beta) in double (P7's
 *      hypot, not narrowed); beta < 0: s = (float)sqrt(((gamma - beta) * 0.5) /
 *      gamma), c = (float)(p / ((gamma * s) * 2)); otherwise c =
 *      (float)sqrt((gamma + beta) / (gamma * 2)), s = (float)(p / ((gamma * c) *
 *      2)); both rows of At and of Vt rotate in float: t0 = c * x + s * y, t1 =
 *      (-s) * x + c * y; a and b are re-summed in double from the rotated rows;
 *      the loop stops after a sweep without a rotation; W[i] = sqrt of the
 *      re-summed squares; selection sort, descending: swap with the first later
 *      maximum under strict <, the rows of Vt moving along.  Only vt.row(3) is
 *      used; U's normalisation is not reproduced.
 *  N7  x3D = v[0..2] / v[3] is Mat / double scalar, P2's statement: v * (float)
 *      (1.0 / (double)v3) + 0.0f (adopted, as cvtScale_ evaluates it); one
 *      correctly rounded float divide per element is the rejected alternative.
 *      normali / cv::norm(normali) likewise: v * (float)(1.0 / norm) + 0.0f;
 *      normal / n with n = 2: v * (float)(1.0 / 2.0) + 0.0f.
 *  N8  UnprojectStereo: the statement of orb_unproject_stereo.
 *  N9  double constants: (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2,
 *      the three-term float sum (ex ex + ey ey) + er er against 7.8 *
 *      (double)sigma2; invz = (float)(1.0 / (double)z); cosParallaxRays <
 *      0.9998 and baseline / median < 0.01 compared in double; u = (fx * x) *
 *      invz + cx, u_r = u - mbf * invz in float; cosParallaxRays + 1 in float.
 *  N10 dist = (float)cv::norm(x3D - Ow) (N3); ratioDist = dist2 / dist1,
 *      ratioOctave = sf[o1] / sf[o2], ratioFactor = 1.5f * sf[1], max_distance =
 *      dist1 * sf[o1], min_distance = max_distance / sf[n_levels - 1]: float. */
orb_status_t orb_create_new_map_points_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
    const orb_keypoint_t* d_kf_keys, const int32_t* d_kf_nkeys, int32_t* d_kf_point_index,
    const orb_pose_t* d_kf_pose, const float* d_kf_u_right, const float* d_kf_depth,
    int kp_stride, const int32_t* d_match12, const float* d_median_depth,
    const orb_camera_t* cam1, const orb_camera_t* cam2, const float* scale_factors,
    const float* level_sigma2, int n_levels, int monocular, orb_map_point_t* d_points,
    int point_capacity, int32_t* d_point_cursor, const int32_t* d_cursor_index,
    uint8_t* d_status, float* d_x3d, int32_t* d_new_pairs, orb_new_point_info_t* d_info,
    void* stream);
int orb_create_new_map_points_max_stride(void);
/* One pair, host buffers.  keys / u_right / depth / point_index per keyframe
 * (u_right1, depth1, u_right2, depth2 all NULL: monocular keyframes);
 * point_index1[n1] and point_index2[n2] are updated in place; points
 * [point_capacity] receives records *cursor .. *cursor + n_new - 1 and *cursor
 * advances; status[n1], x3d[3 * n1], new_pairs[2 * n1] as above (entries the
 * device leaves untouched keep the caller's value). */
orb_status_t orb_create_new_map_points(
    orb_matcher_t* m, int n1, const orb_keypoint_t* keys1, const float* u_right1,
    const float* depth1, int32_t* point_index1, const orb_pose_t* pose1, int n2,
    const orb_keypoint_t* keys2, const float* u_right2, const float* depth2,
    int32_t* point_index2, const orb_pose_t* pose2, const int32_t* match12, float median_depth,
    const orb_camera_t* cam1, const orb_camera_t* cam2, const float* scale_factors,
    const float* level_sigma2, int n_levels, int monocular, orb_map_point_t* points,
    int point_capacity, int32_t* cursor, uint8_t* status, float* x3d, int32_t* new_pairs,
    orb_new_point_info_t* info);

/* Device-batched SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs,
 * bOnlyStereo) (src/ORBmatcher.cc:718-901) as the neighbour loop of
 * LocalMapping::CreateNewMapPoints calls it (src/LocalMapping.cc:313-318):
 * n_problems independent (KF1, KF2) problems in one launch, every array a
 * device pointer, asynchronous on `stream`, no host synchronisation, upload or
 * download.  The arrays are the keyframe slot arrays orb_match_bow_batch and
 * orb_create_new_map_points_batch take, so the same allocations pass unchanged:
 * slot k has d_kf_keys (mvKeysUn), d_kf_point_index, d_kf_fv_nodes and
 * d_kf_fv_feats at k * kp_stride, d_kf_desc at 32 * k * kp_stride, d_kf_fv_offs
 * at k * (kp_stride + 1), the counts d_kf_nkeys[k] and d_kf_n_fv_nodes[k],
 * d_kf_u_right (mvuRight) at k * kp_stride (NULL: every keypoint is monocular)
 * and the pose d_kf_pose[k].  Problem p matches slot d_kf1_slot[p]
 * (mpCurrentKeyFrame) against slot d_kf2_slot[p] (pKF2); a slot may serve many
 * problems on either side; the caller keeps the slot numbers inside the arrays
 * (NOT checked).  d_f12 + 9 * p is ComputeF12(pKF1, pKF2), row-major.
 * Host values: cam2 (fx, fy, cx, cy of pKF2 are read), scale_factors[n_levels]
 * and level_sigma2[n_levels] of pKF2, only_stereo (bOnlyStereo),
 * check_orientation (mbCheckOrientation).
 * Derived on the device: GetMapPoint(i) != NULL is d_kf_point_index[i] >= 0 (a
 * keypoint with a point is skipped on either side; isBad is not asked, :768,
 * :792); stereo is mvuRight >= 0 (0.0 is stereo); the epipole of KF1 in KF2
 * (:728-733) from d_kf_pose[kf1].ow and d_kf_pose[kf2].rcw / tcw with the
 * arithmetic of orb_search_for_triangulation: C2 = ((r0 x + r1 y) + r2 z) + t
 * row by row, invz = 1.0f / C2z, ex = (fx * C2x) * invz + cx, in float, left to
 * right, no contraction.  An infinite or NaN epipole behaves as in the
 * reference: the `<` of the epipole gate (:814-821) is false and nothing is
 * skipped.
 * Out: d_match12 + p * kp_stride, every entry below KF1's clamped count (the
 * rest is not written): the KF2 index matched to the KF1 keypoint, or -1; this
 * is the row orb_create_new_map_points_batch reads.  d_info[p] as below.  Per
 * problem the row and n_matches are orb_search_for_triangulation's on the same
 * inputs: the last passing candidate of minimum distance wins, dist <= 50, the
 * epipole gate on mono-mono pairs only, den == 0 rejects, (double)dsqr < 3.84
 * * (double)sigma2[octave of the KF2 keypoint], the rotation histogram with
 * the strict three-maxima scan.  vbMatched2 is never set in the reference, so
 * one KF2 index may be the match of several KF1 keypoints (n_shared2).
 * Malformed slots are found on the device exactly as orb_match_bow_batch finds
 * them: counts are clamped to [0, kp_stride] and n_fv_nodes to [0, count]; an
 * offset that decreases (or a negative first one), an offset above the slot's
 * count or a feature index >= the slot's count in either FeatureVector gives
 * n_matches = -1, the other fields 0 and the row all -1 over KF1's clamped
 * count, and nothing is indexed with the bad value.  A KF2 keypoint whose
 * octave is outside [0, n_levels) is undefined in the reference (it reads past
 * mvScaleFactors / mvLevelSigma2): a candidate that passes the point, stereo
 * and distance tests and has such an octave is skipped without indexing and
 * counted, once per (KF1 keypoint, candidate) pair, in n_undefined.  Ascending
 * node ids and a feature listed in one node only are the caller's promise and
 * are NOT checked (the node join is a binary search over the ids).
 * Capacity: one workgroup per problem keeps 8 bytes per keypoint slot in LDS
 * (the match word per KF1 keypoint; the partner node per KF1 node, later the
 * match count per KF2 keypoint): 8 * ((kp_stride + 3) & ~3) + 1024 bytes must
 * fit the 160 KiB of one CU; orb_search_for_triangulation_batch_max_stride()
 * is the largest such kp_stride (a pure function, callable without a device;
 * it is above orb_create_new_map_points_max_stride(), so the two calls chain at
 * every stride the second accepts).  Above it: ORB_ECAPACITY before anything is
 * launched, nothing is written.
 * ORB_EINVAL: a null required pointer (all but d_kf_u_right), n_problems < 0,
 * kp_stride <= 0, n_levels outside [1, 16], a scale factor or sigma2 that is
 * not finite and positive.  n_problems == 0: ORB_OK, no launch.
 * The call takes the handle's mutex; its kernel keeps all state in LDS and the
 * caller's arrays and uses none of the handle's scratch, so it is ordered by
 * `stream` alone. */
typedef struct orb_tri_match_info {
  int32_t n_matches;      /* the return value (after the rotation filter); -1: malformed slot */
  int32_t n_accepted;     /* nmatches before the filter (src/ORBmatcher.cc:835) */
  int32_t n_common_nodes; /* node ids present in both FeatureVectors */
  int32_t n_tried;        /* KF1 keypoints of common nodes that pass the point and stereo tests */
  int32_t n_shared2;      /* final matches whose KF2 index another final match names too */
  int32_t n_undefined;    /* candidates skipped for an octave outside [0, n_levels) */
} orb_tri_match_info_t;   /* 24 bytes */
orb_status_t orb_search_for_triangulation_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
    const orb_keypoint_t* d_kf_keys, const uint8_t* d_kf_desc, const int32_t* d_kf_nkeys,
    const int32_t* d_kf_point_index, const uint32_t* d_kf_fv_nodes, const int32_t* d_kf_fv_offs,
    const uint32_t* d_kf_fv_feats, const int32_t* d_kf_n_fv_nodes, const float* d_kf_u_right,
    const orb_pose_t* d_kf_pose, int kp_stride, const float* d_f12, const orb_camera_t* cam2,
    const float* scale_factors, const float* level_sigma2, int n_levels, int only_stereo,
    int check_orientation, int32_t* d_match12, orb_tri_match_info_t* d_info, void* stream);
int orb_search_for_triangulation_batch_max_stride(void);

/* ------------------------------------------------------ DBoW2 vocabulary */

typedef struct orb_vocabulary orb_vocabulary_t;

/* ScoringType / WeightingType values (Thirdparty/DBoW2/DBoW2/BowVector.h:36-53). */
#define ORB_VOC_L1_NORM 0
#define ORB_VOC_L2_NORM 1
#define ORB_VOC_CHI_SQUARE 2
#define ORB_VOC_KL 3
#define ORB_VOC_BHATTACHARYYA 4
#define ORB_VOC_DOT_PRODUCT 5
#define ORB_VOC_TF_IDF 0
#define ORB_VOC_TF 1
#define ORB_VOC_IDF 2
#define ORB_VOC_BINARY 3

/* A vocabulary tree from the node table loadFromTextFile builds
 * (TemplatedVocabulary.h:1400-1444): node 0 is the root; node i >= 1 has
 * parent[i] < i (its children are ordered by id), leaf_flag[i] (word ids go to
 * flagged nodes in id order), descriptor 32 bytes at descriptors + 32 i and
 * weight[i].  Entry 0 of each array is ignored.  k, L, scoring, weighting as in
 * the text header (validated as at :1383).  The tree is copied to the device. */
orb_status_t orb_vocabulary_create(int device, int k, int L, int scoring, int weighting,
                                   int n_nodes, const int32_t* parent, const uint8_t* leaf_flag,
                                   const uint8_t* descriptors, const double* weights,
                                   orb_vocabulary_t** out);
/* loadFromTextFile(path) (ORBvoc.txt format). */
orb_status_t orb_vocabulary_load_text(int device, const char* path, orb_vocabulary_t** out);
void orb_vocabulary_destroy(orb_vocabulary_t* v);
/* info6 = {k, L, scoring, weighting, nodes (incl. root), words}. */
orb_status_t orb_vocabulary_info(const orb_vocabulary_t* v, int32_t* info6);
void* orb_vocabulary_stream(orb_vocabulary_t* v);

/* transform(desc rows, mBowVec, mFeatVec, levelsup) for one frame of n <= 8192
 * descriptors.  BowVector (std::map<WordId, double>) as bow_words ascending +
 * bow_values; FeatureVector (std::map<NodeId, vector<unsigned>>) as CSR in
 * the orb_match_bow layout: fv_nodes ascending, fv_offs[n_fv_nodes + 1],
 * fv_feats.  Every output holds up to n entries (fv_offs n + 1).  Optional
 * per-feature feat_word (0xFFFFFFFF = stopped, weight <= 0) and feat_node. */
orb_status_t orb_vocabulary_transform(orb_vocabulary_t* v, int n, const uint8_t* desc,
                                      int levelsup, uint32_t* bow_words, double* bow_values,
                                      int32_t* n_words, uint32_t* fv_nodes, int32_t* fv_offs,
                                      uint32_t* fv_feats, int32_t* n_fv_nodes,
                                      uint32_t* feat_word, uint32_t* feat_node);
/* Device-batched form: frame f has d_counts[f] descriptors at
 * d_desc + 32 * f * stride (stride <= 8192).  Per-frame outputs at offset
 * f * stride (fv_offs: f * (stride + 1)); d_feat_* are per-feature scratch
 * (also outputs) of n_frames * stride entries.  Asynchronous on `stream`. */
orb_status_t orb_vocabulary_transform_batch(orb_vocabulary_t* v, int n_frames,
                                            const int32_t* d_counts, const uint8_t* d_desc,
                                            int stride, int levelsup, uint32_t* d_feat_word,
                                            double* d_feat_weight, uint32_t* d_feat_node,
                                            uint32_t* d_bow_words, double* d_bow_values,
                                            int32_t* d_n_words, uint32_t* d_fv_nodes,
                                            int32_t* d_fv_offs, uint32_t* d_fv_feats,
                                            int32_t* d_n_fv_nodes, void* stream);

/* ------------------------------------------- place recognition (BoW score) */

/* TemplatedVocabulary::score(v1, v2) with the vocabulary's own scoring type
 * (ScoringObject.cpp:23-311) for n_pairs pairs.  BowVectors in the layout
 * orb_vocabulary_transform emits: pair p's first vector is a_words / a_values
 * [a_offs[p], a_offs[p+1]) with the words strictly ascending, its second b_*
 * likewise; out[p] = the reference's double, bit for bit (the sum over the
 * common words is one chain of double adds in ascending word order).
 * Limits: KL_DIVERGENCE calls log(), whose rounding no build pins: a KL
 * vocabulary returns ORB_EINVAL here and from orb_kf_database_create.  Offsets
 * are int32 (fewer than 2^31 words per call).  Host buffers; synchronous. */
orb_status_t orb_vocabulary_score(orb_vocabulary_t* v, int n_pairs, const int32_t* a_offs,
                                  const uint32_t* a_words, const double* a_values,
                                  const int32_t* b_offs, const uint32_t* b_words,
                                  const double* b_values, double* out);
/* Device-pointer form.  The vectors are not validated.  Asynchronous on
 * `stream`.  An offsets array describes back-to-back vectors: pair p ends where
 * pair p + 1 begins.  orb_vocabulary_transform_batch leaves frame f at
 * [f * stride, f * stride + d_n_words[f]) with a gap behind it, so its outputs
 * are scored in place one pair per call: the caller builds, on the device, the
 * two offsets (f * stride, f * stride + d_n_words[f]) of every frame and passes
 * n_pairs = 1 with d_a_offs / d_b_offs pointing at the two entries of the
 * frames to compare (the words / values pointers stay the buffers' bases);
 * or it compacts the frames first.  Spanning the gaps with pairs of their own
 * would score uninitialised words. */
orb_status_t orb_vocabulary_score_batch(orb_vocabulary_t* v, int n_pairs, const int32_t* d_a_offs,
                                        const uint32_t* d_a_words, const double* d_a_values,
                                        const int32_t* d_b_offs, const uint32_t* d_b_words,
                                        const double* d_b_values, double* d_out, void* stream);

/* --------------------------------------- place recognition (KeyFrameDatabase) */

/* KeyFrameDatabase (src/KeyFrameDatabase.cc) over keyframe ids.  The BowVectors,
 * the add sequence, the covisibility snapshots and the per-keyframe mRelocScore /
 * mLoopScore live in device memory and grow on add; a query uploads its own
 * BowVector (and the connected ids) only.  Every call is synchronous on the
 * handle's own stream and serialised by the handle's mutex.  The vocabulary
 * must outlive the database.
 * Differences from the reference, each a status or a documented value:
 *   - mRelocScore / mLoopScore of a keyframe no query has scored yet read 0.0f
 *     (the reference leaves them uninitialised, include/KeyFrame.h); a keyframe
 *     erased and added again is a new keyframe (new sequence number, scores 0).
 *   - query ids are taken to be unique, as Frame / KeyFrame mnId are; 0 (the
 *     initialiser of mnRelocQuery / mnLoopQuery) and the id of the previous
 *     query of the same kind are refused.
 *   - storage of erased keyframes is reclaimed by orb_kf_database_clear only;
 *     at most 2^31 - 1 keyframes are added between two clears. */
typedef struct orb_kf_database orb_kf_database_t;

orb_status_t orb_kf_database_create(orb_vocabulary_t* v, orb_kf_database_t** out);
void orb_kf_database_destroy(orb_kf_database_t* db);
orb_status_t orb_kf_database_clear(orb_kf_database_t* db);   /* :72-76 */
/* Number of keyframes in the database (added and not erased); < 0 = status. */
int orb_kf_database_size(orb_kf_database_t* db);
/* add(pKF) (:42-49) with pKF->mnId = kf_id and pKF->mBowVec = words / values.
 * ORB_EINVAL if the words are not strictly ascending, a word is >= the
 * vocabulary's word count, or kf_id is present already (the reference would
 * list it twice). */
orb_status_t orb_kf_database_add(orb_kf_database_t* db, int64_t kf_id, int n_words,
                                 const uint32_t* words, const double* values);
/* erase(pKF) (:51-70); an id that is not present is a no-op, as there. */
orb_status_t orb_kf_database_erase(orb_kf_database_t* db, int64_t kf_id);
/* Snapshot of pKF->GetBestCovisibilityKeyFrames(10) (n <= 10 ids, best first),
 * read by the queries' accumulation step until replaced.  An id that is not
 * in the database at query time never shares. */
orb_status_t orb_kf_database_set_covisibility(orb_kf_database_t* db, int64_t kf_id, int n,
                                              const int64_t* neighbour_ids);
/* DetectRelocalizationCandidates(F) (:205-339; Tracking::Relocalization,
 * src/Tracking.cc:1569) with F->mnId = query_id and F->mBowVec = words / values.
 * out_ids = vpRelocCandidates in the reference's order.  On ORB_ECAPACITY
 * *n_out holds the required count (never more than orb_kf_database_size) and
 * the query has run: its scores are stored; asking again under a new query_id
 * returns the same candidates. */
orb_status_t orb_kf_database_detect_relocalization(orb_kf_database_t* db, uint64_t query_id,
                                                   int n_words, const uint32_t* words,
                                                   const double* values, int64_t* out_ids,
                                                   int capacity, int* n_out);
/* DetectLoopCandidates(pKF, minScore) (:79-202; LoopClosing::DetectLoop,
 * src/LoopClosing.cc:125-158): connected_ids = pKF->GetConnectedKeyFrames()
 * (ids not in the database are ignored). */
orb_status_t orb_kf_database_detect_loop(orb_kf_database_t* db, uint64_t query_id, int n_words,
                                         const uint32_t* words, const double* values,
                                         int n_connected, const int64_t* connected_ids,
                                         float min_score, int64_t* out_ids, int capacity,
                                         int* n_out);
/* lKFsSharingWords of the last query on this handle, in list order: ids[i],
 * common[i] = mnRelocWords / mnLoopWords, scored[i] = 1 if that query scored
 * it (common > minCommonWords), scores[i] = its mRelocScore / mLoopScore after
 * the query (for an entry not scored: what an earlier query left, or 0).
 * *n = the list's length (ORB_ECAPACITY if capacity is smaller; all outputs
 * may be NULL to ask for it).  Empty after clear. */
orb_status_t orb_kf_database_last_query(orb_kf_database_t* db, int64_t* ids, int32_t* common,
                                        float* scores, uint8_t* scored, int capacity, int* n);
/* Isolated kernel timing: runs kernel `stage` of the last query again `reps`
 * times between two events (0 k_db_common, 1 k_db_list, 2 k_db_score,
 * 3 k_db_accumulate, 4 k_db_select) and returns the total milliseconds and the
 * kernel's name.  ORB_EINVAL if the database changed since that query. */
orb_status_t orb_kf_database_profile(orb_kf_database_t* db, int stage, int reps,
                                     double* total_ms, const char** name);

/* ---------------------------------------------------------- synthetic input */

/* Deterministic synthetic grayscale images (integer-only generator, identical
 * everywhere).  view 0 = left / mono, 1 = right (shapes shifted by their
 * disparity, bf-consistent).  Frame `frame` of sequence `seed` applies the
 * cumulative ego-motion of frames 0..frame-1. */
void orb_synth_image(uint64_t seed, int frame, int view, int width, int height,
                     uint8_t* out, size_t stride);

/* Synthetic local map of n_mp points derived from one frame's keypoints
 * (SURVEY §8(d) C5 recipe).  Writes mps[n_mp], mp_desc[n_mp*32],
 * kp_locked[n_kp]. */
void orb_synth_local_map(uint64_t seed, const orb_keypoint_t* keys,
                         const uint8_t* desc, int n_kp, int n_mp, int width, int height,
                         orb_mp_track_t* mps, uint8_t* mp_desc, uint8_t* kp_locked);

/* Library / device info. */
int orb_abi_version(void);
orb_status_t orb_device_count(int* n);
const char* orb_status_string(orb_status_t s);

/* ------------------------------------------ Optimizer::OptimizeSim3 on the device */

/* Optimizer::OptimizeSim3 (src/Optimizer.cc:1130-1326) for n_problems
 * independent (pKF1, pKF2, vpMatches1, g2oS12) problems, the last stage of
 * LoopClosing::ComputeSim3: one free VertexSim3Expmap against two edges per
 * correspondence (EdgeSim3ProjectXYZ, EdgeInverseSim3ProjectXYZ), both
 * optimize() calls, both classifications and the nCorrespondences - nBad < 10
 * gate in one launch, one workgroup per problem.  Every per-problem array is a
 * device pointer; the call is asynchronous on `stream`, does not synchronise
 * with the host and uses none of the handle's scratch. */
typedef struct orb_sim3_opt_result {
  int32_t status;     /* 0; -1: malformed (below) */
  int32_t n_corr;     /* nCorrespondences */
  int32_t n_bad;      /* nBad of the first check */
  int32_t n_inliers;  /* the return value (0 on the early return) */
  double q[4];        /* g2oS12 after the call: rotation (x, y, z, w), not normalised */
  double t[3];        /*   translation */
  double s;           /*   scale */
  float R[9];         /* q.toRotationMatrix() narrowed to float, row-major */
  float t_f[3];       /* t narrowed */
  float s_f;          /* s narrowed */
  int32_t _pad;       /* written as 0 */
} orb_sim3_opt_result_t; /* 136 bytes */

/* Keyframes: the slot layout of orb_sim3_solver_setup_batch (d_kf1_slot,
 * d_kf2_slot, d_kf_keys, d_kf_nkeys, d_kf_point_index, d_kf_pose, kp_stride,
 * d_points; the same NOT-checked ranges).  d_kf1_slot / d_kf2_slot may be NULL as
 * there: problem p then uses slot p (for both keyframes if both are NULL).
 * Matches: d_match12 + p * kp_stride holds, per i < N (keyframe 1's clamped count), the global point index of
 * vpMatches1[i] (negative: NULL), d_index2 + p * kp_stride holds
 * pMP2->GetIndexInKeyFrame(pKF2): the arrays given to the solver, after
 * SearchBySim3's row has been merged into them.
 * Start: d_start[p].R, .t, .scale are g2oS12 = Sim3(toMatrix3d(R),
 * toVector3d(t), s): floats widened to double, Quaterniond(Matrix3d), no
 * normalisation.  A problem with d_start[p].has_sim3 == 0, or with
 * d_active[p] == 0 (d_active optional), is skipped: nothing of it is read or
 * written.  d_result of orb_sim3_solver_iterate_batch may be passed as it is.
 * Host values: inv_level_sigma2[n_levels] (mvInvLevelSigma2 of both keyframes;
 * 1 <= n_levels <= 16), cam1 / cam2 (fx, fy, cx, cy are read), th2 (float),
 * fix_scale.
 * Skips, in the reference's order (:1185-1220): NULL match, NULL pMP1, either
 * point bad, i2 < 0.  A kept pair whose i2 is at or above keyframe 2's clamped
 * count, or with either keypoint's octave outside [0, n_levels), makes the
 * problem malformed: d_out[p] = {status -1, counts 0, the start value}, its
 * d_match12 row is not written, and nothing is indexed with the bad value.
 * Out: d_match12 in place, -1 wherever the reference stores NULL (after the
 * first optimize(5), also when the gate then returns 0, and after the second
 * optimize); d_out[p].  On the early return the Sim3 fields hold the start
 * value (g2oS12 is not assigned there).
 * Capacity: the compacted pair records (56 bytes each) stay in LDS beside
 * 39,648 bytes of term tiles and solver state;
 * orb_optimize_sim3_max_stride() is the largest kp_stride that fits the 160
 * KiB of one CU (a pure function, callable without a device).  Above it:
 * ORB_ECAPACITY before anything is launched, nothing written (no scratch tier).
 * ORB_EINVAL: a null required pointer, n_problems < 0, kp_stride <= 0, n_levels
 * outside [1, 16].  n_problems == 0: ORB_OK, no launch.
 *
 * Pins (the same list stands in tests/sim3opt_ref.py and DESIGN.md 4.12; g2o
 * and Eigen themselves are not available to the project: unpinned against
 * their binaries).  Doubles throughout, every expression as written, no
 * contraction; the Eigen closed forms, LDLT<MatrixXd> rules (here n = 7) and
 * Levenberg-Marquardt rules are those of orb_pose_optimization.
 *  O1  P3D1c, P3D2c = Rcw * X + tcw in float (the Sim3 solver's pin P1), then
 *      widened.
 *  O2  Jacobians are numeric (base_binary_edge.hpp:131-200): column d =
 *      (1.0 / (2 * 1e-9)) * (e(+1e-9 e_d) - e(-1e-9 e_d)), each through
 *      oplusImpl: Sim3(update) * estimate.  _error is restored afterwards.
 *  O3  constructQuadraticForm of a binary edge whose `to` vertex alone is
 *      free (:91-113): omega_r = -(Omega e), omega_r *= rho[1], b += B^T omega_r
 *      ((B_0q r_0) + (B_1q r_1)), A += (B^T (rho[1] Omega)) B ((B_0q w) B_0p +
 *      (B_1q w) B_1p, w = rho[1] * invSigma2), the zero off-diagonal terms of
 *      the diagonal Omega dropped; the lower triangle is accumulated.
 *  O4  The active edges add in insertion order e12(i), e21(i), e12(i'),
 *      e21(i'), ... over ascending i; a removed pair adds +0.0.
 *  O5  An edge is classified from the error of the last trial, rejected or
 *      not; chi2() > th2 compares the double chi2 with the float th2 widened;
 *      deltaHuber is the float sqrt(th2) widened; Huber's inlier test is <=.
 *  O6  oplusImpl with fix_scale writes update[6] = 0 into the caller's array:
 *      column 6 is the difference of two equal evaluations, and the solver's
 *      x[6] is zeroed before computeScale reads it.
 *  O7  Sim3(Vector7d) (sim3.h:70-142): branches |sigma| < 1e-5 x theta < 1e-5,
 *      R = (I + Omega) + Omega^2 or (I + (sin / theta) Omega) + ((1 - cos) /
 *      (theta theta)) Omega^2, A, B, C as written, W = ((A Omega) + (B Omega^2))
 *      + (C I), t = W upsilon; Quaterniond(R) is never normalised, nor are
 *      operator*, map or inverse(); inverse() = (r.conjugate(),
 *      r.conjugate() * ((-1. / s) * t), 1. / s); project is two divisions by z.
 *  O8  The second optimize starts at iteration 0: lambda from the 7 diagonals,
 *      ni = 2; the solver's x is kept across both.
 *  O9  exp = pinned_exp (fdlibm e_exp.c from IEEE operations alone); sin and
 *      cos = pinned_sincos_d; sqrt and / are IEEE. */
orb_status_t orb_optimize_sim3_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
    const orb_keypoint_t* d_kf_keys, const int32_t* d_kf_nkeys, const int32_t* d_kf_point_index,
    const orb_pose_t* d_kf_pose, int kp_stride, const orb_map_point_t* d_points,
    int32_t* d_match12, const int32_t* d_index2, const orb_sim3_result_t* d_start,
    const uint8_t* d_active, const float* inv_level_sigma2, int n_levels,
    const orb_camera_t* cam1, const orb_camera_t* cam2, float th2, int fix_scale,
    orb_sim3_opt_result_t* d_out, void* stream);
int orb_optimize_sim3_max_stride(void);

/* One problem with host pointers (synchronises): keys1[n1] / keys2[n2]
 * (mvKeysUn), point_index1[n1] (GetMapPointMatches() of pKF1), pose1 / pose2,
 * points[n_points], match12[n1] (in/out) and index2[n1], start (R, t, scale are
 * read; has_sim3 is ignored), out.  Every non-negative point index must be
 * below n_points (ORB_EINVAL).  Otherwise as the batch of one. */
orb_status_t orb_optimize_sim3(
    orb_matcher_t* m, const orb_keypoint_t* keys1, int n1, const int32_t* point_index1,
    const orb_pose_t* pose1, const orb_keypoint_t* keys2, int n2, const orb_pose_t* pose2,
    const orb_map_point_t* points, int n_points, int32_t* match12, const int32_t* index2,
    const orb_sim3_result_t* start, const float* inv_level_sigma2, int n_levels,
    const orb_camera_t* cam1, const orb_camera_t* cam2, float th2, int fix_scale,
    orb_sim3_opt_result_t* out);

/* pinned_exp (pin O9) over n device doubles, for tests of the pin: d_y[i] =
 * pinned_exp(d_x[i]).  Asynchronous on `stream`. */
orb_status_t orb_pinned_exp_batch(orb_matcher_t* m, int n, const double* d_x, double* d_y,
                                  void* stream);

/* ------------- LoopClosing::ComputeSim3's two matchers as device batches
 * (src/LoopClosing.cc:251-428).  With orb_sim3_solver_*_batch and
 * orb_optimize_sim3_batch they make a round over all loop candidates one chain
 * on one stream: orb_match_bow_kf_batch -> setup -> { iterate ->
 * orb_search_by_sim3_batch -> orb_optimize_sim3_batch }, with no host copy in
 * between.  Both calls: every per-problem array a device pointer, asynchronous
 * on `stream`, no host synchronisation, upload or download, one workgroup per
 * problem, all state in LDS and the caller's arrays (none of the handle's
 * scratch: `stream` alone orders the call).  n_problems == 0: ORB_OK, no
 * launch.  A kp_stride above the call's *_max_stride(): ORB_ECAPACITY before
 * anything is launched, nothing written.
 *
 * Device-batched SearchByBoW(pKF1, pKF2, vpMatches12) (src/ORBmatcher.cc:
 * 581-716).  Slots: one family in orb_match_bow_batch's keyframe layout (keys,
 * point_index, fv_nodes and fv_feats at k * kp_stride, descriptors at
 * 32 * k * kp_stride, fv_offs at k * (kp_stride + 1), the counts nkeys[k] and
 * n_fv_nodes[k]; of the keys only `angle` is read).  Problem p matches slot
 * d_kf1_slot[p] against slot d_kf2_slot[p] (either NULL: slot p; a slot may
 * serve many problems, the current keyframe serves all of them).
 * d_kf_point_index[i] >= 0 names mvpMapPoints[i] in d_points, one array shared
 * by all problems, of which only `bad` is read (d_points NULL: no point is
 * bad); any negative value is NULL.
 * Per problem the reference loop: only common nodes; the KF1 keypoints of a
 * node in list order, each with a non-NULL, non-bad point; KF2 candidates with
 * a non-NULL, non-bad point that are not yet in vbMatched2; best and second
 * best by strict <; accepted iff bestDist1 < 50 and (float)bestDist1 <
 * nnratio * (float)bestDist2; vbMatched2 set at acceptance and never cleared;
 * the rotation histogram over angle1 - angle2 with ComputeThreeMaxima.
 * Out: d_match12 + p * kp_stride over KF1's clamped count: the global point
 * index of the matched KF2 keypoint's point or -1; d_index2 + p * kp_stride:
 * that keypoint's index (bestIdx2) or -1; entries removed by the filter are -1
 * in both rows; entries past the count are not written.  The two rows are
 * orb_sim3_solver_setup_batch's d_match12 and d_index2 as they stand.
 * d_info[p]: orb_bow_match_info_t (n_tried counts KF1 keypoints).
 * min_matches (ComputeSim3: 20; 0: no gate): a problem with fewer matches
 * keeps its counts, gets enough = 0 and both rows -1; the solver's setup then
 * finds N = 0 and iterate returns no_more at once.
 * Malformed slots as in orb_match_bow_batch (counts and node counts clamped;
 * decreasing or oversized offsets or a feature index >= the count in either
 * FeatureVector): n_matches = -1, the other fields 0, both rows -1 over KF1's
 * clamped count, nothing indexed with the bad value.  Ascending node ids are
 * the caller's promise.
 * Per problem the rows equal orb_match_bow_kf's output on the same inputs,
 * mapped through point_index.
 * Capacity: 8 * ((kp_stride + 3) & ~3) + 512 bytes (the claim word per KF2
 * keypoint, the partner node per KF1 node) must fit the 160 KiB of one CU;
 * orb_match_bow_kf_batch_max_stride() is the largest such kp_stride (a pure
 * function, callable without a device).
 * ORB_EINVAL: a null required pointer, n_problems < 0, kp_stride <= 0, nnratio
 * not finite. */
orb_status_t orb_match_bow_kf_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
    const orb_keypoint_t* d_kf_keys, const uint8_t* d_kf_desc, const int32_t* d_kf_nkeys,
    const int32_t* d_kf_point_index, const uint32_t* d_kf_fv_nodes, const int32_t* d_kf_fv_offs,
    const uint32_t* d_kf_fv_feats, const int32_t* d_kf_n_fv_nodes, int kp_stride,
    const orb_map_point_t* d_points, float nnratio, int check_orientation, int min_matches,
    int32_t* d_match12, int32_t* d_index2, orb_bow_match_info_t* d_info, void* stream);
int orb_match_bow_kf_batch_max_stride(void);

/* Device-batched SearchBySim3 (src/ORBmatcher.cc:1212-1458) with the inlier
 * filter of src/LoopClosing.cc:338-343 in front of it.
 * Slots: those of orb_sim3_solver_setup_batch (d_kf1_slot, d_kf2_slot,
 * d_kf_keys, d_kf_nkeys, d_kf_point_index, d_kf_pose of which rcw and tcw are
 * read, kp_stride, d_points) plus d_kf_desc (32 bytes per keypoint slot) and
 * d_mp_desc (32 bytes per entry of d_points, GetDescriptor()).
 * Per problem: the rows d_match12 / d_index2 + p * kp_stride (in/out: the
 * arrays given to the solver), d_inliers12 + p * kp_stride (optional, the
 * solver's vbInliers), d_sim3[p] (R, t, scale and has_sim3 are read; the
 * solver's d_result may be passed as it is), d_active[p] (optional).  A problem
 * with has_sim3 == 0 or d_active[p] == 0 is skipped: nothing of it is read or
 * written.
 * Host values: one `cam` (the reference projects with pKF1's fx, fy, cx, cy in
 * both directions), the bounds min_x, max_x, min_y, max_y of
 * KeyFrame::IsInImage (half-open; max > min), n_levels in [1, 16],
 * scale_factors[n_levels], log_scale_factor, th (ComputeSim3: 7.5).
 * Per problem, in this order:
 *  1 with d_inliers12, every i1 below KF1's clamped count with inliers[i1] == 0
 *    gets match12[i1] = index2[i1] = -1;
 *  2 already1[i1] = match12[i1] >= 0; already2[index2[i1]] = 1 for those
 *    entries with 0 <= index2[i1] < N2 (an index outside is ignored, as in the
 *    reference: not malformed);
 *  3 sR12 = (float)((double)s * (double)R[r][c]), sR21 = (float)((1.0 /
 *    (double)s) * (double)R[c][r]), t21[r] = -((sR21[r][0] t0 + sR21[r][1] t1) +
 *    sR21[r][2] t2) in float, as orb_search_by_sim3 computes them on the host;
 *  4 the 64 x 48 grids of both keyframes, keypoints in ascending index inside a
 *    cell, a keypoint outside the bounds in no cell;
 *  5 KF1's points (non-NULL, not already matched, not bad) through R1w, t1w,
 *    sR21, t21 into KF2: depth < 0 rejected, the projection inside the
 *    half-open bounds, cv::norm in double, the range 0.8f * min_distance ..
 *    1.2f * max_distance, the level from PredictScale with the unscaled
 *    max_distance (clamped to [0, n_levels - 1]), radius = th * scale[level],
 *    GetFeaturesInArea's order, octaves in [level - 1, level], the first
 *    minimum Hamming distance, accepted iff <= 100;
 *  6 the same from KF2 through R2w, t2w, sR12, t12 into KF1;
 *  7 i1 with vnMatch1[i1] = idx2 >= 0 and vnMatch2[idx2] == i1 gets
 *    match12[i1] = point_index2[idx2] and index2[i1] = idx2.
 * Out: the two rows in place (orb_optimize_sim3_batch's d_match12 / d_index2
 * as they stand); d_new12 + p * kp_stride (optional) over KF1's clamped count:
 * idx2 where this call added a match, else -1 (orb_search_by_sim3's match12 on
 * the same inputs); d_info[p] as below, exact and deterministic.
 * Octaves are only compared and the predicted level is clamped: no octave makes
 * a problem malformed.  Counts are clamped to [0, kp_stride].  The caller keeps
 * every non-negative point index inside d_points and d_mp_desc and every slot
 * number inside the slot arrays (NOT checked, as in the solver).
 * Capacity: two cell-start tables of 3,076 ints and 16 bytes per keypoint slot
 * (two cell-ordered index lists, vnMatch1, vnMatch2): 24,608 + 16 *
 * ((kp_stride + 3) & ~3) + 1,024 bytes must fit the 160 KiB of one CU;
 * orb_search_by_sim3_batch_max_stride() is the largest such kp_stride (a pure
 * function, callable without a device; above orb_optimize_sim3_max_stride()).
 * ORB_EINVAL: a null required pointer, n_problems < 0, kp_stride <= 0, n_levels
 * outside [1, 16], bounds with max <= min. */
typedef struct orb_sim3_search_info {
  int32_t n_found;  /* the return value: matches added by this call */
  int32_t n_kept;   /* non-NULL entries of the row after the inlier filter */
  int32_t n_total;  /* n_kept + n_found (nTotalMatches before OptimizeSim3) */
  int32_t n_best12; /* entries of vnMatch1 that are >= 0 */
  int32_t n_best21; /* entries of vnMatch2 that are >= 0 */
} orb_sim3_search_info_t; /* 20 bytes */
orb_status_t orb_search_by_sim3_batch(
    orb_matcher_t* m, int n_problems, const int32_t* d_kf1_slot, const int32_t* d_kf2_slot,
    const orb_keypoint_t* d_kf_keys, const uint8_t* d_kf_desc, const int32_t* d_kf_nkeys,
    const int32_t* d_kf_point_index, const orb_pose_t* d_kf_pose, int kp_stride,
    const orb_map_point_t* d_points, const uint8_t* d_mp_desc, int32_t* d_match12,
    int32_t* d_index2, const uint8_t* d_inliers12, const orb_sim3_result_t* d_sim3,
    const uint8_t* d_active, const orb_camera_t* cam, float min_x, float max_x, float min_y,
    float max_y, int n_levels, const float* scale_factors, float log_scale_factor, float th,
    int32_t* d_new12, orb_sim3_search_info_t* d_info, void* stream);
int orb_search_by_sim3_batch_max_stride(void);

#ifdef __cplusplus
}
#endif
#endif /* ORB_ABI_H */
