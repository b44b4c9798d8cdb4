// orb_kernels.h -- the host launchers of the gfx950 kernels (orb_k_*), declared
// once: the runtime files call them through this header and every .hip file
// that defines launchers includes it, so a definition that drifts from its
// prototype is a compile error (they are extern "C": it would still link).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/orb_abi.h"
#include "orb_kernel_params.h"
#include "orb_plan.h"

extern "C" {
// ---------------------------------------------------- extractor_kernels.hip
hipError_t orb_k_copy_pinned(void* dst, const void* src, size_t bytes, hipStream_t s);
hipError_t orb_k_copy_to_pinned(void* dst, const void* src, size_t bytes, hipStream_t s);
hipError_t orb_k_upload_constants(hipStream_t s);
hipError_t orb_k_upload_umax(const int* umax16, hipStream_t s);
hipError_t orb_k_pyr_resize(const uint8_t* src, long long srcImgPitch, int srcStride, int sw,
                            int sh, uint8_t* dst, long long dstImgPitch, int dstStride, int dw,
                            int dh, const int* xofs, const void* alpha, const int* yofs,
                            const void* beta, int mode, int nimg, hipStream_t s);
hipError_t orb_k_pyr_resize2(const uint8_t* src, long long srcImgPitch, int srcStride, int w0,
                             int h0, uint8_t* mid, long long midImgPitch, int midStride, int w1,
                             int h1, const int* xo1, const void* al1, const int* yo1,
                             const void* be1, uint8_t* dst, long long dstImgPitch, int dstStride,
                             int w2, int h2, const int* xo2, const void* al2, const int* yo2,
                             const void* be2, int nimg, hipStream_t s);
int orb_k_pyr_resize2_fits(int w0, int h0, int w1, int h1, const int* xo1, const int* yo1, int w2,
                           int h2, const int* xo2, const int* yo2);
size_t orb_k_fast_band_lds(int bandElems);
hipError_t orb_k_fast_band(const uint8_t* img0, long long img0Pitch, int img0Stride,
                           const uint8_t* arena, long long arenaPitch, const OrbPlanDesc* plan,
                           const OrbBandDesc* bands, int nbands, const OrbCellDesc* cells,
                           uint32_t* cellKeys, int32_t* cellCount, int32_t* errFlag, int nimg,
                           hipStream_t s);
bool orb_k_fast_cells_fits(const OrbPlanDesc* plan);
size_t orb_k_fast_cells_lds(int maxRows, int maxCols);
hipError_t orb_k_fast_cells(const uint8_t* img0, long long img0Pitch, int img0Stride,
                            const uint8_t* arena, long long arenaPitch, const OrbPlanDesc* plan,
                            const OrbCellDesc* cells, const OrbCellClass* classes,
                            uint32_t* cellKeys, int32_t* cellCount,
                            int32_t* errFlag, int cellBeg, int cellEnd, int nimg, hipStream_t s);
size_t orb_k_octree_lds(int nodeCapMax, int maxCellsPerLevel, int ldsKeyCap);
size_t orb_k_octree_node_bytes(int nodeCapMax, int maxCellsPerLevel);
hipError_t orb_k_octree(const OrbPlanDesc* plan, const int32_t* cellCount,
                        const uint32_t* cellKeys, uint32_t* gKeys, uint16_t* gNid, int ldsKeyCap,
                        int nodeCapMax, int maxCellsPerLevel, uint32_t* outKeys,
                        int32_t* outCount, int32_t* errFlag, int levelBeg, int levelEnd, int nimg,
                        uint8_t* gNodes, long long nodeStride, hipStream_t s);
hipError_t orb_k_blur_levels(const uint8_t* img0, long long img0Pitch, int img0Stride,
                             const uint8_t* arena, long long arenaPitch, const OrbPlanDesc* plan,
                             const OrbTileDesc* tiles, uint8_t* blur, long long blurPitch,
                             int nimg, hipStream_t s);
hipError_t orb_k_orient_desc(const uint8_t* img0, long long img0Pitch, int img0Stride,
                             const uint8_t* arena, long long arenaPitch, const OrbPlanDesc* plan,
                             const uint32_t* outKeys, const int32_t* outCount,
                             const int32_t* errFlag, orb_keypoint_t* kps, uint8_t* desc,
                             int capacity, int32_t* counts, int nimg, int levelBeg,
                             int levelEnd, hipStream_t s);

// ------------------------------------------------------ matcher_kernels.hip
hipError_t orb_k_hamming(const uint8_t* a, const uint8_t* b, int n, int32_t* out, hipStream_t s);
hipError_t orb_k_grid_build(const orb_keypoint_t* keys, const int32_t* nkeys, int kpStride,
                            float minX, float minY, float invW, float invH, int32_t* cellStart,
                            int32_t* cellIdx, int nproblems, hipStream_t s);
hipError_t orb_k_grid_build_staged(const orb_keypoint_t* keys, const int32_t* nkeys,
                                   const uint8_t* locked, const float* uright, int kpStride,
                                   float minX, float minY, float invW, float invH,
                                   int32_t* cellStart, int32_t* cellIdx, void* staged,
                                   int nproblems, hipStream_t s);
int orb_k_grid_stage_max(void);
hipError_t orb_k_proj_candidates(const orb_keypoint_t* keys, const uint8_t* desc,
                                 const float* uright, const uint8_t* locked, int kpStride,
                                 const int32_t* nkeys, const orb_mp_track_t* mps,
                                 const uint8_t* mpDesc, const int32_t* nmps, int mpStride,
                                 int mpMax, const int32_t* cellStart, const int32_t* cellIdx,
                                 const void* stagedGrid, const ProjParams* params, uint32_t* topk,
                                 int32_t* ncand, int nproblems, hipStream_t s);
int orb_k_proj_resolve_kernel(int nproblems, int kpStride, int mpStride, int schedule);
size_t orb_k_proj_jacobi_bytes(int kpStride, int mpStride, int nproblems, int schedule);
hipError_t orb_k_proj_resolve(const orb_keypoint_t* keys, const uint8_t* desc,
                              const float* uright, const uint8_t* locked, const int32_t* nkeys,
                              int kpStride, const orb_mp_track_t* mps, const uint8_t* mpDesc,
                              const int32_t* nmps, int mpStride, const int32_t* cellStart,
                              const int32_t* cellIdx, const ProjParams* params,
                              const uint32_t* topk, const int32_t* ncand, int32_t* kpMatch,
                              int32_t* nmatches, int nproblems, int schedule, int jacobiRounds,
                              int32_t* jacScratch, hipStream_t s);
size_t orb_k_proj_ovf_bytes(int nproblems);
void orb_k_stereo_scratch(const StereoParams* params, int kpStride, size_t* startInts,
                          size_t* idxInts);
hipError_t orb_k_stereo(const orb_keypoint_t* lkeys, const uint8_t* ldesc, const int32_t* nleft,
                        const orb_keypoint_t* rkeys, const uint8_t* rdesc, const int32_t* nright,
                        int kpStride, int maxLeft, const StereoPairLevels* pyr,
                        const StereoParams* params, float* uRight, float* depth, int32_t* sad,
                        int npairs, int32_t* rowStart, int32_t* rowIdx, hipStream_t s);
// Capacity rule of the one-block resolve kernels (k_frame_resolve,
// k_pp_resolve): dynamic LDS + the kernel's static hist[32] must fit one CU.
// orb_k_*_resolve_lds return that total; a call fits iff it is <= ORB_LDS_PER_CU.
#define ORB_LDS_PER_CU ((size_t)160 * 1024)
#define ORB_RESOLVE_STATIC_LDS ((size_t)128)
size_t orb_k_frame_resolve_lds(int nkeys, int nlast);
hipError_t orb_k_frame_proj(const orb_keypoint_t* keys, const uint8_t* desc, const float* uright,
                            const uint8_t* locked, int nkeys, const orb_last_mp_t* last,
                            const uint8_t* lastDesc, int nlast, const int32_t* cellStart,
                            const int32_t* cellIdx, const FrameProjParams* params, uint32_t* topk,
                            int32_t* ncand, int32_t* kpMatch, int32_t* nmatches, hipStream_t s);
hipError_t orb_k_bow(const uint8_t* kfDesc, const float* kfAngle, const int32_t* kfMp,
                     const uint8_t* kfBad, int kfNodes, const uint32_t* kfNodeIds,
                     const int32_t* kfOffs, const uint32_t* kfFeats, int nKfFeats,
                     const uint8_t* fDesc, const float* fAngle, int fNodes,
                     const uint32_t* fNodeIds, const int32_t* fOffs, const uint32_t* fFeats,
                     int nF, const int32_t* fMp, const uint8_t* fBad, int thLow,
                     float nnratio, int checkOri, int32_t* fMatch, int32_t* accF,
                     int32_t* nmatches, hipStream_t s);
hipError_t orb_k_frustum(const orb_map_point_t* mps, const int32_t* nmps, int mpStride,
                         int mpMax, const orb_pose_t* poses, const FrustumParams* params,
                         orb_mp_track_t* tracks, int32_t* nInView, int nproblems, hipStream_t s);

// --------------------------------------------------- projection_kernels.hip
size_t orb_k_pp_resolve_lds(int nkeys, int n);
hipError_t orb_k_pp_match(int mode, const orb_map_point_t* mps, const uint8_t* mpValid,
                          const uint8_t* mpSkip, const uint8_t* mpDesc, int n,
                          const orb_keypoint_t* keys, const uint8_t* desc, const float* uright,
                          const int32_t* cellStart, const int32_t* cellIdx,
                          const PPParams* params, PPRec* recs, int32_t* best, uint32_t* topk,
                          int32_t* ncand, hipStream_t s);
hipError_t orb_k_pp_resolve(const orb_keypoint_t* keys, const uint8_t* desc, int nkeys,
                            const uint8_t* kpLocked, const uint8_t* mpDesc, const float* mpAngle,
                            int n, const int32_t* cellStart, const int32_t* cellIdx,
                            const PPParams* params, const PPRec* recs, const uint32_t* topk,
                            const int32_t* ncand, int32_t* kpMatch, int32_t* nmatches,
                            hipStream_t s);
hipError_t orb_k_sim3_mutual(const int32_t* m1, int n1, const int32_t* m2, int32_t* match12,
                             int32_t* nfound, hipStream_t s);
hipError_t orb_k_triangulation(const orb_keypoint_t* k1, const uint8_t* d1, const float* ur1,
                               const uint8_t* hasMp1, int nodes1, const uint32_t* ids1,
                               const int32_t* offs1, const uint32_t* feats1, int nFeats1,
                               const orb_keypoint_t* k2, const uint8_t* d2, const float* ur2,
                               const uint8_t* hasMp2, int nodes2, const uint32_t* ids2,
                               const int32_t* offs2, const uint32_t* feats2,
                               const TriParams* params, int32_t* match12, int32_t* acc,
                               int32_t* nmatches, hipStream_t s);

// ------------------------------------------------------ mapping_kernels.hip
size_t orb_k_init_list_len(void);
size_t orb_k_init_topk(void);
size_t orb_k_init_stage(void);
int orb_k_init_max_stride(void);
size_t orb_k_init_lds(int kpStride);
hipError_t orb_k_search_init(const orb_keypoint_t* keys1, const uint8_t* desc1, const int32_t* n1,
                             const orb_keypoint_t* keys2, const uint8_t* desc2, const int32_t* n2,
                             int kpStride, float* prev, const int32_t* cellStart,
                             const int32_t* cellIdx, const InitParams* params, int32_t* qList,
                             int32_t* qOrder, int32_t* nQ, InitKey* stage, int32_t* nStage,
                             uint32_t* topk, uint32_t* list, int32_t* ncand, int32_t* m12,
                             int32_t* nmatches, int nproblems, hipStream_t s);
hipError_t orb_k_distinctive(const int32_t* offs, const uint8_t* desc, int nmp, int32_t* best,
                             uint8_t* out, hipStream_t s);

// -------------------------------------------------------- vocab_kernels.hip
hipError_t orb_k_voc_descend(const VocNodeInfo* info, const void* ndesc, const uint32_t* nword,
                             const double* nweight, const uint32_t* norig, int nidLevel,
                             const uint8_t* desc, const int32_t* counts, int nSingle, int stride,
                             int nFrames, uint32_t* fword, double* fweight, uint32_t* fnode,
                             hipStream_t s);
int orb_k_voc_max_features(void);
hipError_t orb_k_voc_vectors(const uint32_t* fword, const double* fweight, const uint32_t* fnode,
                             const int32_t* counts, int nSingle, int stride, int tf, int must,
                             int l2, int nFrames, uint32_t* bowWords, double* bowValues,
                             int32_t* nWords, uint32_t* fvNodes, int32_t* fvOffs,
                             uint32_t* fvFeats, int32_t* nFv, hipStream_t s);

// ----------------------------------------------------- placerec_kernels.hip
hipError_t orb_k_bow_score(int type, int nPairs, const int32_t* aOffs, const uint32_t* aWords,
                           const double* aValues, const int32_t* bOffs, const uint32_t* bWords,
                           const double* bValues, double* out, hipStream_t s);
size_t orb_k_db_key_scratch(int nSlots);
hipError_t orb_k_db_query(const PrQueryArgs* args, hipStream_t s);

// ------------------------------------------------------- camera_kernels.hip
hipError_t orb_k_undistort_points(const UndistortParams* params, int n, const float* in,
                                  float* out, hipStream_t s);
hipError_t orb_k_undistort_keys(const UndistortParams* params, int nFrames,
                                const int32_t* counts, int nSingle, int stride, const void* in,
                                void* out, int copyOnly, hipStream_t s);

// -------------------------------------------------------- depth_kernels.hip
hipError_t orb_k_stereo_from_rgbd(const RgbdParams* params, const int32_t* counts, int nSingle,
                                  const orb_keypoint_t* keys, const orb_keypoint_t* keysUn,
                                  const void* depth, float* uRight, float* depthOut,
                                  hipStream_t s);
hipError_t orb_k_unproject_stereo(const UnprojectParams* params, const int32_t* counts,
                                  int nSingle, const orb_keypoint_t* keysUn, const float* depth,
                                  const orb_pose_t* poses, float* x3d, uint8_t* valid,
                                  hipStream_t s);
// bytes of global key scratch a call needs (0: the keys sort in LDS)
size_t orb_k_close_points_scratch(int nFrames, int stride);
hipError_t orb_k_close_points(int nFrames, const int32_t* counts, int nSingle, int stride,
                              const float* depth, const uint8_t* mpState, const uint8_t* outlier,
                              float thDepth, int32_t* order, uint8_t* create,
                              orb_close_counts_t* out, void* scratch, hipStream_t s);
// --------------------------------------------------------- pose_kernels.hip
// bytes of global edge-record scratch a call needs (0: the records stay in LDS)
size_t orb_k_pose_optimization_scratch(int nProblems, int stride);
hipError_t orb_k_pose_optimization(const PoseOptParams* params, const int32_t* counts,
                                   const orb_keypoint_t* keysUn, const float* uRight,
                                   const int32_t* pointIndex, const void* points,
                                   const orb_pose_t* poseIn, orb_pose_t* poseOut,
                                   uint8_t* outlier, orb_pose_opt_info_t* info, void* scratch,
                                   hipStream_t s);
// -------------------------------------------------------- track_kernels.hip
// largest keypoint-slot count (kp_stride) whose replay state fits one CU's LDS
int orb_k_frame_batch_max_stride(void);
hipError_t orb_k_frame_batch(const FrameBatchParams* params, const orb_keypoint_t* keys,
                             const uint8_t* desc, const float* uright, const uint8_t* locked,
                             const int32_t* nkeys, const orb_pose_t* poseCur,
                             const orb_pose_t* poseLast, const orb_keypoint_t* lastKeys,
                             const int32_t* lastNkeys, const int32_t* lastPointIndex,
                             const uint8_t* lastOutlier, const orb_map_point_t* points,
                             const uint8_t* mpDesc, const int32_t* cellStart,
                             const int32_t* cellIdx, int32_t* kpMatch,
                             orb_frame_match_info_t* info, hipStream_t s);
hipError_t orb_k_track_discard(int nProblems, int stride, long long mpStride, int markSeen,
                               const int32_t* nkeys, int32_t* kpMatch, uint8_t* outlier,
                               orb_map_point_t* points, const int32_t* nMatches, int nMatchesStride,
                               orb_track_discard_info_t* out, hipStream_t s);
// largest kp_stride whose per-problem state fits one CU's LDS
int orb_k_bow_batch_max_stride(void);
hipError_t orb_k_bow_batch(const BowBatchParams* params, int32_t* kpMatch,
                           orb_bow_match_info_t* info, hipStream_t s);
// SearchForTriangulation over keyframe slot pairs; largest kp_stride as above
int orb_k_tri_batch_max_stride(void);
hipError_t orb_k_tri_batch(const TriBatchParams* params, int32_t* match12,
                           orb_tri_match_info_t* info, hipStream_t s);
hipError_t orb_k_track_local_merge(int nProblems, int stride, int mpStride, const int32_t* nkeys,
                                   const int32_t* kmLocal, const int32_t* localIndex,
                                   int32_t* kpMatch, hipStream_t s);
hipError_t orb_k_track_local_finish(int nProblems, int stride, long long ptStride,
                                    int onlyTracking, int nullOutliers, const int32_t* nkeys,
                                    int32_t* kpMatch, const uint8_t* outlier,
                                    const orb_map_point_t* points, int32_t* nInliers,
                                    hipStream_t s);
// ----------------------------------------------------- localmap_kernels.hip
// largest keyframe-slot count (kf_stride >= n_kf) whose per-problem state fits one CU's LDS
int orb_k_local_map_max_keyframes(void);
// distinct point ids the LDS table takes before a problem runs on the scratch table
int orb_k_local_map_hash_cap(void);
hipError_t orb_k_local_map(const LocalMapParams* params, hipStream_t s);
// --------------------------------------------------------- sim3_kernels.hip
// largest kp_stride whose staged correspondences and inlier rows fit one CU's LDS
int orb_k_sim3_max_stride(void);
hipError_t orb_k_sim3_setup(const Sim3SetupParams* params, hipStream_t s);
hipError_t orb_k_sim3_iterate(const Sim3IterParams* params, hipStream_t s);
// ----------------------------------------------------- sim3opt_kernels.hip
// largest kp_stride whose pair records fit one CU's LDS beside the term tiles
int orb_k_sim3opt_max_stride(void);
hipError_t orb_k_optimize_sim3(const Sim3OptParams* params, hipStream_t s);
hipError_t orb_k_pinned_exp(int n, const double* x, double* y, hipStream_t s);
// ---------------------------------------------------- newpoints_kernels.hip
// largest kp_stride whose staged depth keys / statuses and points fit one CU's LDS
int orb_k_median_depth_max_stride(void);
int orb_k_new_points_max_stride(void);
hipError_t orb_k_median_depth(const MedianDepthParams* params, hipStream_t s);
hipError_t orb_k_new_points(const NewPointsParams* params, hipStream_t s);
// ---------------------------------------------------- sim3chain_kernels.hip
// SearchByBoW(KF, KF) and SearchBySim3 over keyframe slot pairs; largest
// kp_stride whose per-problem state fits one CU's LDS
int orb_k_bow_kf_batch_max_stride(void);
hipError_t orb_k_bow_kf_batch(const BowKfBatchParams* params, int32_t* match12, int32_t* index2,
                              orb_bow_match_info_t* info, hipStream_t s);
int orb_k_sim3_search_max_stride(void);
hipError_t orb_k_sim3_search(const Sim3SearchParams* params, hipStream_t s);
}
