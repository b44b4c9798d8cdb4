"""MI355X-native ORB front-end: Python host mirror of the reference interface.

Mirrors, over the C ABI in ``include/orb_abi.h`` (library ``lib/liborb_amd.so``):

* ``ORBextractor``  -- ORB_SLAM2::ORBextractor (reference include/ORBextractor.h:45-114):
  same constructor arguments, ``__call__(image, mask)`` = ``operator()``
  (src/ORBextractor.cc:1091-1169), the ``Get*`` scale accessors and
  ``mvImagePyramid``.
* ``ORBmatcher``    -- ORB_SLAM2::ORBmatcher (include/ORBmatcher.h:37-102):
  ``DescriptorDistance`` and ``SearchByProjection(Frame, local map, th)``
  (src/ORBmatcher.cc:47-133).

Every result is computed by the gfx950 HIP kernels; there is no CPU path.  If
the library is missing or no gfx950 device is visible the calls raise.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
# ORB_AMD_LIB selects another build of the same library (A/B kernel experiments)
LIB_PATH = Path(os.environ.get("ORB_AMD_LIB", PKG_DIR / "lib" / "liborb_amd.so"))

ORB_OK, ORB_EEMPTY, ORB_EINVAL, ORB_ENOMEM, ORB_EDEVICE, ORB_ECAPACITY, ORB_ENODEV = 0, 1, -1, -2, -3, -4, -5

KEYPOINT_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
     ("octave", "<i4"), ("class_id", "<i4")]
)
MP_TRACK_DTYPE = np.dtype(
    [("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("view_cos", "<f4"),
     ("level", "<i4"), ("in_view", "u1"), ("bad", "u1"), ("has_obs", "u1"), ("_pad", "u1")]
)
LAST_MP_DTYPE = np.dtype([("xc", "<f4"), ("yc", "<f4"), ("invzc", "<f4"), ("last_octave", "<i4"),
                          ("last_angle", "<f4"), ("valid", "u1"), ("has_obs", "u1"),
                          ("_pad", "u1", 2), ("mp_id", "<i4")])
assert KEYPOINT_DTYPE.itemsize == 28 and MP_TRACK_DTYPE.itemsize == 24
assert LAST_MP_DTYPE.itemsize == 28


MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"),
                            ("max_distance", "<f4"), ("bad", "u1"), ("seen", "u1"),
                            ("has_obs", "u1"), ("_pad", "u1")])
POSE_DTYPE = np.dtype([("rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("ow", "<f4", (3,))])
CLOSE_COUNTS_DTYPE = np.dtype([("n_sorted", "<i4"), ("n_visit", "<i4"),
                               ("n_tracked_close", "<i4"), ("n_non_tracked_close", "<i4")])
POSE_OPT_INFO_DTYPE = np.dtype([("n_inliers", "<i4"), ("n_edges", "<i4"),
                                ("lm_iterations", "<i4"), ("rejected_trials", "<i4")])
FRAME_MATCH_INFO_DTYPE = np.dtype([("n_matches", "<i4"), ("n_matches_first_pass", "<i4"),
                                   ("retried", "<i4"), ("forward", "<i4"), ("backward", "<i4")])
TRACK_DISCARD_INFO_DTYPE = np.dtype([("n_matches", "<i4"), ("n_matches_map", "<i4"),
                                     ("n_discarded", "<i4")])
BOW_MATCH_INFO_DTYPE = np.dtype([("n_matches", "<i4"), ("n_accepted", "<i4"),
                                 ("n_common_nodes", "<i4"), ("n_tried", "<i4"), ("enough", "<i4")])
LOCAL_MAP_INFO_DTYPE = np.dtype([("n_local_kf", "<i4"), ("n_voted", "<i4"), ("n_added", "<i4"),
                                 ("ref_kf", "<i4"), ("max_votes", "<i4"),
                                 ("n_local_points", "<i4"), ("n_nulled", "<i4"), ("kept", "<i4")])
assert LOCAL_MAP_INFO_DTYPE.itemsize == 32
SIM3_CORR_DTYPE = np.dtype([("index1", "<i4"), ("x1", "<f4", (3,)), ("x2", "<f4", (3,)),
                            ("p1", "<f4", (2,)), ("p2", "<f4", (2,)), ("max_err1", "<f4"),
                            ("max_err2", "<f4"), ("best_inlier", "u1"), ("_pad", "u1", (3,))])
SIM3_STATE_DTYPE = np.dtype([("status", "<i4"), ("n1", "<i4"), ("n", "<i4"), ("max_its", "<i4"),
                             ("iterations", "<i4"), ("best_inliers", "<i4"),
                             ("best_iteration", "<i4"), ("min_inliers", "<i4"),
                             ("fix_scale", "<i4"), ("best_scale", "<f4"), ("best_R", "<f4", (9,)),
                             ("best_t", "<f4", (3,)), ("best_T12", "<f4", (16,)),
                             ("k1", "<f4", (4,)), ("k2", "<f4", (4,))])
SIM3_RESULT_DTYPE = np.dtype([("has_sim3", "<i4"), ("no_more", "<i4"), ("n_inliers", "<i4"),
                              ("iterations_run", "<i4"), ("T12", "<f4", (16,)),
                              ("R", "<f4", (9,)), ("t", "<f4", (3,)), ("scale", "<f4")])
assert SIM3_CORR_DTYPE.itemsize == 56 and SIM3_STATE_DTYPE.itemsize == 184
assert SIM3_RESULT_DTYPE.itemsize == 132
SIM3_OPT_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_corr", "<i4"), ("n_bad", "<i4"),
                                  ("n_inliers", "<i4"), ("q", "<f8", (4,)), ("t", "<f8", (3,)),
                                  ("s", "<f8"), ("R", "<f4", (9,)), ("t_f", "<f4", (3,)),
                                  ("s_f", "<f4"), ("_pad", "<i4")])
assert SIM3_OPT_RESULT_DTYPE.itemsize == 136
NEW_POINT_INFO_DTYPE = np.dtype([("gated", "<i4"), ("overflow", "<i4"), ("n_new", "<i4"),
                                 ("first_point", "<i4"), ("counts", "<i4", (12,))])
assert NEW_POINT_INFO_DTYPE.itemsize == 64
TRI_MATCH_INFO_DTYPE = np.dtype([("n_matches", "<i4"), ("n_accepted", "<i4"),
                                 ("n_common_nodes", "<i4"), ("n_tried", "<i4"),
                                 ("n_shared2", "<i4"), ("n_undefined", "<i4")])
assert TRI_MATCH_INFO_DTYPE.itemsize == 24
SIM3_SEARCH_INFO_DTYPE = np.dtype([("n_found", "<i4"), ("n_kept", "<i4"), ("n_total", "<i4"),
                                   ("n_best12", "<i4"), ("n_best21", "<i4")])
assert SIM3_SEARCH_INFO_DTYPE.itemsize == 20
# orb_new_point_info_t.counts / the status bytes (ORB_NP_*)
(NP_NOT_TRIED, NP_NO_MATCH, NP_ACCEPTED, NP_LOW_PARALLAX, NP_W_ZERO, NP_Z1, NP_Z2, NP_REPROJ1,
 NP_REPROJ2, NP_ZERO_DIST, NP_SCALE_RATIO, NP_UNDEFINED) = range(12)
ORB_DEPTH_U16, ORB_DEPTH_F32 = 0, 1


class OrbError(RuntimeError):
    def __init__(self, status: int, what: str):
        self.status = status
        super().__init__(f"{what}: {_status_str(status)} ({status})")


_lib = None


def _status_str(s: int) -> str:
    if _lib is None:
        return str(s)
    return _lib.orb_status_string(s).decode()


class _Frame(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_int32), ("keys", ctypes.c_void_p), ("descriptors", ctypes.c_void_p),
        ("u_right", ctypes.c_void_p), ("min_x", ctypes.c_float), ("max_x", ctypes.c_float),
        ("min_y", ctypes.c_float), ("max_y", ctypes.c_float), ("n_levels", ctypes.c_int32),
        ("scale_factors", ctypes.c_void_p),
    ]


class _MapView(ctypes.Structure):
    _fields_ = [("n_kf", ctypes.c_int32), ("n_mp", ctypes.c_int32)] + [
        (name, ctypes.c_void_p) for name in (
            "kf_rank", "kf_by_rank", "kf_bad", "kf_parent", "kf_cov_offs", "kf_cov",
            "kf_child_offs", "kf_child", "kf_mp_offs", "kf_mp", "mp_obs_offs", "mp_obs",
            "points", "mp_desc")]


def lib() -> ctypes.CDLL:
    """Load liborb_amd.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise OrbError(ORB_ENODEV, f"{LIB_PATH} not built (run __graft_entry__.build())")
    # One HIP runtime per process: torch-ROCm ships its own libamdhip64 (soname
    # libamdhip64.so.7).  Loading torch first lets liborb_amd.so's DT_NEEDED on
    # libamdhip64.so.7 bind to that same copy, so device pointers and streams
    # can be shared with torch (plumbing for device memory / torch.distributed).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(str(LIB_PATH))
    vp, i32, f32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    i64, u64 = ctypes.c_int64, ctypes.c_uint64
    sig = {
        "orb_abi_version": (i32, []),
        "orb_status_string": (ctypes.c_char_p, [i32]),
        "orb_device_count": (i32, [vp]),
        "orb_extractor_create": (i32, [i32, f32, i32, i32, i32, i32, vp]),
        "orb_extractor_destroy": (None, [vp]),
        "orb_extractor_get_levels": (i32, [vp]),
        "orb_extractor_get_scale_factor": (f32, [vp]),
        "orb_extractor_get_scale_factors": (None, [vp, vp]),
        "orb_extractor_get_inverse_scale_factors": (None, [vp, vp]),
        "orb_extractor_get_scale_sigma_squares": (None, [vp, vp]),
        "orb_extractor_get_inverse_scale_sigma_squares": (None, [vp, vp]),
        "orb_extractor_get_features_per_level": (None, [vp, vp]),
        "orb_extractor_capacity": (i32, [vp, i32, i32]),
        "orb_extractor_extract": (i32, [vp, vp, i32, i32, sz, vp, vp, i32, vp]),
        "orb_extractor_pyramid_level": (i32, [vp, i32, vp, sz, vp, vp]),
        "orb_extractor_blurred_level": (i32, [vp, i32, vp, sz, vp, vp]),
        "orb_extractor_host_pyramid": (i32, [vp, i32, vp, vp, vp, vp]),
        "orb_extractor_host_pyramid_off": (i32, [vp]),
        "orb_extractor_extract_batch": (i32, [vp, vp, i32, i32, i32, sz, sz, vp, vp, i32, vp, vp]),
        "orb_extractor_batch_level": (i32, [vp, i32, i32, vp, vp, vp, vp]),
        "orb_match_projection_local_stage": (i32, [vp, i32, i32, vp]),
        "orb_match_projection_local_begin": (i32, [vp, vp, i32, i32]),
        "orb_match_projection_local_staged": (i32, [vp, vp, i32, i32, i32, f32, f32, vp, vp]),
        "orb_extractor_stream": (vp, [vp]),
        "orb_extractor_profile": (i32, [vp, i32]),
        "orb_extractor_profile_read": (i32, [vp, i32, vp, vp, vp]),
        "orb_descriptor_distance": (i32, [vp, vp]),
        "orb_matcher_create": (i32, [i32, vp]),
        "orb_matcher_destroy": (None, [vp]),
        "orb_matcher_stream": (vp, [vp]),
        "orb_matcher_profile": (i32, [vp, i32]),
        "orb_matcher_set_resolve": (i32, [vp, i32, i32]),
        "orb_matcher_resolve_kernel": (i32, [vp, i32, i32, i32, vp]),
        "orb_matcher_profile_read": (i32, [vp, i32, vp, vp, vp]),
        "orb_hamming_batch": (i32, [vp, vp, vp, i32, vp, vp]),
        "orb_match_projection_local": (i32, [vp, vp, vp, i32, vp, vp, f32, f32, vp, vp]),
        "orb_match_projection_local_batch": (
            i32, [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, f32, f32, f32, f32, i32, vp,
                  f32, f32, vp, vp, vp]),
        "orb_stereo_match": (i32, [vp, vp, vp, vp]),
        "orb_stereo_match_extracted": (i32, [vp, vp, vp, f32, f32, vp, vp, i32, vp]),
        "orb_stereo_match_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, f32,
                                         vp, vp, vp, vp]),
        "orb_match_projection_frame": (i32, [vp, vp, vp, i32, vp, vp, vp, f32, f32, i32, i32, vp,
                                             vp]),
        "orb_match_bow": (i32, [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp,
                                vp, vp, f32, i32, vp, vp]),
        "orb_frustum": (i32, [vp, i32, vp, vp, vp, f32, f32, f32, f32, f32, f32, i32, vp, vp]),
        "orb_frustum_batch": (i32, [vp, i32, vp, vp, i32, vp, vp, f32, f32, f32, f32, f32, f32,
                                    i32, vp, vp, vp]),
        "orb_search_for_initialization": (i32, [vp, vp, vp, vp, i32, f32, i32, vp, vp]),
        "orb_search_for_initialization_batch": (
            i32, [vp, i32, vp, vp, vp, vp, vp, vp, i32, f32, f32, f32, f32, i32, f32, i32, vp, vp,
                  vp, vp]),
        "orb_distinctive_descriptors": (i32, [vp, i32, vp, vp, vp, vp]),
        "orb_distinctive_descriptors_batch": (i32, [vp, i32, vp, vp, vp, vp, vp]),
        "orb_search_by_projection_reloc": (i32, [vp, vp, vp, vp, vp, f32, i32, vp, vp, vp, f32,
                                                 i32, i32, vp, vp]),
        "orb_search_by_projection_sim3": (i32, [vp, vp, vp, vp, f32, i32, vp, vp, f32, vp, vp]),
        "orb_fuse": (i32, [vp, vp, vp, vp, vp, f32, i32, vp, vp, f32, vp, vp]),
        "orb_fuse_sim3": (i32, [vp, vp, vp, vp, f32, i32, vp, vp, f32, vp, vp]),
        "orb_search_by_sim3": (i32, [vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                     vp, vp, f32, vp, vp, f32, vp, vp]),
        "orb_match_bow_kf": (i32, [vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp,
                                   i32, vp, vp, vp, f32, i32, vp, vp]),
        "orb_search_for_triangulation": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32,
                                               vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp]),
        "orb_vocabulary_create": (i32, [i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
        "orb_vocabulary_load_text": (i32, [i32, ctypes.c_char_p, vp]),
        "orb_vocabulary_destroy": (None, [vp]),
        "orb_vocabulary_info": (i32, [vp, vp]),
        "orb_vocabulary_stream": (vp, [vp]),
        "orb_vocabulary_transform": (i32, [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "orb_vocabulary_transform_batch": (i32, [vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp,
                                                 vp, vp, vp, vp, vp, vp]),
        "orb_vocabulary_score": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp]),
        "orb_vocabulary_score_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "orb_kf_database_create": (i32, [vp, vp]),
        "orb_kf_database_destroy": (None, [vp]),
        "orb_kf_database_clear": (i32, [vp]),
        "orb_kf_database_size": (i32, [vp]),
        "orb_kf_database_add": (i32, [vp, i64, i32, vp, vp]),
        "orb_kf_database_erase": (i32, [vp, i64]),
        "orb_kf_database_set_covisibility": (i32, [vp, i64, i32, vp]),
        "orb_kf_database_detect_relocalization": (i32, [vp, u64, i32, vp, vp, vp, i32, vp]),
        "orb_kf_database_detect_loop": (i32, [vp, u64, i32, vp, vp, i32, vp, f32, vp, i32, vp]),
        "orb_kf_database_last_query": (i32, [vp, vp, vp, vp, vp, i32, vp]),
        "orb_kf_database_profile": (i32, [vp, i32, i32, vp, vp]),
        "orb_undistort_points": (i32, [vp, i32, vp, vp, vp, i32, vp]),
        "orb_undistort_keypoints": (i32, [vp, i32, vp, vp, vp, i32, vp]),
        "orb_compute_image_bounds": (i32, [vp, i32, i32, vp, vp, i32, vp]),
        "orb_undistort_keypoints_batch": (i32, [vp, i32, vp, vp, i32, vp, vp, i32, vp, vp]),
        "orb_match_projection_local_batch_stereo": (
            i32, [vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, f32, f32, f32, f32, i32, vp,
                  f32, f32, vp, vp, vp]),
        "orb_stereo_from_rgbd": (i32, [vp, i32, vp, vp, vp, i32, i32, i32, sz, f32, f32, vp, vp]),
        "orb_stereo_from_rgbd_batch": (i32, [vp, i32, vp, vp, vp, i32, vp, i32, i32, i32, sz, sz,
                                             f32, f32, vp, vp, vp]),
        "orb_unproject_stereo": (i32, [vp, i32, vp, vp, vp, vp, vp, vp]),
        "orb_unproject_stereo_batch": (i32, [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]),
        "orb_close_points": (i32, [vp, i32, vp, vp, vp, f32, vp, vp, vp]),
        "orb_close_points_batch": (i32, [vp, i32, vp, vp, vp, vp, i32, f32, vp, vp, vp, vp]),
        "orb_close_points_lds_keys": (i32, []),
        "orb_pose_optimization": (i32, [vp, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]),
        "orb_pose_optimization_batch": (i32, [vp, i32, vp, vp, vp, i32, vp, vp, i32, i64, vp, i32,
                                              vp, vp, vp, vp, vp, vp]),
        "orb_pose_optimization_lds_edges": (i32, []),
        "orb_match_projection_frame_batch": (
            i32, [vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, f32,
                  f32, f32, f32, i32, vp, f32, i32, i32, i32, vp, vp, vp]),
        "orb_match_projection_frame_batch_max_stride": (i32, []),
        "orb_track_discard_outliers_batch": (i32, [vp, i32, vp, i32, vp, vp, vp, i32, i32, vp, vp,
                                                   vp]),
        "orb_track_discard_outliers_batch_n": (i32, [vp, i32, vp, i32, vp, vp, vp, i32, i32, vp,
                                                     i32, vp, vp]),
        "orb_match_bow_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                      vp, vp, vp, vp, i32, vp, i64, f32, i32, i32, vp, vp, vp]),
        "orb_match_bow_batch_max_stride": (i32, []),
        "orb_update_local_map_batch": (i32, [vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp,
                                             vp, i32, vp, vp, vp]),
        "orb_update_local_map_max_keyframes": (i32, []),
        "orb_track_local_merge_batch": (i32, [vp, i32, vp, i32, vp, vp, i32, vp, vp]),
        "orb_track_local_map_finish_batch": (i32, [vp, i32, vp, i32, vp, vp, vp, i64, i32, i32,
                                                   vp, vp]),
        "orb_sim3_solver_setup_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp,
                                              vp, i32, vp, vp, i32, ctypes.c_double, i32, i32, vp,
                                              vp, vp]),
        "orb_sim3_solver_max_stride": (i32, []),
        "orb_sim3_solver_iterate_batch": (i32, [vp, i32, i32, vp, vp, vp, i32, ctypes.c_uint32,
                                                i32, i32, vp, vp, vp, vp]),
        "orb_scene_median_depth_batch": (i32, [vp, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp]),
        "orb_scene_median_depth_max_stride": (i32, []),
        "orb_scene_median_depth": (i32, [vp, i32, vp, vp, vp, i32, i32, vp, vp]),
        "orb_create_new_map_points_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp,
                                                  vp, vp, vp, vp, vp, i32, i32, vp, i32, vp, vp,
                                                  vp, vp, vp, vp, vp]),
        "orb_create_new_map_points_max_stride": (i32, []),
        "orb_create_new_map_points": (i32, [vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp,
                                            vp, f32, vp, vp, vp, vp, i32, i32, vp, i32, vp, vp,
                                            vp, vp, vp]),
        "orb_search_for_triangulation_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                     vp, vp, vp, i32, vp, vp, vp, vp, i32, i32,
                                                     i32, vp, vp, vp]),
        "orb_search_for_triangulation_batch_max_stride": (i32, []),
        "orb_optimize_sim3_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp,
                                          vp, i32, vp, vp, f32, i32, vp, vp]),
        "orb_optimize_sim3_max_stride": (i32, []),
        "orb_optimize_sim3": (i32, [vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, i32,
                                    vp, vp, f32, i32, vp]),
        "orb_pinned_exp_batch": (i32, [vp, i32, vp, vp, vp]),
        "orb_match_bow_kf_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp,
                                         f32, i32, i32, vp, vp, vp, vp]),
        "orb_match_bow_kf_batch_max_stride": (i32, []),
        "orb_search_by_sim3_batch": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp,
                                           vp, vp, vp, vp, f32, f32, f32, f32, i32, vp, f32, f32,
                                           vp, vp, vp]),
        "orb_search_by_sim3_batch_max_stride": (i32, []),
        "orb_synth_image": (None, [ctypes.c_uint64, i32, i32, i32, i32, vp, sz]),
        "orb_synth_local_map": (None, [ctypes.c_uint64, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
    }
    # entries an older build named by ORB_AMD_LIB (a baseline for an A/B
    # measurement) does not have; calling one there is an AttributeError
    newer = ("orb_match_projection_frame_batch", "orb_match_projection_frame_batch_max_stride",
             "orb_track_discard_outliers_batch", "orb_track_discard_outliers_batch_n",
             "orb_match_bow_batch", "orb_match_bow_batch_max_stride",
             "orb_update_local_map_batch", "orb_update_local_map_max_keyframes",
             "orb_track_local_merge_batch", "orb_track_local_map_finish_batch",
             "orb_sim3_solver_setup_batch", "orb_sim3_solver_max_stride",
             "orb_sim3_solver_iterate_batch", "orb_scene_median_depth_batch",
             "orb_scene_median_depth_max_stride", "orb_scene_median_depth",
             "orb_create_new_map_points_batch", "orb_create_new_map_points_max_stride",
             "orb_create_new_map_points", "orb_search_for_triangulation_batch",
             "orb_search_for_triangulation_batch_max_stride", "orb_optimize_sim3_batch",
             "orb_optimize_sim3_max_stride", "orb_optimize_sim3", "orb_pinned_exp_batch",
             "orb_match_bow_kf_batch", "orb_match_bow_kf_batch_max_stride",
             "orb_search_by_sim3_batch", "orb_search_by_sim3_batch_max_stride")
    for name, (res, args) in sig.items():
        if name in newer and "ORB_AMD_LIB" in os.environ and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


_HIP_RT = None


def _hip_runtime() -> ctypes.CDLL:
    """The HIP runtime this process already uses: liborb_amd.so's dependency,
    looked up by its SONAME, so the loaded copy (torch's, when torch came
    first) is returned rather than a second runtime."""
    global _HIP_RT
    if _HIP_RT is None:
        lib()
        _HIP_RT = ctypes.CDLL("libamdhip64.so.7")
    return _HIP_RT


def _check(status: int, what: str) -> int:
    if status not in (ORB_OK,):
        raise OrbError(status, what)
    return status


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def match_bow_batch_max_stride() -> int:
    """orb_match_bow_batch_max_stride(): a pure function of k_bow_batch's LDS
    layout, callable without a device."""
    return lib().orb_match_bow_batch_max_stride()


def search_for_triangulation_batch_max_stride() -> int:
    """orb_search_for_triangulation_batch_max_stride(): a pure function of
    k_tri_batch's LDS layout, callable without a device."""
    return lib().orb_search_for_triangulation_batch_max_stride()


def match_bow_kf_batch_max_stride() -> int:
    """orb_match_bow_kf_batch_max_stride(): a pure function of k_bow_kf_batch's
    LDS layout, callable without a device."""
    return lib().orb_match_bow_kf_batch_max_stride()


def search_by_sim3_batch_max_stride() -> int:
    """orb_search_by_sim3_batch_max_stride(): a pure function of
    k_sim3_search_batch's LDS layout, callable without a device."""
    return lib().orb_search_by_sim3_batch_max_stride()


def update_local_map_max_keyframes() -> int:
    """orb_update_local_map_max_keyframes(): the largest keyframe count (and
    kf_stride) update_local_map_batch accepts; a pure function of k_local_map's
    LDS layout, callable without a device."""
    return lib().orb_update_local_map_max_keyframes()


def sim3_solver_max_stride() -> int:
    """orb_sim3_solver_max_stride(): the largest kp_stride the Sim3Solver batch
    accepts; a pure function of k_sim3_iterate's LDS layout, callable without
    a device."""
    return lib().orb_sim3_solver_max_stride()


def optimize_sim3_max_stride() -> int:
    """orb_optimize_sim3_max_stride(): the largest kp_stride optimize_sim3_batch
    accepts; a pure function of k_optimize_sim3's LDS layout, callable without
    a device."""
    return lib().orb_optimize_sim3_max_stride()


class MapView:
    """orb_map_view_t from numpy arrays: the map as Tracking::UpdateLocalMap
    reads it, copied to the device once and kept there.

    kf_rank (n_kf): position of each keyframe in std::map / std::set<KeyFrame*>
    order; kf_bad, kf_parent (-1 none); cov / child / kf_mp: per keyframe a CSR
    pair (offs of n_kf + 1 entries, values); mp_obs likewise per map point;
    points (MAP_POINT_DTYPE, n_mp) and mp_desc (n_mp x 32).  to_device(a) copies
    one contiguous array to the device and returns an object with data_ptr()
    (default: a torch CUDA tensor).  Nothing is validated, as in the C entry."""

    def __init__(self, kf_rank, kf_bad, kf_parent, kf_cov_offs, kf_cov, kf_child_offs, kf_child,
                 kf_mp_offs, kf_mp, mp_obs_offs, mp_obs, points, mp_desc, to_device=None):
        if to_device is None:
            import torch

            def to_device(a):
                return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()
        i32 = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)
        rank = i32(kf_rank)
        self.n_kf = len(rank)
        by_rank = np.zeros(self.n_kf, np.int32)
        by_rank[rank] = np.arange(self.n_kf, dtype=np.int32)
        pts = np.ascontiguousarray(points, MAP_POINT_DTYPE).reshape(-1)
        self.n_mp = len(pts)
        host = dict(kf_rank=rank, kf_by_rank=by_rank,
                    kf_bad=np.ascontiguousarray(kf_bad, np.uint8).reshape(-1),
                    kf_parent=i32(kf_parent), kf_cov_offs=i32(kf_cov_offs), kf_cov=i32(kf_cov),
                    kf_child_offs=i32(kf_child_offs), kf_child=i32(kf_child),
                    kf_mp_offs=i32(kf_mp_offs), kf_mp=i32(kf_mp), mp_obs_offs=i32(mp_obs_offs),
                    mp_obs=i32(mp_obs), points=pts,
                    mp_desc=np.ascontiguousarray(mp_desc, np.uint8).reshape(-1))
        self.host = host
        self.dev = {}
        self.c = _MapView(n_kf=self.n_kf, n_mp=self.n_mp)
        for name, a in host.items():
            # an empty list array still needs a valid device address
            t = to_device(a if a.size else np.zeros(16, np.uint8))
            self.dev[name] = t
            setattr(self.c, name, t.data_ptr())

    def addr(self) -> int:
        return ctypes.addressof(self.c)


def device_count() -> int:
    n = ctypes.c_int(0)
    lib().orb_device_count(ctypes.byref(n))
    return n.value


# --------------------------------------------------------------- synthetic input
def synth_image(seed: int, frame: int, width: int, height: int, view: int = 0) -> np.ndarray:
    """Deterministic synthetic grayscale frame (orb_synth_image)."""
    img = np.empty((height, width), np.uint8)
    lib().orb_synth_image(seed, frame, view, width, height, _ptr(img), width)
    return img


def synth_local_map(seed: int, keys: np.ndarray, desc: np.ndarray, n_mp: int, width: int,
                    height: int):
    """SURVEY §8(d) C5 synthetic local map: (mps, mp_desc, kp_locked)."""
    keys = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
    desc = np.ascontiguousarray(desc, np.uint8)
    mps = np.zeros(n_mp, MP_TRACK_DTYPE)
    mp_desc = np.zeros((n_mp, 32), np.uint8)
    locked = np.zeros(len(keys), np.uint8)
    lib().orb_synth_local_map(seed, _ptr(keys), _ptr(desc), len(keys), n_mp, width, height,
                              _ptr(mps), _ptr(mp_desc), _ptr(locked))
    return mps, mp_desc, locked


# ------------------------------------------------------------------- extractor
class ORBextractor:
    """ORB_SLAM2::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)."""

    def __init__(self, nfeatures: int, scaleFactor: float, nlevels: int, iniThFAST: int,
                 minThFAST: int, device: int = 0):
        L = lib()
        h = ctypes.c_void_p()
        _check(L.orb_extractor_create(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST,
                                      device, ctypes.byref(h)), "orb_extractor_create")
        self._h = h
        self.nlevels = nlevels
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            lib().orb_extractor_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def _floats(self, fn) -> list:
        out = np.zeros(self.nlevels, np.float32)
        fn(self._h, _ptr(out))
        return out.tolist()

    def GetLevels(self) -> int:
        return lib().orb_extractor_get_levels(self._h)

    def GetScaleFactor(self) -> float:
        return lib().orb_extractor_get_scale_factor(self._h)

    def GetScaleFactors(self) -> list:
        return self._floats(lib().orb_extractor_get_scale_factors)

    def GetInverseScaleFactors(self) -> list:
        return self._floats(lib().orb_extractor_get_inverse_scale_factors)

    def GetScaleSigmaSquares(self) -> list:
        return self._floats(lib().orb_extractor_get_scale_sigma_squares)

    def GetInverseScaleSigmaSquares(self) -> list:
        return self._floats(lib().orb_extractor_get_inverse_scale_sigma_squares)

    def features_per_level(self) -> list:
        out = np.zeros(self.nlevels, np.int32)
        lib().orb_extractor_get_features_per_level(self._h, _ptr(out))
        return out.tolist()

    def capacity(self, width: int, height: int) -> int:
        return lib().orb_extractor_capacity(self._h, width, height)

    def __call__(self, image: np.ndarray, mask=None):
        """operator(): returns (keypoints[KEYPOINT_DTYPE], descriptors uint8 N x 32).

        An empty image returns (None, None) -- the reference returns with its
        outputs untouched (src/ORBextractor.cc:1095-1096).  A non-uint8 or
        non-2D image is rejected like the reference's assert (:1100)."""
        if image is None or image.size == 0:
            return None, None
        if image.dtype != np.uint8 or image.ndim != 2:
            raise OrbError(ORB_EINVAL, "image must be 8UC1 (CV_8UC1)")
        image = np.ascontiguousarray(image)
        H, W = image.shape
        cap = self.capacity(W, H)
        if cap < 0:
            raise OrbError(ORB_EINVAL, f"unsupported image size {W}x{H}")
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = ctypes.c_int(0)
        _check(lib().orb_extractor_extract(self._h, _ptr(image), W, H, image.strides[0], _ptr(kps),
                                           _ptr(desc), cap, ctypes.byref(n)),
               "orb_extractor_extract")
        return kps[: n.value].copy(), desc[: n.value].copy()

    def host_pyramid(self, level: int) -> np.ndarray:
        """Level `level` of the last __call__ through the library's pinned host
        mirror (orb_extractor_host_pyramid), copied into a new array."""
        p, w, h, st = ctypes.c_void_p(), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
        _check(lib().orb_extractor_host_pyramid(self._h, level, ctypes.byref(p), ctypes.byref(w),
                                                ctypes.byref(h), ctypes.byref(st)), "host_pyramid")
        buf = (ctypes.c_uint8 * (st.value * (h.value - 1) + w.value)).from_address(p.value)
        a = np.frombuffer(buf, np.uint8)
        return np.lib.stride_tricks.as_strided(a, (h.value, w.value), (st.value, 1)).copy()

    def host_pyramid_off(self):
        """Stop the per-call host mirror of levels 1.. (orb_extractor_host_pyramid_off)."""
        _check(lib().orb_extractor_host_pyramid_off(self._h), "host_pyramid_off")

    @property
    def mvImagePyramid(self) -> list:
        """Host copies of the last image's pyramid levels."""
        L = lib()
        out = []
        for l in range(self.nlevels):
            w, h = ctypes.c_int(0), ctypes.c_int(0)
            _check(L.orb_extractor_pyramid_level(self._h, l, None, 0, ctypes.byref(w),
                                                 ctypes.byref(h)), "pyramid_level")
            a = np.zeros((h.value, w.value), np.uint8)
            _check(L.orb_extractor_pyramid_level(self._h, l, _ptr(a), w.value, None, None),
                   "pyramid_level")
            out.append(a)
        return out

    def blurred_levels(self) -> list:
        """Host copies of the last image's 7x7-blurred levels (what rBRIEF samples)."""
        L = lib()
        out = []
        for l in range(self.nlevels):
            w, h = ctypes.c_int(0), ctypes.c_int(0)
            _check(L.orb_extractor_blurred_level(self._h, l, None, 0, ctypes.byref(w),
                                                 ctypes.byref(h)), "blurred_level")
            a = np.zeros((h.value, w.value), np.uint8)
            _check(L.orb_extractor_blurred_level(self._h, l, _ptr(a), w.value, None, None),
                   "blurred_level")
            out.append(a)
        return out

    def extract_batch(self, d_images: int, n_images: int, width: int, height: int, stride: int,
                      image_pitch: int, d_keypoints: int, d_descriptors: int, capacity: int,
                      d_counts: int, stream: int = 0):
        """Device-resident batch form (raw device pointers, e.g. torch .data_ptr())."""
        _check(lib().orb_extractor_extract_batch(self._h, d_images, n_images, width, height,
                                                 stride, image_pitch, d_keypoints, d_descriptors,
                                                 capacity, d_counts, stream or None),
               "orb_extractor_extract_batch")

    def stream(self) -> int:
        return lib().orb_extractor_stream(self._h) or 0

    def batch_level(self, image: int, level: int) -> np.ndarray:
        """Host copy of pyramid level `level` of batch image `image` after
        extract_batch (orb_extractor_batch_level's device view, copied with the
        process's HIP runtime; call after the batch's stream is synchronised)."""
        p, w, h, st = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        _check(lib().orb_extractor_batch_level(self._h, image, level, ctypes.byref(p), ctypes.byref(w),
                                               ctypes.byref(h), ctypes.byref(st)),
               "orb_extractor_batch_level")
        out = np.zeros((h.value, w.value), np.uint8)
        hip = _hip_runtime()
        rc = hip.hipMemcpy2D(ctypes.c_void_p(out.ctypes.data), ctypes.c_size_t(w.value), p, st,
                             ctypes.c_size_t(w.value), ctypes.c_size_t(h.value), ctypes.c_int(2))
        if rc != 0:
            raise OrbError(ORB_EDEVICE, f"hipMemcpy2D -> {rc}")
        return out

    def profile(self, enable: bool = True):
        _check(lib().orb_extractor_profile(self._h, int(enable)), "profile")

    def profile_read(self, stage: int):
        ms = ctypes.c_double(0)
        n = ctypes.c_int(0)
        name = ctypes.c_char_p()
        _check(lib().orb_extractor_profile_read(self._h, stage, ctypes.byref(ms), ctypes.byref(n),
                                                ctypes.byref(name)), "profile_read")
        return name.value.decode(), ms.value, n.value


# --------------------------------------------------------------------- matcher
class Frame:
    """The Frame members ORBmatcher reads (src/Frame.cc, include/Frame.h)."""

    def __init__(self, keys, descriptors, scale_factors, width, height, u_right=None,
                 min_x=0.0, min_y=0.0):
        self.mvKeysUn = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
        self.mDescriptors = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        self.mvScaleFactors = np.ascontiguousarray(scale_factors, np.float32)
        self.mvuRight = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        self.mnMinX, self.mnMaxX = float(min_x), float(width)
        self.mnMinY, self.mnMaxY = float(min_y), float(height)
        self.N = len(self.mvKeysUn)

    def _c(self) -> _Frame:
        f = _Frame()
        f.n = self.N
        f.keys = _ptr(self.mvKeysUn) if self.N else None
        f.descriptors = _ptr(self.mDescriptors) if self.N else None
        f.u_right = _ptr(self.mvuRight) if self.mvuRight is not None else None
        f.min_x, f.max_x, f.min_y, f.max_y = self.mnMinX, self.mnMaxX, self.mnMinY, self.mnMaxY
        f.n_levels = len(self.mvScaleFactors)
        f.scale_factors = _ptr(self.mvScaleFactors)
        return f


class _LocalStage(ctypes.Structure):  # orb_local_stage_t
    _fields_ = [("keys", ctypes.c_void_p), ("descriptors", ctypes.c_void_p),
                ("u_right", ctypes.c_void_p), ("kp_locked", ctypes.c_void_p),
                ("mps", ctypes.c_void_p), ("mp_desc", ctypes.c_void_p)]


class _StereoInput(ctypes.Structure):
    _fields_ = [
        ("left", ctypes.c_void_p), ("n_right", ctypes.c_int32), ("right_keys", ctypes.c_void_p),
        ("right_desc", ctypes.c_void_p), ("n_levels", ctypes.c_int32),
        ("left_levels", ctypes.c_void_p), ("right_levels", ctypes.c_void_p),
        ("level_width", ctypes.c_void_p), ("level_height", ctypes.c_void_p),
        ("level_stride", ctypes.c_void_p), ("inv_scale_factors", ctypes.c_void_p),
        ("bf", ctypes.c_float), ("fx", ctypes.c_float),
    ]


class _Camera(ctypes.Structure):
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float),
                ("cy", ctypes.c_float), ("bf", ctypes.c_float), ("mb", ctypes.c_float)]


class ORBmatcher:
    """ORB_SLAM2::ORBmatcher(nnratio=0.6, checkOri=true)."""

    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

    def __init__(self, nnratio: float = 0.6, checkOri: bool = True, device: int = 0):
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)
        h = ctypes.c_void_p()
        _check(lib().orb_matcher_create(device, ctypes.byref(h)), "orb_matcher_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().orb_matcher_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @staticmethod
    def DescriptorDistance(a: np.ndarray, b: np.ndarray) -> int:
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        return lib().orb_descriptor_distance(_ptr(a), _ptr(b))

    def profile(self, enable: bool = True):
        _check(lib().orb_matcher_profile(self._h, int(enable)), "profile")

    def profile_read(self, stage: int):
        ms = ctypes.c_double(0)
        n = ctypes.c_int(0)
        name = ctypes.c_char_p()
        _check(lib().orb_matcher_profile_read(self._h, stage, ctypes.byref(ms), ctypes.byref(n),
                                              ctypes.byref(name)), "profile_read")
        return name.value.decode(), ms.value, n.value

    def stream(self) -> int:
        return lib().orb_matcher_stream(self._h) or 0

    # resolve schedules of SearchByProjection(F, localMap) (orb_abi.h)
    RESOLVE_AUTO, RESOLVE_PREFIX, RESOLVE_FIXED_POINT, RESOLVE_JACOBI = 0, 1, 2, 3
    RESOLVE_KERNELS = {1: "k_proj_resolve<1>", 4: "k_proj_resolve<4>", 8: "k_proj_resolve<8>",
                       16: "k_proj_resolve_fp<1024>", 32: "k_proj_jacobi+k_proj_resolve_fp"}

    def set_resolve(self, schedule: int, jacobi_rounds: int = 6):
        """Resolve schedule of the local-map matcher (every schedule is exact)."""
        _check(lib().orb_matcher_set_resolve(self._h, schedule, jacobi_rounds), "set_resolve")

    def resolve_kernel(self, n_problems: int, kp_stride: int, mp_stride: int) -> str:
        """Name of the resolve kernel a call of this shape launches."""
        k = ctypes.c_int(0)
        _check(lib().orb_matcher_resolve_kernel(self._h, n_problems, kp_stride, mp_stride,
                                                ctypes.byref(k)), "resolve_kernel")
        return self.RESOLVE_KERNELS[k.value]

    def search_by_projection_batch(self, n_problems, d_keys, d_desc, d_nkeys, d_locked, kp_stride,
                                   d_mps, d_mp_desc, d_nmps, mp_stride, width, height,
                                   scale_factors, th, d_kp_match, d_nmatches, stream: int = 0,
                                   min_x=0.0, min_y=0.0):
        """Device-batched SearchByProjection(F, localMap, th) over P problems."""
        sc = np.ascontiguousarray(scale_factors, np.float32)
        _check(lib().orb_match_projection_local_batch(
            self._h, n_problems, d_keys, d_desc, d_nkeys, d_locked or None, kp_stride, d_mps,
            d_mp_desc, d_nmps, mp_stride, min_x, float(width), min_y, float(height), len(sc),
            _ptr(sc), th, self.mfNNratio, d_kp_match, d_nmatches, stream or None),
            "orb_match_projection_local_batch")

    def hamming_batch(self, d_a: int, d_b: int, n: int, d_out: int, stream: int = 0):
        _check(lib().orb_hamming_batch(self._h, d_a, d_b, n, d_out, stream or None), "hamming")

    def SearchByProjection(self, F: Frame, mps: np.ndarray, mp_desc: np.ndarray, th: float,
                           kp_locked: np.ndarray | None = None):
        """SearchByProjection(F, vpMapPoints, th): returns (nmatches, kp_match).

        kp_match[i] = index of the map point assigned to keypoint i by this
        call (F.mvpMapPoints[i] = vpMapPoints[kp_match[i]]) or -1."""
        mps = np.ascontiguousarray(mps, MP_TRACK_DTYPE)
        mp_desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        locked = None if kp_locked is None else np.ascontiguousarray(kp_locked, np.uint8)
        kp_match = np.full(F.N, -1, np.int32)
        nm = ctypes.c_int32(0)
        f = F._c()
        _check(lib().orb_match_projection_local(
            self._h, ctypes.byref(f), _ptr(locked) if locked is not None else None, len(mps),
            _ptr(mps) if len(mps) else None, _ptr(mp_desc) if len(mps) else None, th,
            self.mfNNratio, _ptr(kp_match), ctypes.byref(nm)), "SearchByProjection")
        return nm.value, kp_match

    def SearchByProjectionStaged(self, F: Frame, mps: np.ndarray, mp_desc: np.ndarray, th: float,
                                 kp_locked: np.ndarray | None = None, begin: bool = True):
        """SearchByProjection through the zero-copy pair
        orb_match_projection_local_stage / _staged: the inputs are written
        straight into the handle's pinned block (as the C++ drop-in does);
        with `begin`, _begin sends the frame's part before the map is written."""
        mps = np.ascontiguousarray(mps, MP_TRACK_DTYPE)
        mp_desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        n, M = F.N, len(mps)
        if n == 0:
            return 0, np.zeros(0, np.int32)
        st = _LocalStage()
        _check(lib().orb_match_projection_local_stage(self._h, n, M, ctypes.byref(st)), "stage")

        def view(ptr, dtype, count):
            nbytes = count * np.dtype(dtype).itemsize
            buf = (ctypes.c_uint8 * max(nbytes, 1)).from_address(ptr)
            return np.frombuffer(buf, np.uint8, nbytes).view(dtype)
        view(st.keys, KEYPOINT_DTYPE, n)[:] = F.mvKeysUn
        view(st.descriptors, np.uint8, n * 32)[:] = F.mDescriptors.reshape(-1)
        stereo = F.mvuRight is not None
        if stereo:
            view(st.u_right, np.float32, n)[:] = F.mvuRight
        if kp_locked is not None:
            view(st.kp_locked, np.uint8, n)[:] = kp_locked
        f = F._c()
        if begin:
            _check(lib().orb_match_projection_local_begin(self._h, ctypes.byref(f), int(stereo),
                                                          int(kp_locked is not None)), "begin")
        if M:
            view(st.mps, MP_TRACK_DTYPE, M)[:] = mps
            view(st.mp_desc, np.uint8, M * 32)[:] = mp_desc.reshape(-1)
        kp_match = np.full(n, -1, np.int32)
        nm = ctypes.c_int32(0)
        _check(lib().orb_match_projection_local_staged(
            self._h, ctypes.byref(f), M, int(stereo), int(kp_locked is not None), th, self.mfNNratio,
            _ptr(kp_match), ctypes.byref(nm)), "SearchByProjectionStaged")
        return nm.value, kp_match


    # ---------------------------------------------------- Frame::ComputeStereoMatches
    def ComputeStereoMatchesExtracted(self, left_ext, right_ext, bf: float, fx: float):
        """Frame::ComputeStereoMatches for the pair last extracted by the two
        handles' __call__ (orb_stereo_match_extracted): nothing but mvuRight /
        mvDepth crosses PCIe.  Returns (mvuRight, mvDepth)."""
        n = ctypes.c_int(0)
        L = lib()
        _check(L.orb_stereo_match_extracted(self._h, left_ext.handle, right_ext.handle, bf, fx,
                                            None, None, 0, ctypes.byref(n)),
               "orb_stereo_match_extracted")
        ur = np.full(n.value, -1, np.float32)
        dp = np.full(n.value, -1, np.float32)
        if n.value:
            _check(L.orb_stereo_match_extracted(self._h, left_ext.handle, right_ext.handle, bf,
                                                fx, _ptr(ur), _ptr(dp), n.value, ctypes.byref(n)),
                   "orb_stereo_match_extracted")
        return ur, dp

    def ComputeStereoMatches(self, left: Frame, right_keys, right_desc, left_pyramid,
                             right_pyramid, inv_scale_factors, bf: float, fx: float):
        """Frame::ComputeStereoMatches (src/Frame.cc:516-704): (mvuRight, mvDepth)."""
        rk = np.ascontiguousarray(right_keys, KEYPOINT_DTYPE)
        rd = np.ascontiguousarray(right_desc, np.uint8).reshape(-1, 32)
        L = len(left_pyramid)
        lp = [np.ascontiguousarray(a, np.uint8) for a in left_pyramid]
        rp = [np.ascontiguousarray(a, np.uint8) for a in right_pyramid]
        for a, b in zip(lp, rp):
            if a.shape != b.shape:
                raise OrbError(ORB_EINVAL, "left/right pyramid level shapes differ")
        lptr = (ctypes.c_void_p * L)(*[a.ctypes.data for a in lp])
        rptr = (ctypes.c_void_p * L)(*[a.ctypes.data for a in rp])
        w = np.array([a.shape[1] for a in lp], np.int32)
        h = np.array([a.shape[0] for a in lp], np.int32)
        st = np.array([a.strides[0] for a in lp], np.int64)
        inv = np.ascontiguousarray(inv_scale_factors, np.float32)
        f = left._c()
        s = _StereoInput()
        s.left = ctypes.addressof(f)
        s.n_right = len(rk)
        s.right_keys = _ptr(rk) if len(rk) else None
        s.right_desc = _ptr(rd) if len(rk) else None
        s.n_levels = L
        s.left_levels, s.right_levels = ctypes.addressof(lptr), ctypes.addressof(rptr)
        s.level_width, s.level_height, s.level_stride = _ptr(w), _ptr(h), _ptr(st)
        s.inv_scale_factors = _ptr(inv)
        s.bf, s.fx = bf, fx
        ur = np.full(left.N, -1, np.float32)
        dp = np.full(left.N, -1, np.float32)
        _check(lib().orb_stereo_match(self._h, ctypes.byref(s), _ptr(ur), _ptr(dp)),
               "ComputeStereoMatches")
        return ur, dp

    def stereo_match_batch(self, n_pairs, left_ext, right_ext, d_lk, d_ld, d_ln, d_rk, d_rd,
                           d_rn, kp_stride, bf, fx, d_ur, d_depth, d_sad, stream: int = 0):
        _check(lib().orb_stereo_match_batch(self._h, n_pairs, left_ext.handle, right_ext.handle,
                                            d_lk, d_ld, d_ln, d_rk, d_rd, d_rn, kp_stride, bf, fx,
                                            d_ur, d_depth, d_sad, stream or None),
               "orb_stereo_match_batch")

    # -------------------------------------------- SearchByProjection(F, LastFrame)
    def SearchByProjectionFrame(self, current: Frame, last, last_desc, cam, tlc_z: float,
                                th: float, bMono: bool, kp_locked=None):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono): (nmatches, kp_match).
        kp_match: MapPoint id assigned, -1 untouched, -2 reset by the rotation filter.
        Limit: 4 * (W + 2 * N + max(len(last), 1)) + 128 bytes must fit 160 KiB
        (N = current.N, W = ceil(N / 32), both rounded up to 4), else OrbError
        with ORB_ECAPACITY and nothing is launched."""
        last = np.ascontiguousarray(last, LAST_MP_DTYPE)
        last_desc = np.ascontiguousarray(last_desc, np.uint8).reshape(-1, 32)
        locked = None if kp_locked is None else np.ascontiguousarray(kp_locked, np.uint8)
        c = _Camera(*cam)
        km = np.full(current.N, -1, np.int32)
        nm = ctypes.c_int32(0)
        f = current._c()
        _check(lib().orb_match_projection_frame(
            self._h, ctypes.byref(f), _ptr(locked) if locked is not None else None, len(last),
            _ptr(last) if len(last) else None, _ptr(last_desc) if len(last) else None,
            ctypes.byref(c), tlc_z, th, int(bMono), int(self.mbCheckOrientation), _ptr(km),
            ctypes.byref(nm)), "SearchByProjection(F, LastFrame)")
        return nm.value, km

    # ------------------------------------------------------------ isInFrustum
    def isInFrustum(self, mps, pose, cam, min_x: float, max_x: float, min_y: float, max_y: float,
                    viewingCosLimit: float, logScaleFactor: float, nLevels: int):
        """Tracking::SearchLocalPoints' loop of Frame::isInFrustum over the local map
        (src/Tracking.cc:1360-1377): (nToMatch, tracks as MP_TRACK_DTYPE)."""
        mps = np.ascontiguousarray(mps, MAP_POINT_DTYPE)
        pose = np.ascontiguousarray(pose, POSE_DTYPE).reshape(1)
        tracks = np.zeros(len(mps), MP_TRACK_DTYPE)
        n = ctypes.c_int32(0)
        c = _Camera(*cam)
        _check(lib().orb_frustum(self._h, len(mps), _ptr(mps) if len(mps) else None, _ptr(pose),
                                 ctypes.byref(c), min_x, max_x, min_y, max_y, viewingCosLimit,
                                 logScaleFactor, nLevels, _ptr(tracks) if len(mps) else None,
                                 ctypes.byref(n)), "isInFrustum")
        return n.value, tracks

    def frustum_batch(self, n_problems, d_mps, d_nmps, mp_stride, d_poses, cam, min_x, max_x,
                      min_y, max_y, viewingCosLimit, logScaleFactor, nLevels, d_tracks,
                      d_n_in_view, stream: int = 0):
        c = _Camera(*cam)
        _check(lib().orb_frustum_batch(self._h, n_problems, d_mps, d_nmps, mp_stride, d_poses,
                                       ctypes.byref(c), min_x, max_x, min_y, max_y,
                                       viewingCosLimit, logScaleFactor, nLevels, d_tracks,
                                       d_n_in_view, stream or None), "frustum_batch")

    # ------------------------------------------------------------- SearchByBoW
    def SearchByBoW(self, kf_desc, kf_angle, kf_mp, kf_bad, kf_fv, f_desc, f_angle, f_fv):
        """SearchByBoW(pKF, F, vpMapPointMatches): (nmatches, f_match).
        *_fv = DBoW2 FeatureVector as (node ids ascending, offsets, feature indices)."""
        kd = np.ascontiguousarray(kf_desc, np.uint8)
        ka = np.ascontiguousarray(kf_angle, np.float32)
        km = np.ascontiguousarray(kf_mp, np.int32)
        kb = None if kf_bad is None else np.ascontiguousarray(kf_bad, np.uint8)
        fd = np.ascontiguousarray(f_desc, np.uint8)
        fa = np.ascontiguousarray(f_angle, np.float32)
        kfv = [np.ascontiguousarray(kf_fv[0], np.uint32), np.ascontiguousarray(kf_fv[1], np.int32),
               np.ascontiguousarray(kf_fv[2], np.uint32)]
        ffv = [np.ascontiguousarray(f_fv[0], np.uint32), np.ascontiguousarray(f_fv[1], np.int32),
               np.ascontiguousarray(f_fv[2], np.uint32)]
        fm = np.full(len(fd), -1, np.int32)
        nm = ctypes.c_int32(0)
        _check(lib().orb_match_bow(
            self._h, len(kd), _ptr(kd), _ptr(ka), _ptr(km), _ptr(kb) if kb is not None else None,
            len(kfv[0]), _ptr(kfv[0]), _ptr(kfv[1]), _ptr(kfv[2]), len(fd), _ptr(fd), _ptr(fa),
            len(ffv[0]), _ptr(ffv[0]), _ptr(ffv[1]), _ptr(ffv[2]), self.mfNNratio,
            int(self.mbCheckOrientation), _ptr(fm), ctypes.byref(nm)), "SearchByBoW")
        return nm.value, fm

    # ------------------------------------------- projection-window variants (§8(f))
    @staticmethod
    def _mps(mps):
        return np.ascontiguousarray(mps, MAP_POINT_DTYPE)

    def SearchByProjectionKF(self, F: Frame, pose, cam, logScaleFactor: float, mps, mp_desc,
                             kf_angle, th: float, ORBdist: int, kp_locked=None):
        """SearchByProjection(F, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1622-1759):
        (nmatches, kp_match) -- point index per frame keypoint, -1 none, -2 reset.
        Limit (also of SearchByProjectionSim3): 4 * (W + N + max(len(mps), 1)) + 128
        bytes must fit 160 KiB (N = F.N, W = ceil(N / 32), both rounded up to 4),
        else OrbError with ORB_ECAPACITY and nothing is launched."""
        mps = self._mps(mps)
        md = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        ka = np.ascontiguousarray(kf_angle, np.float32)
        pose = np.ascontiguousarray(pose, POSE_DTYPE).reshape(1)
        lk = None if kp_locked is None else np.ascontiguousarray(kp_locked, np.uint8)
        km = np.full(F.N, -1, np.int32)
        nm = ctypes.c_int32(0)
        f, c = F._c(), _Camera(*cam)
        _check(lib().orb_search_by_projection_reloc(
            self._h, ctypes.byref(f), _ptr(lk) if lk is not None else None, _ptr(pose),
            ctypes.byref(c), logScaleFactor, len(mps), _ptr(mps) if len(mps) else None,
            _ptr(md) if len(mps) else None, _ptr(ka) if len(mps) else None, th, int(ORBdist),
            int(self.mbCheckOrientation), _ptr(km) if F.N else None, ctypes.byref(nm)),
            "SearchByProjection(F, KF)")
        return nm.value, km

    def SearchByProjectionSim3(self, KF: Frame, Scw, cam, logScaleFactor: float, mps, mp_desc,
                               th: float, kp_matched):
        """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:311-425):
        (nmatches, kp_matched updated)."""
        mps = self._mps(mps)
        md = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        S = np.ascontiguousarray(Scw, np.float32).reshape(12)
        km = np.array(kp_matched, np.int32).copy()
        nm = ctypes.c_int32(0)
        f, c = KF._c(), _Camera(*cam)
        _check(lib().orb_search_by_projection_sim3(
            self._h, ctypes.byref(f), _ptr(S), ctypes.byref(c), logScaleFactor, len(mps),
            _ptr(mps) if len(mps) else None, _ptr(md) if len(mps) else None, th,
            _ptr(km) if KF.N else None, ctypes.byref(nm)), "SearchByProjection(KF, Scw)")
        return nm.value, km

    def Fuse(self, KF: Frame, invLevelSigma2, pose, cam, logScaleFactor: float, mps, mp_desc,
             th: float = 3.0):
        """Fuse(pKF, vpMapPoints, th) targets (src/ORBmatcher.cc:903-1077): (n, fuse_idx)."""
        mps = self._mps(mps)
        md = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        inv = np.ascontiguousarray(invLevelSigma2, np.float32)
        pose = np.ascontiguousarray(pose, POSE_DTYPE).reshape(1)
        out = np.full(len(mps), -1, np.int32)
        nm = ctypes.c_int32(0)
        f, c = KF._c(), _Camera(*cam)
        _check(lib().orb_fuse(self._h, ctypes.byref(f), _ptr(inv), _ptr(pose), ctypes.byref(c),
                              logScaleFactor, len(mps), _ptr(mps) if len(mps) else None,
                              _ptr(md) if len(mps) else None, th,
                              _ptr(out) if len(mps) else None, ctypes.byref(nm)), "Fuse")
        return nm.value, out

    def FuseSim3(self, KF: Frame, Scw, cam, logScaleFactor: float, mps, mp_desc, th: float):
        """Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) targets (src/ORBmatcher.cc:1079-1210)."""
        mps = self._mps(mps)
        md = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        S = np.ascontiguousarray(Scw, np.float32).reshape(12)
        out = np.full(len(mps), -1, np.int32)
        nm = ctypes.c_int32(0)
        f, c = KF._c(), _Camera(*cam)
        _check(lib().orb_fuse_sim3(self._h, ctypes.byref(f), _ptr(S), ctypes.byref(c),
                                   logScaleFactor, len(mps), _ptr(mps) if len(mps) else None,
                                   _ptr(md) if len(mps) else None, th,
                                   _ptr(out) if len(mps) else None, ctypes.byref(nm)),
               "Fuse(Scw)")
        return nm.value, out

    def SearchBySim3(self, KF1: Frame, KF2: Frame, logScaleFactor: float, cam, R1w, t1w, R2w,
                     t2w, mps1, valid1, already1, mp_desc1, mps2, valid2, already2, mp_desc2,
                     s12: float, R12, t12, th: float):
        """SearchBySim3 (src/ORBmatcher.cc:1212-1458): (nFound, match12 = idx2 or -1)."""
        f32a = lambda a, n: np.ascontiguousarray(a, np.float32).reshape(n)
        u8 = lambda a: np.ascontiguousarray(a, np.uint8)
        keep = [f32a(R1w, 9), f32a(t1w, 3), f32a(R2w, 9), f32a(t2w, 3), self._mps(mps1),
                u8(valid1), u8(already1), u8(mp_desc1), self._mps(mps2), u8(valid2),
                u8(already2), u8(mp_desc2), f32a(R12, 9), f32a(t12, 3)]
        m12 = np.full(KF1.N, -1, np.int32)
        nm = ctypes.c_int32(0)
        f1, f2, c = KF1._c(), KF2._c(), _Camera(*cam)
        p = [_ptr(a) if a.size else None for a in keep]
        _check(lib().orb_search_by_sim3(self._h, ctypes.byref(f1), ctypes.byref(f2),
                                        logScaleFactor, ctypes.byref(c), *p[:12], s12, p[12],
                                        p[13], th, _ptr(m12) if KF1.N else None,
                                        ctypes.byref(nm)), "SearchBySim3")
        return nm.value, m12

    def SearchByBoWKF(self, desc1, angle1, mp1, bad1, fv1, desc2, angle2, mp2, bad2, fv2):
        """SearchByBoW(pKF1, pKF2, vpMatches12) (src/ORBmatcher.cc:581-716):
        (nmatches, match12 = MapPoint id of KF2 or -1)."""
        d1 = np.ascontiguousarray(desc1, np.uint8)
        d2 = np.ascontiguousarray(desc2, np.uint8)
        a1, a2 = (np.ascontiguousarray(a, np.float32) for a in (angle1, angle2))
        m1, m2 = (np.ascontiguousarray(a, np.int32) for a in (mp1, mp2))
        b1 = None if bad1 is None else np.ascontiguousarray(bad1, np.uint8)
        b2 = None if bad2 is None else np.ascontiguousarray(bad2, np.uint8)
        v1 = [np.ascontiguousarray(fv1[0], np.uint32), np.ascontiguousarray(fv1[1], np.int32),
              np.ascontiguousarray(fv1[2], np.uint32)]
        v2 = [np.ascontiguousarray(fv2[0], np.uint32), np.ascontiguousarray(fv2[1], np.int32),
              np.ascontiguousarray(fv2[2], np.uint32)]
        out = np.full(len(d1), -1, np.int32)
        nm = ctypes.c_int32(0)
        _check(lib().orb_match_bow_kf(
            self._h, len(d1), _ptr(d1), _ptr(a1), _ptr(m1), _ptr(b1) if b1 is not None else None,
            len(v1[0]), _ptr(v1[0]), _ptr(v1[1]), _ptr(v1[2]), len(d2), _ptr(d2), _ptr(a2),
            _ptr(m2), _ptr(b2) if b2 is not None else None, len(v2[0]), _ptr(v2[0]), _ptr(v2[1]),
            _ptr(v2[2]), self.mfNNratio, int(self.mbCheckOrientation), _ptr(out),
            ctypes.byref(nm)), "SearchByBoW(KF, KF)")
        return nm.value, out

    def SearchForTriangulation(self, KF1: Frame, has_mp1, KF2: Frame, has_mp2, levelSigma2, F12,
                               cam, Cw, R2w, t2w, fv1, fv2, bOnlyStereo: bool = False):
        """SearchForTriangulation (src/ORBmatcher.cc:718-901): (nmatches, match12)."""
        h1, h2 = (np.ascontiguousarray(a, np.uint8) for a in (has_mp1, has_mp2))
        keep = [np.ascontiguousarray(a, np.float32).reshape(-1)
                for a in (levelSigma2, F12, Cw, R2w, t2w)]
        v1 = [np.ascontiguousarray(fv1[0], np.uint32), np.ascontiguousarray(fv1[1], np.int32),
              np.ascontiguousarray(fv1[2], np.uint32)]
        v2 = [np.ascontiguousarray(fv2[0], np.uint32), np.ascontiguousarray(fv2[1], np.int32),
              np.ascontiguousarray(fv2[2], np.uint32)]
        out = np.full(KF1.N, -1, np.int32)
        nm = ctypes.c_int32(0)
        f1, f2, c = KF1._c(), KF2._c(), _Camera(*cam)
        _check(lib().orb_search_for_triangulation(
            self._h, ctypes.byref(f1), _ptr(h1), ctypes.byref(f2), _ptr(h2), _ptr(keep[0]),
            _ptr(keep[1]), ctypes.byref(c), _ptr(keep[2]), _ptr(keep[3]), _ptr(keep[4]),
            len(v1[0]), _ptr(v1[0]), _ptr(v1[1]), _ptr(v1[2]), len(v2[0]), _ptr(v2[0]),
            _ptr(v2[1]), _ptr(v2[2]), int(bOnlyStereo), int(self.mbCheckOrientation), _ptr(out),
            ctypes.byref(nm)), "SearchForTriangulation")
        return nm.value, out

    # ------------------------------------------------- SearchForInitialization
    def SearchForInitialization(self, F1: Frame, F2: Frame, vbPrevMatched, windowSize: int = 10):
        """SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
        (src/ORBmatcher.cc:429-577): returns (nmatches, vnMatches12, vbPrevMatched
        updated).  vbPrevMatched: (N1, 2) float32 points."""
        prev = np.array(vbPrevMatched, np.float32).reshape(F1.N, 2).copy()
        m12 = np.full(F1.N, -1, np.int32)
        nm = ctypes.c_int32(0)
        f1, f2 = F1._c(), F2._c()
        _check(lib().orb_search_for_initialization(
            self._h, ctypes.byref(f1), ctypes.byref(f2), _ptr(prev) if F1.N else None,
            int(windowSize), self.mfNNratio, int(self.mbCheckOrientation),
            _ptr(m12) if F1.N else None, ctypes.byref(nm)), "SearchForInitialization")
        return nm.value, m12, prev

    def search_for_initialization_batch(self, n_problems, d_keys1, d_desc1, d_n1, d_keys2,
                                        d_desc2, d_n2, kp_stride, min_x, max_x, min_y, max_y,
                                        windowSize, d_prev, d_matches12, d_nmatches,
                                        stream: int = 0):
        _check(lib().orb_search_for_initialization_batch(
            self._h, n_problems, d_keys1, d_desc1, d_n1, d_keys2, d_desc2, d_n2, kp_stride,
            min_x, max_x, min_y, max_y, int(windowSize), self.mfNNratio,
            int(self.mbCheckOrientation), d_prev, d_matches12, d_nmatches, stream or None),
            "search_for_initialization_batch")

    @staticmethod
    def search_init_limits() -> dict:
        """The SearchForInitialization kernels' sizes, read from the build: `topk`
        (sorted candidates kept per query), `list` (candidates listed per query),
        `stage` (level-0 F2 keypoints staged in LDS) and `max_stride` (largest
        kp_stride / keypoint count accepted).  Callable without a device."""
        L, out = lib(), {}
        for key, name, res in (("topk", "orb_k_init_topk", ctypes.c_size_t),
                               ("list", "orb_k_init_list_len", ctypes.c_size_t),
                               ("stage", "orb_k_init_stage", ctypes.c_size_t),
                               ("max_stride", "orb_k_init_max_stride", ctypes.c_int)):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, []
            out[key] = int(fn())
        return out

    # ----------------------------------------------------- undistortion (Frame)
    @staticmethod
    def _cam(K, dist):
        K = np.ascontiguousarray(K, np.float32).reshape(9)
        dist = np.ascontiguousarray(dist, np.float32).reshape(-1)
        return K, dist

    def undistort_points(self, xy, K, dist):
        """cv::undistortPoints(src, dst, K, D, noArray(), K) on (n, 2) float points."""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        K, dist = self._cam(K, dist)
        out = np.zeros_like(xy)
        _check(lib().orb_undistort_points(self._h, len(xy), _ptr(xy) if len(xy) else None,
                                          _ptr(K), _ptr(dist), len(dist),
                                          _ptr(out) if len(xy) else None), "undistortPoints")
        return out

    def UndistortKeyPoints(self, mvKeys, K, dist):
        """Frame::UndistortKeyPoints (src/Frame.cc:452-482): returns mvKeysUn."""
        keys = np.ascontiguousarray(mvKeys, KEYPOINT_DTYPE)
        K, dist = self._cam(K, dist)
        out = np.zeros_like(keys)
        _check(lib().orb_undistort_keypoints(self._h, len(keys), _ptr(keys) if len(keys) else None,
                                             _ptr(K), _ptr(dist), len(dist),
                                             _ptr(out) if len(keys) else None),
               "UndistortKeyPoints")
        return out

    def ComputeImageBounds(self, cols, rows, K, dist):
        """Frame::ComputeImageBounds (src/Frame.cc:484-514): (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
        K, dist = self._cam(K, dist)
        b = np.zeros(4, np.float32)
        _check(lib().orb_compute_image_bounds(self._h, cols, rows, _ptr(K), _ptr(dist), len(dist),
                                              _ptr(b)), "ComputeImageBounds")
        return tuple(float(v) for v in b)

    def undistort_keypoints_batch(self, n_frames, d_n, d_keys, stride, K, dist, d_keys_un,
                                  stream: int = 0):
        K, dist = self._cam(K, dist)
        _check(lib().orb_undistort_keypoints_batch(self._h, n_frames, d_n, d_keys, stride, _ptr(K),
                                                   _ptr(dist), len(dist), d_keys_un,
                                                   stream or None), "undistort_keypoints_batch")

    # ------------------------------------------------------- RGB-D depth (Frame)
    def search_by_projection_batch_stereo(self, n_problems, d_keys, d_desc, d_u_right, d_nkeys,
                                          d_locked, kp_stride, d_mps, d_mp_desc, d_nmps,
                                          mp_stride, width, height, scale_factors, th,
                                          d_kp_match, d_nmatches, stream: int = 0, min_x=0.0,
                                          min_y=0.0):
        """search_by_projection_batch for stereo / RGB-D frames: d_u_right holds
        mvuRight per problem at p * kp_stride (src/ORBmatcher.cc:95-100)."""
        sc = np.ascontiguousarray(scale_factors, np.float32)
        _check(lib().orb_match_projection_local_batch_stereo(
            self._h, n_problems, d_keys, d_desc, d_u_right, d_nkeys, d_locked or None, kp_stride,
            d_mps, d_mp_desc, d_nmps, mp_stride, min_x, float(width), min_y, float(height),
            len(sc), _ptr(sc), th, self.mfNNratio, d_kp_match, d_nmatches, stream or None),
            "orb_match_projection_local_batch_stereo")

    @staticmethod
    def _depth_image(imDepth):
        """(array, depth_type) of a CV_16U / CV_32F depth image; rows may be padded."""
        im = np.asarray(imDepth)
        if im.ndim != 2 or im.dtype not in (np.dtype(np.uint16), np.dtype(np.float32)):
            raise OrbError(ORB_EINVAL, "depth image must be 2-D uint16 or float32")
        if im.strides[1] != im.itemsize or im.strides[0] < im.shape[1] * im.itemsize:
            im = np.ascontiguousarray(im)
        return im, (ORB_DEPTH_U16 if im.dtype == np.uint16 else ORB_DEPTH_F32)

    def ComputeStereoFromRGBD(self, mvKeys, mvKeysUn, imDepth, mDepthMapFactor, mbf):
        """Frame::ComputeStereoFromRGBD (src/Frame.cc:707-728) on the depth image
        as GrabImageRGBD receives it (src/Tracking.cc:229-230; uint16 or float32,
        mDepthMapFactor already inverted): returns (mvuRight, mvDepth)."""
        keys = np.ascontiguousarray(mvKeys, KEYPOINT_DTYPE)
        un = np.ascontiguousarray(mvKeysUn, KEYPOINT_DTYPE)
        if len(un) != len(keys):
            raise OrbError(ORB_EINVAL, "mvKeys and mvKeysUn differ in length")
        im, typ = self._depth_image(imDepth)
        n = len(keys)
        ur = np.full(n, -1, np.float32)
        dp = np.full(n, -1, np.float32)
        _check(lib().orb_stereo_from_rgbd(
            self._h, n, _ptr(keys) if n else None, _ptr(un) if n else None, _ptr(im), typ,
            im.shape[1], im.shape[0], im.strides[0], float(mDepthMapFactor), float(mbf),
            _ptr(ur) if n else None, _ptr(dp) if n else None), "ComputeStereoFromRGBD")
        return ur, dp

    def stereo_from_rgbd_batch(self, n_frames, d_n, d_keys, d_keys_un, kp_stride, d_depth,
                               depth_type, cols, rows, row_bytes, image_bytes, depth_map_factor,
                               bf, d_u_right, d_depth_out, stream: int = 0):
        """Device-batched ComputeStereoFromRGBD (orb_stereo_from_rgbd_batch)."""
        _check(lib().orb_stereo_from_rgbd_batch(
            self._h, n_frames, d_n, d_keys, d_keys_un, kp_stride, d_depth, depth_type, cols, rows,
            row_bytes, image_bytes, float(depth_map_factor), float(bf), d_u_right, d_depth_out,
            stream or None), "stereo_from_rgbd_batch")

    @staticmethod
    def _camera(cam):
        return cam if isinstance(cam, _Camera) else _Camera(*[float(v) for v in cam])

    def UnprojectStereo(self, mvKeysUn, mvDepth, pose, cam):
        """Frame::UnprojectStereo (src/Frame.cc:730-744) for every keypoint:
        returns (x3D (n, 3) float32, valid (n,) uint8; invalid rows are 0).
        pose: POSE_DTYPE record; cam: (fx, fy, cx, cy, bf, mb)."""
        un = np.ascontiguousarray(mvKeysUn, KEYPOINT_DTYPE)
        z = np.ascontiguousarray(mvDepth, np.float32)
        if len(z) != len(un):
            raise OrbError(ORB_EINVAL, "mvKeysUn and mvDepth differ in length")
        pose = np.ascontiguousarray(pose, POSE_DTYPE).reshape(1)
        c = self._camera(cam)
        n = len(un)
        x3d = np.zeros((n, 3), np.float32)
        valid = np.zeros(n, np.uint8)
        _check(lib().orb_unproject_stereo(
            self._h, n, _ptr(un) if n else None, _ptr(z) if n else None, _ptr(pose),
            ctypes.addressof(c), _ptr(x3d) if n else None, _ptr(valid) if n else None),
            "UnprojectStereo")
        return x3d, valid

    def unproject_stereo_batch(self, n_frames, d_n, d_keys_un, d_depth, kp_stride, d_poses, cam,
                               d_x3d, d_valid, stream: int = 0):
        """Device-batched UnprojectStereo (orb_unproject_stereo_batch)."""
        c = self._camera(cam)
        _check(lib().orb_unproject_stereo_batch(
            self._h, n_frames, d_n, d_keys_un, d_depth, kp_stride, d_poses, ctypes.addressof(c),
            d_x3d, d_valid, stream or None), "unproject_stereo_batch")

    def ClosePoints(self, mvDepth, mp_state, outlier, mThDepth):
        """The closest-point selection of Tracking::UpdateLastFrame /
        CreateNewKeyFrame and the counts of NeedNewKeyFrame
        (src/Tracking.cc:969-1021, :1263-1318, :1181-1197).  mp_state: 0 no
        MapPoint, 1 one without observations, 2 one with.  Returns (order
        [n_sorted], create [n_visit], n_tracked_close, n_non_tracked_close)."""
        z = np.ascontiguousarray(mvDepth, np.float32)
        n = len(z)
        ms = None if mp_state is None else np.ascontiguousarray(mp_state, np.uint8)
        ol = None if outlier is None else np.ascontiguousarray(outlier, np.uint8)
        if (ms is not None and len(ms) != n) or (ol is not None and len(ol) != n):
            raise OrbError(ORB_EINVAL, "mp_state / outlier differ in length from mvDepth")
        order = np.full(n, -1, np.int32)
        create = np.zeros(n, np.uint8)
        counts = np.zeros(1, CLOSE_COUNTS_DTYPE)
        _check(lib().orb_close_points(
            self._h, n, _ptr(z) if n else None, _ptr(ms) if ms is not None and n else None,
            _ptr(ol) if ol is not None and n else None, float(mThDepth),
            _ptr(order) if n else None, _ptr(create) if n else None, _ptr(counts)),
            "ClosePoints")
        c = counts[0]
        return (order[: c["n_sorted"]].copy(), create[: c["n_visit"]].copy(),
                int(c["n_tracked_close"]), int(c["n_non_tracked_close"]))

    def close_points_batch(self, n_frames, d_n, d_depth, d_mp_state, d_outlier, kp_stride,
                           th_depth, d_order, d_create, d_counts, stream: int = 0):
        """Device-batched ClosePoints (orb_close_points_batch); d_counts holds
        n_frames CLOSE_COUNTS_DTYPE records."""
        _check(lib().orb_close_points_batch(
            self._h, n_frames, d_n, d_depth, d_mp_state or None, d_outlier or None, kp_stride,
            float(th_depth), d_order, d_create, d_counts, stream or None), "close_points_batch")

    @staticmethod
    def close_points_lds_keys() -> int:
        """Largest keypoint-slot count whose keys k_close_points sorts in LDS."""
        return lib().orb_close_points_lds_keys()

    # ------------------------------------------------- Optimizer::PoseOptimization
    def PoseOptimization(self, mvKeysUn, mvuRight, point_index, points, mvInvLevelSigma2, cam,
                         pose, mvbOutlier=None):
        """Optimizer::PoseOptimization (src/Optimizer.cc:243-477) for one frame.
        point_index[i] >= 0 names the row of `points` ((m, 3) float32, or a
        MAP_POINT_DTYPE array) that mvpMapPoints[i] holds; mvuRight None is
        monocular.  Returns (n_inliers, pose POSE_DTYPE record, mvbOutlier
        uint8, info POSE_OPT_INFO_DTYPE record); mvbOutlier slots without an
        edge keep the value passed in (0 when none is)."""
        un = np.ascontiguousarray(mvKeysUn, KEYPOINT_DTYPE)
        n = len(un)
        ur = None if mvuRight is None else np.ascontiguousarray(mvuRight, np.float32)
        idx = np.ascontiguousarray(point_index, np.int32)
        if len(idx) != n or (ur is not None and len(ur) != n):
            raise OrbError(ORB_EINVAL, "mvKeysUn, mvuRight and point_index differ in length")
        pts = np.ascontiguousarray(points)
        if pts.dtype.fields is None:
            pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
            stride = 12
        else:
            stride = pts.dtype.itemsize
        if n and idx.max(initial=-1) >= len(pts):
            raise OrbError(ORB_EINVAL, "point_index names a point past the array")
        lv = np.ascontiguousarray(mvInvLevelSigma2, np.float32)
        pin = np.ascontiguousarray(pose, POSE_DTYPE).reshape(1)
        pout = np.zeros(1, POSE_DTYPE)
        ol = (np.zeros(n, np.uint8) if mvbOutlier is None
              else np.array(mvbOutlier, np.uint8, copy=True))
        if len(ol) != n:
            raise OrbError(ORB_EINVAL, "mvbOutlier differs in length from mvKeysUn")
        info = np.zeros(1, POSE_OPT_INFO_DTYPE)
        c = self._camera(cam)
        _check(lib().orb_pose_optimization(
            self._h, n, _ptr(un) if n else None, _ptr(ur) if ur is not None and n else None,
            _ptr(idx) if n else None, _ptr(pts) if len(pts) else None, stride, _ptr(lv), len(lv),
            ctypes.addressof(c), _ptr(pin), _ptr(pout), _ptr(ol) if n else None, _ptr(info)),
            "PoseOptimization")
        return int(info[0]["n_inliers"]), pout[0], ol, info[0]

    def pose_optimization_batch(self, n_problems, d_nkeys, d_keys_un, d_u_right, kp_stride,
                                d_point_index, d_points, point_stride_bytes, pt_stride,
                                inv_level_sigma2, cam, d_pose_in, d_pose_out, d_outlier, d_info,
                                stream: int = 0):
        """Device-batched PoseOptimization (orb_pose_optimization_batch); d_info
        holds n_problems POSE_OPT_INFO_DTYPE records.  inv_level_sigma2 and cam
        are host values."""
        lv = np.ascontiguousarray(inv_level_sigma2, np.float32)
        c = self._camera(cam)
        _check(lib().orb_pose_optimization_batch(
            self._h, n_problems, d_nkeys, d_keys_un, d_u_right or None, kp_stride, d_point_index,
            d_points, point_stride_bytes, pt_stride, _ptr(lv), len(lv), ctypes.addressof(c),
            d_pose_in, d_pose_out, d_outlier, d_info, stream or None), "pose_optimization_batch")

    @staticmethod
    def pose_optimization_lds_edges() -> int:
        """Largest keypoint-slot count whose edge records k_pose_optimization keeps in LDS."""
        return lib().orb_pose_optimization_lds_edges()

    # ------------------------- TrackWithMotionModel's matcher stage, device batch
    def search_by_projection_frame_batch(self, n_problems, d_keys, d_desc, d_u_right, d_locked,
                                         d_nkeys, kp_stride, d_pose_cur, d_pose_last,
                                         d_last_keys, d_last_nkeys, d_last_point_index,
                                         d_last_outlier, d_points, d_mp_desc, mp_stride, cam,
                                         min_x, max_x, min_y, max_y, scale_factors, th, bMono,
                                         retry_below, d_kp_match, d_info, stream: int = 0):
        """Device-batched SearchByProjection(CurrentFrame, LastFrame, th, bMono)
        with TrackWithMotionModel's 2 * th retry (orb_match_projection_frame_batch).
        d_* are device addresses; d_u_right, d_locked and d_last_outlier may be 0
        (monocular / none); d_info holds n_problems FRAME_MATCH_INFO_DTYPE
        records; cam = (fx, fy, cx, cy, bf, mb) and scale_factors are host
        values.  Asynchronous on `stream`."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        c = self._camera(cam)
        _check(lib().orb_match_projection_frame_batch(
            self._h, n_problems, d_keys, d_desc, d_u_right or None, d_locked or None, d_nkeys,
            kp_stride, d_pose_cur, d_pose_last, d_last_keys, d_last_nkeys, d_last_point_index,
            d_last_outlier or None, d_points, d_mp_desc, mp_stride, ctypes.addressof(c), min_x,
            max_x, min_y, max_y, len(sf), _ptr(sf), th, int(bMono),
            int(self.mbCheckOrientation), retry_below, d_kp_match, d_info, stream or None),
            "search_by_projection_frame_batch")

    @staticmethod
    def search_by_projection_frame_batch_max_stride() -> int:
        """Largest kp_stride search_by_projection_frame_batch accepts."""
        return lib().orb_match_projection_frame_batch_max_stride()

    def track_discard_outliers_batch(self, n_problems, d_nkeys, kp_stride, d_kp_match, d_outlier,
                                     d_points, mp_stride, mark_seen, d_info, d_out,
                                     stream: int = 0):
        """TrackWithMotionModel's "Discard outliers" loop and, with mark_seen,
        SearchLocalPoints' already-matched marking (orb_track_discard_outliers_batch);
        d_out holds n_problems TRACK_DISCARD_INFO_DTYPE records."""
        _check(lib().orb_track_discard_outliers_batch(
            self._h, n_problems, d_nkeys, kp_stride, d_kp_match, d_outlier, d_points, mp_stride,
            int(bool(mark_seen)), d_info, d_out, stream or None), "track_discard_outliers_batch")

    def track_discard_outliers_batch_n(self, n_problems, d_nkeys, kp_stride, d_kp_match,
                                       d_outlier, d_points, mp_stride, mark_seen, d_n_matches,
                                       n_matches_stride, d_out, stream: int = 0):
        """track_discard_outliers_batch with the match counts read from
        d_n_matches[p * n_matches_stride] (int32 units): the first field of a
        FRAME_MATCH_INFO_DTYPE or BOW_MATCH_INFO_DTYPE array, stride 5
        (orb_track_discard_outliers_batch_n)."""
        _check(lib().orb_track_discard_outliers_batch_n(
            self._h, n_problems, d_nkeys, kp_stride, d_kp_match, d_outlier, d_points, mp_stride,
            int(bool(mark_seen)), d_n_matches, n_matches_stride, d_out, stream or None),
            "track_discard_outliers_batch_n")

    # ---------------- TrackReferenceKeyFrame / Relocalization's matcher, device batch
    def search_by_bow_batch(self, n_problems, d_kf_index, d_f_index, d_kf_keys, d_kf_desc,
                            d_kf_nkeys, d_kf_point_index, d_kf_fv_nodes, d_kf_fv_offs,
                            d_kf_fv_feats, d_kf_n_fv_nodes, d_f_keys, d_f_desc, d_f_nkeys,
                            d_f_fv_nodes, d_f_fv_offs, d_f_fv_feats, d_f_n_fv_nodes, kp_stride,
                            d_points, mp_stride, min_matches, d_kp_match, d_info,
                            stream: int = 0):
        """Device-batched SearchByBoW(pKF, F, vpMapPointMatches) (orb_match_bow_batch)
        with this matcher's mfNNratio and mbCheckOrientation.  d_* are device
        addresses in the slot layout of ORBextractor's batch and
        ORBVocabulary.transform_batch; d_kf_index, d_f_index (slot per problem)
        and d_points may be 0 (identity / no bad point); d_info holds n_problems
        BOW_MATCH_INFO_DTYPE records.  Asynchronous on `stream`."""
        _check(lib().orb_match_bow_batch(
            self._h, n_problems, d_kf_index or None, d_f_index or None, d_kf_keys, d_kf_desc,
            d_kf_nkeys, d_kf_point_index, d_kf_fv_nodes, d_kf_fv_offs, d_kf_fv_feats,
            d_kf_n_fv_nodes, d_f_keys, d_f_desc, d_f_nkeys, d_f_fv_nodes, d_f_fv_offs,
            d_f_fv_feats, d_f_n_fv_nodes, kp_stride, d_points or None, mp_stride,
            self.mfNNratio, int(self.mbCheckOrientation), min_matches, d_kp_match, d_info,
            stream or None), "search_by_bow_batch")

    @staticmethod
    def search_by_bow_batch_max_stride() -> int:
        """Largest kp_stride search_by_bow_batch accepts."""
        return lib().orb_match_bow_batch_max_stride()

    # ------------------------------------------------ TrackLocalMap, device batch
    def update_local_map_batch(self, n_problems, view, d_nkeys, d_kp_match, kp_stride,
                               d_local_kf, d_n_local_kf, kf_stride, d_local_index, d_mps,
                               d_mp_desc, d_nmps, mp_stride, d_locked, d_info, stream: int = 0):
        """Tracking::UpdateLocalMap (UpdateLocalKeyFrames, UpdateLocalPoints and
        SearchLocalPoints' already-matched marking) for n_problems frames against
        `view` (a MapView) (orb_update_local_map_batch).  d_* are device
        addresses; d_kp_match, d_local_kf and d_n_local_kf are in/out; d_info
        holds n_problems LOCAL_MAP_INFO_DTYPE records.  Asynchronous on `stream`."""
        _check(lib().orb_update_local_map_batch(
            self._h, n_problems, view.addr() if view is not None else None, d_nkeys or None,
            d_kp_match or None, kp_stride, d_local_kf or None, d_n_local_kf or None, kf_stride,
            d_local_index or None, d_mps or None, d_mp_desc or None, d_nmps or None, mp_stride,
            d_locked or None, d_info or None, stream or None), "update_local_map_batch")

    @staticmethod
    def update_local_map_max_keyframes() -> int:
        """Largest keyframe count and kf_stride update_local_map_batch accepts."""
        return lib().orb_update_local_map_max_keyframes()

    def track_local_merge_batch(self, n_problems, d_nkeys, kp_stride, d_km_local, d_local_index,
                                mp_stride, d_kp_match, stream: int = 0):
        """d_kp_match[i] = d_local_index[d_km_local[i]] where the local matcher
        matched keypoint i (orb_track_local_merge_batch)."""
        _check(lib().orb_track_local_merge_batch(
            self._h, n_problems, d_nkeys or None, kp_stride, d_km_local or None,
            d_local_index or None, mp_stride, d_kp_match or None, stream or None),
            "track_local_merge_batch")

    def track_local_map_finish_batch(self, n_problems, d_nkeys, kp_stride, d_kp_match, d_outlier,
                                     d_points, pt_stride, only_tracking, null_outliers,
                                     d_n_inliers, stream: int = 0):
        """mnMatchesInliers per problem and, with null_outliers (stereo), the
        outliers' matches reset (orb_track_local_map_finish_batch;
        src/Tracking.cc:1109-1135)."""
        _check(lib().orb_track_local_map_finish_batch(
            self._h, n_problems, d_nkeys or None, kp_stride, d_kp_match or None,
            d_outlier or None, d_points or None, pt_stride, int(bool(only_tracking)),
            int(bool(null_outliers)), d_n_inliers or None, stream or None),
            "track_local_map_finish_batch")

    # ------------------------------------- LoopClosing::ComputeSim3's solver, device batch
    @staticmethod
    def _camera4(cam):
        v = [float(x) for x in cam]
        return _Camera(*(v + [0.0] * (6 - len(v))))

    def sim3_solver_setup_batch(self, n_problems, d_kf1_slot, d_kf2_slot, d_kf_keys, d_kf_nkeys,
                                d_kf_point_index, d_kf_pose, kp_stride, d_points, d_match12,
                                d_index1, d_index2, level_sigma2, cam1, cam2, fix_scale,
                                d_state, d_corr, probability: float = 0.99,
                                min_inliers: int = 20, max_iterations: int = 300,
                                stream: int = 0):
        """Sim3Solver's constructor and SetRansacParameters for n_problems
        (pKF1, pKF2, vpMatched12) problems (orb_sim3_solver_setup_batch).  d_* are
        device addresses in the keyframe slot layout of search_by_bow_batch;
        d_kf1_slot, d_kf2_slot and d_index1 may be 0 (identity).  cam1, cam2:
        (fx, fy, cx, cy[, bf, mb]).  d_state holds n_problems SIM3_STATE_DTYPE
        records, d_corr n_problems x kp_stride SIM3_CORR_DTYPE records.
        Asynchronous on `stream`."""
        ls = np.ascontiguousarray(level_sigma2, np.float32).reshape(-1)
        c1, c2 = self._camera4(cam1), self._camera4(cam2)
        _check(lib().orb_sim3_solver_setup_batch(
            self._h, n_problems, d_kf1_slot or None, d_kf2_slot or None, d_kf_keys or None,
            d_kf_nkeys or None, d_kf_point_index or None, d_kf_pose or None, kp_stride,
            d_points or None, d_match12 or None, d_index1 or None, d_index2 or None,
            _ptr(ls) if len(ls) else None, len(ls), ctypes.byref(c1), ctypes.byref(c2),
            int(bool(fix_scale)), float(probability), int(min_inliers), int(max_iterations),
            d_state or None, d_corr or None, stream or None), "sim3_solver_setup_batch")

    def sim3_solver_iterate_batch(self, n_problems, kp_stride, d_state, d_corr, d_draws,
                                  draw_stride, n_iterations, d_inliers12, d_result,
                                  d_active: int = 0, rand_max: int = 2147483647,
                                  max_iterations: int = 300, stream: int = 0):
        """Sim3Solver::iterate(n_iterations) on every problem whose d_active byte
        is not 0 (d_active 0: all) (orb_sim3_solver_iterate_batch).  d_draws:
        raw rand() values, uint32, entry 3 * it + j of each problem's
        draw_stride entries for lifetime iteration it, draw j.  d_result holds
        n_problems SIM3_RESULT_DTYPE records, d_inliers12 n_problems x
        kp_stride bytes.  Asynchronous on `stream`."""
        _check(lib().orb_sim3_solver_iterate_batch(
            self._h, n_problems, kp_stride, d_state or None, d_corr or None, d_draws or None,
            draw_stride, int(rand_max), int(max_iterations), int(n_iterations),
            d_active or None, d_inliers12 or None, d_result or None, stream or None),
            "sim3_solver_iterate_batch")

    @staticmethod
    def sim3_solver_max_stride() -> int:
        """Largest kp_stride the Sim3Solver batch accepts."""
        return lib().orb_sim3_solver_max_stride()

    # ------------------------------------------------- Optimizer::OptimizeSim3
    def optimize_sim3_batch(self, n_problems, d_kf1_slot, d_kf2_slot, d_kf_keys, d_kf_nkeys,
                            d_kf_point_index, d_kf_pose, kp_stride, d_points, d_match12, d_index2,
                            d_start, inv_level_sigma2, cam1, cam2, d_out, th2: float = 10.0,
                            fix_scale: bool = False, d_active: int = 0, stream: int = 0):
        """Optimizer::OptimizeSim3 for n_problems (pKF1, pKF2, vpMatches1, g2oS12)
        problems (orb_optimize_sim3_batch).  d_* are device addresses in the
        slot layout of sim3_solver_setup_batch; d_match12 is updated in place;
        d_start holds n_problems SIM3_RESULT_DTYPE records (the solver's
        d_result serves as it is), d_out n_problems SIM3_OPT_RESULT_DTYPE
        records.  Asynchronous on `stream`."""
        ls = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
        c1, c2 = self._camera4(cam1), self._camera4(cam2)
        _check(lib().orb_optimize_sim3_batch(
            self._h, n_problems, d_kf1_slot or None, d_kf2_slot or None, d_kf_keys or None,
            d_kf_nkeys or None, d_kf_point_index or None, d_kf_pose or None, kp_stride,
            d_points or None, d_match12 or None, d_index2 or None, d_start or None,
            d_active or None, _ptr(ls) if len(ls) else None, len(ls), ctypes.byref(c1),
            ctypes.byref(c2), float(th2), int(bool(fix_scale)), d_out or None, stream or None),
            "optimize_sim3_batch")

    def OptimizeSim3(self, keys1, point_index1, pose1, keys2, pose2, points, match12, index2,
                     start_R, start_t, start_scale, inv_level_sigma2, cam1, cam2,
                     th2: float = 10.0, bFixScale: bool = False):
        """Optimizer::OptimizeSim3 for one problem with host arrays
        (orb_optimize_sim3).  keys1 / keys2: KEYPOINT_DTYPE (mvKeysUn);
        point_index1: GetMapPointMatches() of pKF1 as indices into `points`
        (MAP_POINT_DTYPE); match12: the point index of vpMatches1[i] or
        negative; index2: GetIndexInKeyFrame(pKF2) per i; the start is g2oS12
        as float R (9), t (3) and scale.  Returns (nInliers, match12 updated,
        the SIM3_OPT_RESULT_DTYPE record)."""
        k1 = np.ascontiguousarray(keys1, KEYPOINT_DTYPE).reshape(-1)
        k2 = np.ascontiguousarray(keys2, KEYPOINT_DTYPE).reshape(-1)
        n1 = len(k1)
        pi1 = np.ascontiguousarray(np.asarray(point_index1, np.int32).reshape(-1)[:n1])
        m12 = np.ascontiguousarray(np.asarray(match12, np.int32).reshape(-1)[:n1]).copy()
        i2 = np.ascontiguousarray(np.asarray(index2, np.int32).reshape(-1)[:n1])
        if not (len(pi1) == n1 and len(m12) == n1 and len(i2) == n1):
            raise OrbError(ORB_EINVAL, "OptimizeSim3: arrays shorter than keys1")
        p1, p2 = np.zeros(1, POSE_DTYPE), np.zeros(1, POSE_DTYPE)
        p1[0], p2[0] = pose1, pose2
        pts = np.ascontiguousarray(points, MAP_POINT_DTYPE).reshape(-1)
        st = np.zeros(1, SIM3_RESULT_DTYPE)
        st["has_sim3"], st["scale"] = 1, np.float32(start_scale)
        st["R"][0] = np.asarray(start_R, np.float32).reshape(9)
        st["t"][0] = np.asarray(start_t, np.float32).reshape(3)
        ls = np.ascontiguousarray(inv_level_sigma2, np.float32).reshape(-1)
        c1, c2 = self._camera4(cam1), self._camera4(cam2)
        out = np.zeros(1, SIM3_OPT_RESULT_DTYPE)
        _check(lib().orb_optimize_sim3(
            self._h, _ptr(k1) if n1 else None, n1, _ptr(pi1) if n1 else None, _ptr(p1),
            _ptr(k2) if len(k2) else None, len(k2), _ptr(p2), _ptr(pts) if len(pts) else None,
            len(pts), _ptr(m12) if n1 else None, _ptr(i2) if n1 else None, _ptr(st),
            _ptr(ls) if len(ls) else None, len(ls), ctypes.byref(c1), ctypes.byref(c2),
            float(th2), int(bool(bFixScale)), _ptr(out)), "OptimizeSim3")
        return int(out["n_inliers"][0]), m12, out[0]

    @staticmethod
    def optimize_sim3_max_stride() -> int:
        """Largest kp_stride optimize_sim3_batch accepts."""
        return lib().orb_optimize_sim3_max_stride()

    def pinned_exp_batch(self, n, d_x, d_y, stream: int = 0):
        """pinned_exp over n device doubles (orb_pinned_exp_batch; test support
        for the pin)."""
        _check(lib().orb_pinned_exp_batch(self._h, n, d_x or None, d_y or None, stream or None),
               "pinned_exp_batch")

    # ----------------------------------------- LocalMapping::CreateNewMapPoints
    def scene_median_depth_batch(self, n_problems, d_slot, d_kf_nkeys, d_kf_point_index,
                                 d_kf_pose, kp_stride, d_points, d_median, d_count, q: int = 2,
                                 stream: int = 0):
        """KeyFrame::ComputeSceneMedianDepth(q) for n_problems keyframe slots
        (orb_scene_median_depth_batch).  d_* are device addresses in the slot
        layout of search_by_bow_batch; d_slot may be 0 (identity).  d_median:
        n_problems floats (NaN for a keyframe without points), d_count:
        n_problems int32.  Asynchronous on `stream`."""
        _check(lib().orb_scene_median_depth_batch(
            self._h, n_problems, d_slot or None, d_kf_nkeys or None, d_kf_point_index or None,
            d_kf_pose or None, kp_stride, d_points or None, int(q), d_median or None,
            d_count or None, stream or None), "scene_median_depth_batch")

    def create_new_map_points_batch(self, n_problems, d_kf1_slot, d_kf2_slot, d_kf_keys,
                                    d_kf_nkeys, d_kf_point_index, d_kf_pose, d_kf_u_right,
                                    d_kf_depth, kp_stride, d_match12, d_median_depth, cam1, cam2,
                                    scale_factors, level_sigma2, monocular, d_points,
                                    point_capacity, d_point_cursor, d_cursor_index, d_status,
                                    d_x3d, d_new_pairs, d_info, stream: int = 0):
        """The gate and loop body of LocalMapping::CreateNewMapPoints for
        n_problems (current keyframe, neighbour) pairs
        (orb_create_new_map_points_batch).  d_* are device addresses;
        d_kf_u_right / d_kf_depth 0: monocular keyframes; d_median_depth is read
        only when `monocular`.  cam1, cam2: (fx, fy, cx, cy, bf, mb).  d_status:
        n_problems x kp_stride bytes (NP_* codes), d_x3d: 3 floats per slot,
        d_new_pairs: 2 int32 per slot, d_info: NEW_POINT_INFO_DTYPE records.
        Asynchronous on `stream`."""
        sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
        ls = np.ascontiguousarray(level_sigma2, np.float32).reshape(-1)
        if len(sf) != len(ls):
            raise OrbError(ORB_EINVAL, "scale_factors and level_sigma2 differ in length")
        c1, c2 = self._camera(cam1), self._camera(cam2)
        _check(lib().orb_create_new_map_points_batch(
            self._h, n_problems, d_kf1_slot or None, d_kf2_slot or None, d_kf_keys or None,
            d_kf_nkeys or None, d_kf_point_index or None, d_kf_pose or None,
            d_kf_u_right or None, d_kf_depth or None, kp_stride, d_match12 or None,
            d_median_depth or None, ctypes.byref(c1), ctypes.byref(c2),
            _ptr(sf) if len(sf) else None, _ptr(ls) if len(ls) else None, len(sf),
            int(bool(monocular)), d_points or None, int(point_capacity), d_point_cursor or None,
            d_cursor_index or None, d_status or None, d_x3d or None, d_new_pairs or None,
            d_info or None, stream or None), "create_new_map_points_batch")

    def search_for_triangulation_batch(self, n_problems, d_kf1_slot, d_kf2_slot, d_kf_keys,
                                       d_kf_desc, d_kf_nkeys, d_kf_point_index, d_kf_fv_nodes,
                                       d_kf_fv_offs, d_kf_fv_feats, d_kf_n_fv_nodes, d_kf_u_right,
                                       d_kf_pose, kp_stride, d_f12, cam2, scale_factors,
                                       level_sigma2, only_stereo, d_match12, d_info,
                                       stream: int = 0):
        """Device-batched SearchForTriangulation for n_problems (KF1, KF2) pairs
        (orb_search_for_triangulation_batch) with this matcher's
        mbCheckOrientation.  d_* are device addresses (a torch tensor's
        data_ptr()) in the keyframe slot layout of search_by_bow_batch and
        create_new_map_points_batch; d_kf_u_right 0: every keypoint is
        monocular; d_f12: nine floats per problem (ComputeF12, row-major).
        cam2: (fx, fy, cx, cy[, bf, mb]) of pKF2; scale_factors and
        level_sigma2 are pKF2's.  d_match12: n_problems x kp_stride int32, the
        row create_new_map_points_batch reads; d_info: TRI_MATCH_INFO_DTYPE
        records.  Asynchronous on `stream`."""
        sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
        ls = np.ascontiguousarray(level_sigma2, np.float32).reshape(-1)
        if len(sf) != len(ls):
            raise OrbError(ORB_EINVAL, "scale_factors and level_sigma2 differ in length")
        c2 = self._camera4(cam2)
        _check(lib().orb_search_for_triangulation_batch(
            self._h, n_problems, d_kf1_slot or None, d_kf2_slot or None, d_kf_keys or None,
            d_kf_desc or None, d_kf_nkeys or None, d_kf_point_index or None,
            d_kf_fv_nodes or None, d_kf_fv_offs or None, d_kf_fv_feats or None,
            d_kf_n_fv_nodes or None, d_kf_u_right or None, d_kf_pose or None, kp_stride,
            d_f12 or None, ctypes.byref(c2), _ptr(sf) if len(sf) else None,
            _ptr(ls) if len(ls) else None, len(sf), int(bool(only_stereo)),
            int(self.mbCheckOrientation), d_match12 or None, d_info or None, stream or None),
            "search_for_triangulation_batch")

    @staticmethod
    def search_for_triangulation_batch_max_stride() -> int:
        """Largest kp_stride search_for_triangulation_batch accepts."""
        return lib().orb_search_for_triangulation_batch_max_stride()

    # ------------------------- LoopClosing::ComputeSim3's matchers, device batches
    def search_by_bow_kf_batch(self, n_problems, d_kf1_slot, d_kf2_slot, d_kf_keys, d_kf_desc,
                               d_kf_nkeys, d_kf_point_index, d_kf_fv_nodes, d_kf_fv_offs,
                               d_kf_fv_feats, d_kf_n_fv_nodes, kp_stride, d_points, min_matches,
                               d_match12, d_index2, d_info, stream: int = 0):
        """Device-batched SearchByBoW(pKF1, pKF2, vpMatches12) for n_problems
        pairs of keyframe slots (orb_match_bow_kf_batch) with this matcher's
        mfNNratio and mbCheckOrientation.  d_* are device addresses (a torch
        tensor's data_ptr()) in the keyframe slot layout of
        search_by_bow_batch; d_kf1_slot, d_kf2_slot (0: slot p) and d_points
        (0: no bad point) are optional.  d_match12 / d_index2: n_problems x
        kp_stride int32, the rows sim3_solver_setup_batch reads; d_info:
        BOW_MATCH_INFO_DTYPE records.  min_matches: ComputeSim3's 20 (0: no
        gate).  Asynchronous on `stream`."""
        _check(lib().orb_match_bow_kf_batch(
            self._h, n_problems, d_kf1_slot or None, d_kf2_slot or None, d_kf_keys or None,
            d_kf_desc or None, d_kf_nkeys or None, d_kf_point_index or None,
            d_kf_fv_nodes or None, d_kf_fv_offs or None, d_kf_fv_feats or None,
            d_kf_n_fv_nodes or None, kp_stride, d_points or None, self.mfNNratio,
            int(self.mbCheckOrientation), int(min_matches), d_match12 or None, d_index2 or None,
            d_info or None, stream or None), "search_by_bow_kf_batch")

    @staticmethod
    def search_by_bow_kf_batch_max_stride() -> int:
        """Largest kp_stride search_by_bow_kf_batch accepts."""
        return lib().orb_match_bow_kf_batch_max_stride()

    def search_by_sim3_batch(self, n_problems, d_kf1_slot, d_kf2_slot, d_kf_keys, d_kf_desc,
                             d_kf_nkeys, d_kf_point_index, d_kf_pose, kp_stride, d_points,
                             d_mp_desc, d_match12, d_index2, d_inliers12, d_sim3, cam, bounds,
                             scale_factors, log_scale_factor, d_info, th: float = 7.5,
                             d_active: int = 0, d_new12: int = 0, stream: int = 0):
        """Device-batched SearchBySim3 with ComputeSim3's inlier filter in front
        (orb_search_by_sim3_batch).  d_* are device addresses in the slot
        layout of sim3_solver_setup_batch plus the descriptors per keypoint
        slot (d_kf_desc) and per point (d_mp_desc); d_match12 / d_index2 are
        the solver's rows, updated in place for optimize_sim3_batch;
        d_inliers12 (0: no filter) and d_sim3 (SIM3_RESULT_DTYPE records) are
        the solver's outputs as they stand; d_active and d_new12 are optional.
        cam: (fx, fy, cx, cy[, bf, mb]); bounds: (min_x, max_x, min_y, max_y).
        d_info: SIM3_SEARCH_INFO_DTYPE records.  Asynchronous on `stream`."""
        sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
        c = self._camera4(cam)
        min_x, max_x, min_y, max_y = (float(v) for v in bounds)
        _check(lib().orb_search_by_sim3_batch(
            self._h, n_problems, d_kf1_slot or None, d_kf2_slot or None, d_kf_keys or None,
            d_kf_desc or None, d_kf_nkeys or None, d_kf_point_index or None, d_kf_pose or None,
            kp_stride, d_points or None, d_mp_desc or None, d_match12 or None, d_index2 or None,
            d_inliers12 or None, d_sim3 or None, d_active or None, ctypes.byref(c), min_x, max_x,
            min_y, max_y, len(sf), _ptr(sf) if len(sf) else None, float(log_scale_factor),
            float(th), d_new12 or None, d_info or None, stream or None), "search_by_sim3_batch")

    @staticmethod
    def search_by_sim3_batch_max_stride() -> int:
        """Largest kp_stride search_by_sim3_batch accepts."""
        return lib().orb_search_by_sim3_batch_max_stride()

    @staticmethod
    def create_new_map_points_max_stride() -> int:
        """Largest kp_stride create_new_map_points_batch accepts."""
        return lib().orb_create_new_map_points_max_stride()

    @staticmethod
    def scene_median_depth_max_stride() -> int:
        """Largest kp_stride scene_median_depth_batch accepts."""
        return lib().orb_scene_median_depth_max_stride()

    def ComputeSceneMedianDepth(self, point_index, pose, points, q: int = 2):
        """KeyFrame::ComputeSceneMedianDepth(q) (src/KeyFrame.cc:658-694) for one
        keyframe, host buffers: point_index = GetMapPointMatches() as indices
        into `points` (MAP_POINT_DTYPE; negative NULL), pose a POSE_DTYPE record.
        Returns (median float32, NaN without points; the number of depths)."""
        pi = np.ascontiguousarray(point_index, np.int32).reshape(-1)
        pts = np.ascontiguousarray(points, MAP_POINT_DTYPE).reshape(-1)
        pose = np.ascontiguousarray(pose, POSE_DTYPE).reshape(1)
        med, cnt = np.zeros(1, np.float32), np.zeros(1, np.int32)
        _check(lib().orb_scene_median_depth(
            self._h, len(pi), _ptr(pi) if len(pi) else None, _ptr(pose),
            _ptr(pts) if len(pts) else None, len(pts), int(q), _ptr(med), _ptr(cnt)),
            "ComputeSceneMedianDepth")
        return med[0], int(cnt[0])

    def CreateNewMapPoints(self, kf1, kf2, match12, cam1, cam2, scale_factors, level_sigma2,
                           monocular, points, cursor, median_depth=float("nan"), status=None,
                           x3d=None, new_pairs=None):
        """The gate and loop body of LocalMapping::CreateNewMapPoints for one
        (current keyframe, neighbour) pair, host buffers.  kf1 / kf2: dicts with
        keys (KEYPOINT_DTYPE, mvKeysUn), u_right, depth (both None: monocular
        keyframe), point_index (int32, updated in place) and pose (POSE_DTYPE).
        points: a MAP_POINT_DTYPE array whose length is the capacity, updated in
        place from `cursor` on.  Returns (info record, the cursor after the call,
        status, x3d, new_pairs); the three arrays (given, or zero-filled) keep
        their value where the call writes nothing."""
        k1 = np.ascontiguousarray(kf1["keys"], KEYPOINT_DTYPE).reshape(-1)
        k2 = np.ascontiguousarray(kf2["keys"], KEYPOINT_DTYPE).reshape(-1)
        n1, n2 = len(k1), len(k2)
        stereo = kf1.get("u_right") is not None or kf2.get("u_right") is not None
        fa = lambda a, n: np.ascontiguousarray(
            a if a is not None else np.full(n, -1, np.float32), np.float32).reshape(-1)
        ur1, dp1 = fa(kf1.get("u_right"), n1), fa(kf1.get("depth"), n1)
        ur2, dp2 = fa(kf2.get("u_right"), n2), fa(kf2.get("depth"), n2)
        pi1, pi2 = kf1["point_index"], kf2["point_index"]
        for a, n in ((pi1, n1), (pi2, n2)):
            if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags.c_contiguous
                    and len(a) == n):
                raise OrbError(ORB_EINVAL, "point_index: a contiguous int32 array per keypoint")
        if not (isinstance(points, np.ndarray) and points.dtype == MAP_POINT_DTYPE
                and points.flags.c_contiguous):
            raise OrbError(ORB_EINVAL, "points: a contiguous MAP_POINT_DTYPE array")
        m12 = np.ascontiguousarray(match12, np.int32).reshape(-1)
        if len(m12) != n1:
            raise OrbError(ORB_EINVAL, "match12: one entry per keypoint of kf1")
        p1 = np.ascontiguousarray(kf1["pose"], POSE_DTYPE).reshape(1)
        p2 = np.ascontiguousarray(kf2["pose"], POSE_DTYPE).reshape(1)
        sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
        ls = np.ascontiguousarray(level_sigma2, np.float32).reshape(-1)
        if len(sf) != len(ls):
            raise OrbError(ORB_EINVAL, "scale_factors and level_sigma2 differ in length")
        status = np.zeros(n1, np.uint8) if status is None else status
        x3d = np.zeros((n1, 3), np.float32) if x3d is None else x3d
        new_pairs = np.zeros((n1, 2), np.int32) if new_pairs is None else new_pairs
        cur = np.array([cursor], np.int32)
        info = np.zeros(1, NEW_POINT_INFO_DTYPE)
        c1, c2 = self._camera(cam1), self._camera(cam2)
        q = lambda a, n: _ptr(a) if n else None
        _check(lib().orb_create_new_map_points(
            self._h, n1, q(k1, n1), q(ur1, n1 and stereo), q(dp1, n1 and stereo), q(pi1, n1),
            _ptr(p1), n2, q(k2, n2), q(ur2, n2 and stereo), q(dp2, n2 and stereo), q(pi2, n2),
            _ptr(p2), q(m12, n1), float(median_depth), ctypes.byref(c1), ctypes.byref(c2),
            _ptr(sf) if len(sf) else None, _ptr(ls) if len(ls) else None, len(sf),
            int(bool(monocular)), q(points, len(points)), len(points), _ptr(cur), q(status, n1),
            q(x3d, n1), q(new_pairs, n1), _ptr(info)), "CreateNewMapPoints")
        return info[0], int(cur[0]), status, x3d, new_pairs

    # ------------------------------------------ MapPoint::ComputeDistinctiveDescriptors
    def ComputeDistinctiveDescriptors(self, obs_offs, obs_desc, descriptors=None):
        """MapPoint::ComputeDistinctiveDescriptors for many points (src/MapPoint.cc:250-326).
        obs_offs (n_mp + 1) CSR offsets into obs_desc rows (observations in map
        order, bad KeyFrames dropped).  Returns (best_idx, descriptors): best_idx
        -1 for empty lists, whose descriptor rows keep their input value."""
        offs = np.ascontiguousarray(obs_offs, np.int32)
        od = np.ascontiguousarray(obs_desc, np.uint8).reshape(-1, 32)
        n = len(offs) - 1
        best = np.full(max(n, 0), -1, np.int32)
        out = (np.zeros((max(n, 0), 32), np.uint8) if descriptors is None
               else np.array(descriptors, np.uint8).reshape(n, 32))
        if n <= 0:
            return best, out
        _check(lib().orb_distinctive_descriptors(
            self._h, n, _ptr(offs), _ptr(od) if len(od) else None, _ptr(best), _ptr(out)),
            "ComputeDistinctiveDescriptors")
        return best, out

    def distinctive_descriptors_batch(self, n_mp, d_offs, d_desc, d_best, d_out=None,
                                      stream: int = 0):
        _check(lib().orb_distinctive_descriptors_batch(self._h, n_mp, d_offs, d_desc, d_best,
                                                       d_out, stream or None),
               "distinctive_descriptors_batch")


# ------------------------------------------------------------------ Sim3Solver
class Sim3Solver:
    """ORB_SLAM2::Sim3Solver for one (pKF1, pKF2, vpMatched12) problem on the
    device batch of one (include/Sim3Solver.h).  keys1 / keys2: KEYPOINT_DTYPE
    (mvKeysUn); point_index1: GetMapPointMatches() of pKF1 as indices into
    `points` (MAP_POINT_DTYPE; negative NULL); pose1 / pose2: POSE_DTYPE records;
    match12: the point index of vpMatched12[i1] or negative; index2:
    GetIndexInKeyFrame(pKF2) per i1; index1 optional.  draws: raw rand() values,
    three per iteration (uint32); the solver owns its draw stream."""

    def __init__(self, matcher: "ORBmatcher", keys1, point_index1, pose1, keys2, pose2, points,
                 match12, index2, level_sigma2, cam1, cam2, bFixScale: bool, draws,
                 index1=None, rand_max: int = 2147483647, probability: float = 0.99,
                 minInliers: int = 20, maxIterations: int = 300):
        import torch

        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        k1 = np.ascontiguousarray(keys1, KEYPOINT_DTYPE).reshape(-1)
        k2 = np.ascontiguousarray(keys2, KEYPOINT_DTYPE).reshape(-1)
        S = max(len(k1), len(k2), 1)
        if S > sim3_solver_max_stride():
            raise OrbError(ORB_ECAPACITY, "Sim3Solver")
        self._m, self._S, self.mN1 = matcher, S, len(k1)
        self._rand_max, self._max_its = int(rand_max), int(maxIterations)
        keys = np.zeros((2, S), KEYPOINT_DTYPE)
        keys[0, :len(k1)], keys[1, :len(k2)] = k1, k2
        pidx = np.full((2, S), -1, np.int32)
        pidx[0, :len(k1)] = np.asarray(point_index1, np.int32)[:len(k1)]
        pose = np.zeros(2, POSE_DTYPE)
        pose[0], pose[1] = pose1, pose2
        pad = lambda a: np.concatenate([np.asarray(a, np.int32).reshape(-1)[:S],
                                        np.full(max(S - len(a), 0), -1, np.int32)])
        d = np.ascontiguousarray(draws, np.uint32).reshape(-1)
        if len(d) < 3 * self._max_its:
            raise OrbError(ORB_EINVAL, "Sim3Solver: fewer than 3 * maxIterations draws")
        self._bufs = [dev(keys), dev(np.array([len(k1), len(k2)], np.int32)), dev(pidx), dev(pose),
                      dev(np.ascontiguousarray(points, MAP_POINT_DTYPE)), dev(pad(match12)),
                      dev(pad(index2)), dev(pad(index1)) if index1 is not None else None, dev(d),
                      dev(np.array([0, 1], np.int32))]
        self._state = torch.zeros(SIM3_STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        self._corr = torch.zeros(S * SIM3_CORR_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        self._inl = torch.zeros(S, dtype=torch.uint8, device="cuda")
        self._res = torch.zeros(SIM3_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        self._draw_stride = len(d)
        b = self._bufs
        # a stream of the solver's own, behind what the current stream has queued
        self._stream = torch.cuda.Stream()
        self._stream.wait_stream(torch.cuda.current_stream())
        stream = self._stream.cuda_stream
        matcher.sim3_solver_setup_batch(
            1, b[9].data_ptr(), b[9].data_ptr() + 4, b[0].data_ptr(), b[1].data_ptr(),
            b[2].data_ptr(), b[3].data_ptr(), S, b[4].data_ptr(), b[5].data_ptr(),
            b[7].data_ptr() if b[7] is not None else 0, b[6].data_ptr(), level_sigma2, cam1, cam2,
            bFixScale, self._state.data_ptr(), self._corr.data_ptr(), probability, minInliers,
            maxIterations, stream)

    def state(self):
        """The solver's members (SIM3_STATE_DTYPE record)."""
        self._stream.synchronize()
        return self._state.cpu().numpy().view(SIM3_STATE_DTYPE)[0]

    def iterate(self, nIterations: int):
        """(T12 (4 x 4) or None, bNoMore, vbInliers (mN1 bools), nInliers)."""
        self._m.sim3_solver_iterate_batch(
            1, self._S, self._state.data_ptr(), self._corr.data_ptr(), self._bufs[8].data_ptr(),
            self._draw_stride, nIterations, self._inl.data_ptr(), self._res.data_ptr(), 0,
            self._rand_max, self._max_its, self._stream.cuda_stream)
        self._stream.synchronize()
        r = self._res.cpu().numpy().view(SIM3_RESULT_DTYPE)[0]
        inl = self._inl.cpu().numpy()[:self.mN1].astype(bool)
        T = r["T12"].reshape(4, 4).copy() if r["has_sim3"] else None
        return T, bool(r["no_more"]), inl, int(r["n_inliers"])

    def find(self):
        """(T12 or None, vbInliers12, nInliers)."""
        T, _, inl, n = self.iterate(self._max_its)
        return T, inl, n

    def GetEstimatedRotation(self):
        return self.state()["best_R"].reshape(3, 3).copy()

    def GetEstimatedTranslation(self):
        return self.state()["best_t"].copy()

    def GetEstimatedScale(self) -> float:
        return float(self.state()["best_scale"])


# ------------------------------------------------------------------ vocabulary
class ORBVocabulary:
    """DBoW2 TemplatedVocabulary<FORB::TDescriptor, FORB> (include/ORBVocabulary.h),
    device-resident.  Built from a loadFromTextFile node table
    (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1362-1448) or a text file.
    Scoring / weighting codes as BowVector.h:36-53 (L1_NORM 0 ... DOT_PRODUCT 5;
    TF_IDF 0, TF 1, IDF 2, BINARY 3)."""

    def __init__(self, k: int, L: int, parent, leaf, descriptors, weights, scoring: int = 0,
                 weighting: int = 0, device: int = 0, _handle=None):
        if _handle is not None:
            self._h = _handle
        else:
            parent = np.ascontiguousarray(parent, np.int32)
            leaf = np.ascontiguousarray(leaf, np.uint8)
            desc = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
            w = np.ascontiguousarray(weights, np.float64)
            n = len(parent)
            if not (len(leaf) == n and len(desc) == n and len(w) == n):
                raise ValueError("vocabulary node table arrays differ in length")
            h = ctypes.c_void_p()
            _check(lib().orb_vocabulary_create(device, k, L, scoring, weighting, n, _ptr(parent),
                                               _ptr(leaf), _ptr(desc), _ptr(w), ctypes.byref(h)),
                   "orb_vocabulary_create")
            self._h = h
        info = np.zeros(6, np.int32)
        _check(lib().orb_vocabulary_info(self._h, _ptr(info)), "orb_vocabulary_info")
        self.k, self.L, self.scoring, self.weighting, self.n_nodes, self.n_words = map(int, info)

    @classmethod
    def loadFromTextFile(cls, path, device: int = 0) -> "ORBVocabulary":
        h = ctypes.c_void_p()
        _check(lib().orb_vocabulary_load_text(device, str(path).encode(), ctypes.byref(h)),
               "orb_vocabulary_load_text")
        return cls(0, 0, None, None, None, None, _handle=h)

    def close(self):
        if getattr(self, "_h", None):
            lib().orb_vocabulary_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self) -> int:
        return self.n_words

    def empty(self) -> bool:
        return self.n_words == 0

    @property
    def stream(self) -> int:
        return lib().orb_vocabulary_stream(self._h) or 0

    def transform(self, descriptors, levelsup: int = 4, per_feature: bool = False):
        """transform(features, BowVector&, FeatureVector&, levelsup) as called by
        Frame::ComputeBoW (src/Frame.cc:439-449).  Returns (bow_words, bow_values,
        feat_vec) with feat_vec = (node ids, CSR offsets, feature indices) in the
        layout ORBmatcher.SearchByBoW takes; with per_feature also (word per
        feature, 0xFFFFFFFF if stopped; FeatureVector node per feature)."""
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
        n = len(d)
        cap = max(n, 1)
        bw = np.zeros(cap, np.uint32)
        bv = np.zeros(cap, np.float64)
        fvn = np.zeros(cap, np.uint32)
        fvo = np.zeros(cap + 1, np.int32)
        fvf = np.zeros(cap, np.uint32)
        fw = np.zeros(cap, np.uint32) if per_feature else None
        fn = np.zeros(cap, np.uint32) if per_feature else None
        nw = ctypes.c_int(0)
        nf = ctypes.c_int(0)
        _check(lib().orb_vocabulary_transform(
            self._h, n, _ptr(d) if n else None, levelsup, _ptr(bw), _ptr(bv), ctypes.byref(nw),
            _ptr(fvn), _ptr(fvo), _ptr(fvf), ctypes.byref(nf),
            _ptr(fw) if per_feature else None, _ptr(fn) if per_feature else None), "transform")
        a, b = nw.value, nf.value
        fv = (fvn[:b], fvo[:b + 1], fvf[:fvo[b]])
        if per_feature:
            return bw[:a], bv[:a], fv, fw[:n], fn[:n]
        return bw[:a], bv[:a], fv

    def transform_batch(self, n_frames, d_counts, d_desc, stride, levelsup, d_feat_word,
                        d_feat_weight, d_feat_node, d_bow_words, d_bow_values, d_n_words,
                        d_fv_nodes, d_fv_offs, d_fv_feats, d_n_fv_nodes, stream: int = 0):
        """Device-resident batch form (raw device pointers, e.g. torch .data_ptr())."""
        _check(lib().orb_vocabulary_transform_batch(
            self._h, n_frames, d_counts, d_desc, stride, levelsup, d_feat_word, d_feat_weight,
            d_feat_node, d_bow_words, d_bow_values, d_n_words, d_fv_nodes, d_fv_offs, d_fv_feats,
            d_n_fv_nodes, stream or None), "transform_batch")

    def score_pairs(self, a_list, b_list) -> np.ndarray:
        """score(a_list[p], b_list[p]) for every pair: the reference's double
        (ScoringObject.cpp:23-311), bit for bit.  Each vector is a (words,
        values) pair as transform returns them (further tuple entries ignored)."""
        if len(a_list) != len(b_list):
            raise ValueError("score_pairs: lists differ in length")

        def csr(vs):
            offs = np.zeros(len(vs) + 1, np.int32)
            offs[1:] = np.cumsum([len(v[0]) for v in vs])
            w = np.concatenate([np.asarray(v[0], np.uint32) for v in vs] + [np.zeros(0, np.uint32)])
            x = np.concatenate([np.asarray(v[1], np.float64) for v in vs] + [np.zeros(0)])
            return offs, np.ascontiguousarray(w), np.ascontiguousarray(x)

        n = len(a_list)
        out = np.zeros(n, np.float64)
        ao, aw, av = csr(a_list)
        bo, bw, bv = csr(b_list)
        _check(lib().orb_vocabulary_score(self._h, n, _ptr(ao), _ptr(aw), _ptr(av), _ptr(bo),
                                          _ptr(bw), _ptr(bv), _ptr(out)), "orb_vocabulary_score")
        return out

    def score(self, a, b) -> float:
        """TemplatedVocabulary::score(a, b) with this vocabulary's scoring type."""
        return float(self.score_pairs([a], [b])[0])

    def score_batch(self, n_pairs, d_a_offs, d_a_words, d_a_values, d_b_offs, d_b_words,
                    d_b_values, d_out, stream: int = 0):
        """Device-pointer form of score_pairs (CSR offsets int32, asynchronous)."""
        _check(lib().orb_vocabulary_score_batch(self._h, n_pairs, d_a_offs, d_a_words, d_a_values,
                                                d_b_offs, d_b_words, d_b_values, d_out,
                                                stream or None), "orb_vocabulary_score_batch")


# ---------------------------------------------------------- keyframe database
class KeyFrameDatabase:
    """KeyFrameDatabase (src/KeyFrameDatabase.cc) over keyframe ids, resident on
    the device.  `bow` arguments are (words, values[, ...]) as
    ORBVocabulary.transform returns them.  The vocabulary must outlive it."""

    def __init__(self, voc: ORBVocabulary):
        self._voc = voc  # keeps the vocabulary alive
        h = ctypes.c_void_p()
        _check(lib().orb_kf_database_create(voc._h, ctypes.byref(h)), "orb_kf_database_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().orb_kf_database_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _bow(bow):
        w = np.ascontiguousarray(bow[0], np.uint32)
        v = np.ascontiguousarray(bow[1], np.float64)
        if len(w) != len(v):
            raise ValueError("BowVector words and values differ in length")
        return w, v

    def __len__(self) -> int:
        n = lib().orb_kf_database_size(self._h)
        if n < 0:
            raise OrbError(n, "orb_kf_database_size")
        return n

    def add(self, kf_id: int, bow):
        w, v = self._bow(bow)
        _check(lib().orb_kf_database_add(self._h, kf_id, len(w), _ptr(w), _ptr(v)),
               "orb_kf_database_add")

    def erase(self, kf_id: int):
        _check(lib().orb_kf_database_erase(self._h, kf_id), "orb_kf_database_erase")

    def clear(self):
        _check(lib().orb_kf_database_clear(self._h), "orb_kf_database_clear")

    def set_covisibility(self, kf_id: int, neighbour_ids):
        """Snapshot of GetBestCovisibilityKeyFrames(10) of keyframe kf_id."""
        nb = np.ascontiguousarray(neighbour_ids, np.int64)
        _check(lib().orb_kf_database_set_covisibility(self._h, kf_id, len(nb), _ptr(nb)),
               "orb_kf_database_set_covisibility")

    def _query(self, call, what):
        cap = max(len(self), 1)
        out = np.zeros(cap, np.int64)
        n = ctypes.c_int(0)
        _check(call(_ptr(out), cap, ctypes.byref(n)), what)
        return out[:n.value].copy()

    def DetectRelocalizationCandidates(self, query_id: int, bow) -> np.ndarray:
        """Candidate keyframe ids in the reference's order (:205-339)."""
        w, v = self._bow(bow)
        return self._query(lambda o, c, n: lib().orb_kf_database_detect_relocalization(
            self._h, query_id, len(w), _ptr(w), _ptr(v), o, c, n), "detect_relocalization")

    def DetectLoopCandidates(self, query_id: int, bow, connected_ids, min_score: float) -> np.ndarray:
        """Candidate keyframe ids in the reference's order (:79-202)."""
        w, v = self._bow(bow)
        cn = np.ascontiguousarray(connected_ids, np.int64)
        return self._query(lambda o, c, n: lib().orb_kf_database_detect_loop(
            self._h, query_id, len(w), _ptr(w), _ptr(v), len(cn), _ptr(cn), min_score, o, c, n),
            "detect_loop")

    def last_query(self):
        """lKFsSharingWords of the last query in list order: (ids, common word
        counts, scores as float32, scored flags)."""
        n = ctypes.c_int(0)
        st = lib().orb_kf_database_last_query(self._h, None, None, None, None, 0, ctypes.byref(n))
        if st not in (ORB_OK, ORB_ECAPACITY):
            raise OrbError(st, "orb_kf_database_last_query")
        cap = max(n.value, 1)
        ids = np.zeros(cap, np.int64)
        common = np.zeros(cap, np.int32)
        scores = np.zeros(cap, np.float32)
        scored = np.zeros(cap, np.uint8)
        _check(lib().orb_kf_database_last_query(self._h, _ptr(ids), _ptr(common), _ptr(scores),
                                                _ptr(scored), cap, ctypes.byref(n)),
               "orb_kf_database_last_query")
        k = n.value
        return ids[:k], common[:k], scores[:k], scored[:k]

    def profile(self, stage: int, reps: int):
        """Isolated time of one kernel of the last query: (total ms, kernel name)."""
        ms = ctypes.c_double(0)
        name = ctypes.c_char_p()
        _check(lib().orb_kf_database_profile(self._h, stage, reps, ctypes.byref(ms),
                                             ctypes.byref(name)), "orb_kf_database_profile")
        return ms.value, name.value.decode()
