"""ctypes binding of csrc/libnsc_hip.so (include/nsc.h).  No fallback: if the library is missing
or a call fails, this raises."""
import collections
import ctypes as C
import os
import threading

import torch  # noqa: F401  -- loads torch's libamdhip64 first so the library shares its HIP runtime

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libnsc_hip.so")


class NscError(RuntimeError):
    pass


class EncParams(C.Structure):
    """struct NscEncParams (include/nsc.h)"""
    _fields_ = [
        ("n_elevation", C.c_int32), ("n_azimuth", C.c_int32), ("n_bins", C.c_int32),
        ("target_rows", C.c_int32), ("elev_min_rad", C.c_double), ("elev_max_rad", C.c_double),
        ("min_range", C.c_float), ("max_range", C.c_float), ("epsilon", C.c_float),
        ("interpolate", C.c_int32), ("elev_f64", C.c_int32),
    ]


class GatLayer(C.Structure):
    """struct NscGatLayer"""
    _fields_ = [(n, C.c_void_p) for n in (
        "lin_w", "att_src", "att_dst", "lin_edge_w", "att_edge", "bias",
        "bn_w", "bn_b", "bn_mean", "bn_var")]


ABI_VERSION = 4            # NSC_ABI_VERSION of include/nsc.h
GAT_MAX_LAYERS = 8
GAT_MAX_EDGE_DIM = 8
# include/nsc.h: the ``flags`` of nsc_gat_forward_ex, by the value of SpectralGNN.coresident that selects them
GAT_KERNEL_SETS = {
    False: 0,            # the stand-alone forward (LDS-DMA GEMMs, one-launch layers on a banded graph)
    True: 1,             # NSC_GAT_CORESIDENT
    "shared_b": 1 | 2,   # NSC_GAT_CORESIDENT | NSC_GAT_SHARED_B
    "lds_tiled": 4,      # NSC_GAT_LDS_TILED
    "generic": 8,        # NSC_GAT_GENERIC
}


class GatModel(C.Structure):
    """struct NscGatModel"""
    _fields_ = [
        ("in_dim", C.c_int32), ("hidden", C.c_int32), ("out_dim", C.c_int32), ("n_layers", C.c_int32),
        ("edge_dim", C.c_int32), ("residual", C.c_int32), ("bn_eps", C.c_float),
        ("negative_slope", C.c_float),
        ("in_w", C.c_void_p), ("in_b", C.c_void_p),
        ("in_bn_w", C.c_void_p), ("in_bn_b", C.c_void_p), ("in_bn_mean", C.c_void_p), ("in_bn_var", C.c_void_p),
        ("out_w", C.c_void_p), ("out_b", C.c_void_p), ("res_w", C.c_void_p), ("res_b", C.c_void_p),
        ("folded", C.c_void_p),
        ("layers", GatLayer * GAT_MAX_LAYERS),
    ]


class Graph(C.Structure):
    """struct NscGraph"""
    _fields_ = [("n_nodes", C.c_int32), ("nnz", C.c_int32), ("row_ptr", C.c_void_p),
                ("src", C.c_void_p), ("eid", C.c_void_p), ("loop_attr", C.c_void_p),
                ("t_ptr", C.c_void_p), ("t_entry", C.c_void_p), ("tgt", C.c_void_p),
                ("band_entries", C.c_void_p), ("band", C.c_int32)]


class GatTrainCfg(C.Structure):
    """struct NscGatTrainCfg"""
    _fields_ = [("dropout_p", C.c_float), ("bn_momentum", C.c_float), ("seed", C.c_uint64),
                ("update_running_stats", C.c_int32), ("accumulate_grads", C.c_int32), ("seed_dev", C.c_void_p)]


class MineParams(C.Structure):
    """struct NscMineParams"""
    _fields_ = [("positive_distance_max", C.c_double), ("negative_distance_min", C.c_double),
                ("negative_distance_max", C.c_double), ("positive_temporal_min", C.c_int32),
                ("negative_temporal_min", C.c_int32), ("strategy", C.c_int32),
                ("triplets_per_anchor", C.c_int32), ("seed", C.c_uint64)]


class GicpParams(C.Structure):
    """struct NscGicpParams"""
    _fields_ = [("voxel_size", C.c_double), ("max_correspondence_distance", C.c_double),
                ("relative_fitness", C.c_double), ("relative_rmse", C.c_double), ("epsilon", C.c_double),
                ("max_iteration", C.c_int32), ("covariance_knn", C.c_int32)]


class GicpStages(C.Structure):
    """struct NscGicpStages"""
    _fields_ = [(n, C.c_void_p) for n in ("points", "counts", "covariances", "system0")]


class GicpCloudSet(C.Structure):
    """struct NscGicpCloudSet"""
    _fields_ = [("voxel_size", C.c_double), ("epsilon", C.c_double), ("covariance_knn", C.c_int32),
                ("n_clouds", C.c_int32), ("n_rows", C.c_int64), ("n_slots", C.c_int64), ("cap_clouds", C.c_int64),
                ("cap_rows", C.c_int64), ("cap_slots", C.c_int64)] + [
        (n, C.c_void_p) for n in ("row_offsets", "slot_offsets", "bounds", "points", "covariances", "slots")]


class PlanarParams(C.Structure):
    """struct NscPlanarParams"""
    _fields_ = [("cell", C.c_double), ("z_window", C.c_double), ("normal_z2_max", C.c_double),
                ("half_bins", C.c_int32), ("source_stride", C.c_int32), ("guard", C.c_int32)]


class PlanarStages(C.Structure):
    """struct NscPlanarStages"""
    _fields_ = [(n, C.c_void_p) for n in ("yaw_peaks", "votes")]


class PoseGraphParams(C.Structure):
    """struct NscPoseGraphParams"""
    _fields_ = [("max_iteration", C.c_int32), ("max_pcg_iterations", C.c_int32), ("pcg_tolerance", C.c_double),
                ("lambda0", C.c_double), ("lambda_min", C.c_double), ("lambda_factor", C.c_double),
                ("relative_cost", C.c_double), ("min_step", C.c_double)]


class MapParams(C.Structure):
    """struct NscMapParams"""
    _fields_ = [("voxel_size", C.c_double), ("origin", C.c_double * 3)]


class MapDistParams(C.Structure):
    """struct NscMapDistParams"""
    _fields_ = [("min_points", C.c_int32), ("reserved", C.c_int32), ("eigen_ratio", C.c_double),
                ("sigma_floor", C.c_double)]


class MapRegisterParams(C.Structure):
    """struct NscMapRegisterParams"""
    _fields_ = [("max_iteration", C.c_int32), ("reserved", C.c_int32), ("relative_fitness", C.c_double),
                ("relative_rmse", C.c_double)]


class MapRobustParams(C.Structure):
    """struct NscMapRobustParams"""
    _fields_ = [("kernel", C.c_int32), ("neighbours", C.c_int32), ("scale", C.c_double)]


class MapRayParams(C.Structure):
    """struct NscMapRayParams"""
    _fields_ = [("min_range", C.c_double), ("max_range", C.c_double), ("end_margin", C.c_double), ("gate", C.c_double)]


# include/nsc.h NSC_MAP_DTYPE_F32, NSC_MAP_DTYPE_F64, NSC_MAP_STATS and NSC_MAP_STAT_*: the name of each entry of `stats`
MAP_DTYPE_F32, MAP_DTYPE_F64, MAP_STATS = 0, 1, 7
MAP_STAT_NAMES = ("voxels_found", "voxels_written", "rows_used", "rows_not_finite", "rows_outside", "rows_without_pose",
                  "rows_unplaced")
# include/nsc.h NSC_MAP_TILE_ROWS, NSC_MAP_SCAN_THREADS, NSC_MAP_INSERT_ROWS, NSC_MAP_INSERT_BLOCKS
MAP_TILE_ROWS, MAP_SCAN_THREADS, MAP_INSERT_ROWS, MAP_INSERT_BLOCKS = 4096, 256, 512, 2048
MAP_MAX_VOXELS, MAP_MAX_ROWS = 1 << 36, 1 << 46     # include/nsc.h NSC_MAP_MAX_VOXELS, NSC_MAP_MAX_ROWS
# include/nsc.h NSC_MAP_VOXEL_DOUBLES, NSC_MAP_REGISTER_BLOCKS, NSC_MAP_REGISTER_SYSTEM, NSC_MAP_REGISTER_MAX_SCANS
MAP_VOXEL_DOUBLES, MAP_REGISTER_BLOCKS, MAP_REGISTER_SYSTEM, MAP_REGISTER_MAX_SCANS = 16, 64, 30, 65535
MAP_INSERT_LAUNCHES = 8                 # include/nsc.h NSC_MAP_INSERT_LAUNCHES
MAP_REMOVE_LAUNCHES, MAP_REPLACE_LAUNCHES = 3, 10      # include/nsc.h NSC_MAP_REMOVE_LAUNCHES, NSC_MAP_REPLACE_LAUNCHES
# include/nsc.h NSC_MAP_REMOVE_STATS and NSC_MAP_REMOVE_STAT_*: the name of each entry of `removed`
MAP_REMOVE_STATS = 8
MAP_REMOVE_STAT_NAMES = ("rows_removed", "removed_not_finite", "removed_outside", "removed_without_pose", "rows_missing",
                         "voxels_touched", "voxels_emptied", "voxels_inconsistent")
# include/nsc.h NSC_MAP_REHASH_LAUNCHES, NSC_MAP_REHASH_STATS and NSC_MAP_REHASH_STAT_*: the name of each entry of `rehashed`
MAP_REHASH_LAUNCHES, MAP_REHASH_STATS = 4, 6
MAP_REHASH_STAT_NAMES = ("voxels_kept", "voxels_dropped", "source_keys_unplaced", "inconsistent_kept", "kept_unplaced",
                         "kept_table_full")
MAP_REGISTER_ROBUST_SYSTEM = 32         # include/nsc.h NSC_MAP_REGISTER_ROBUST_SYSTEM
# include/nsc.h NSC_MAP_KERNEL_*: the pose graph's names and numbers
MAP_KERNELS = {None: 0, "huber": 1, "cauchy": 2, "geman_mcclure": 3}
# include/nsc.h NSC_MAP_RAY_LAUNCHES, NSC_MAP_FLAG_LAUNCHES, NSC_MAP_RAY_MAX_REACH, NSC_MAP_RAY_STATS and NSC_MAP_RAY_STAT_*,
# NSC_MAP_FLAG_STATS and NSC_MAP_FLAG_STAT_*: the name of each entry of `ray_stats` and of `flag_stats`
MAP_RAY_LAUNCHES, MAP_FLAG_LAUNCHES, MAP_RAY_MAX_REACH, MAP_RAY_STATS, MAP_FLAG_STATS = 2, 2, 65536, 8, 4
MAP_RAY_STAT_NAMES = ("rays_cast", "rays_not_finite", "rays_outside", "rays_without_pose", "rays_short", "voxels_visited",
                      "crossings", "rays_truncated")
MAP_FLAG_STAT_NAMES = ("rows_flagged", "rows_kept", "rows_dropped", "rows_without_voxel")

# include/nsc.h NSC_POSEGRAPH_MAX_EDGES, NSC_POSEGRAPH_MAX_LAUNCHES, NSC_POSEGRAPH_STATS
POSEGRAPH_MAX_EDGES, POSEGRAPH_MAX_LAUNCHES, POSEGRAPH_STATS = 1073741823, 1000000, 10
POSEGRAPH_MAX_AGGREGATES = 128                   # include/nsc.h NSC_POSEGRAPH_MAX_AGGREGATES
# include/nsc.h NSC_POSEGRAPH_STAT_*: where each statistic stands in `stats`
(POSEGRAPH_STAT_ITERATIONS, POSEGRAPH_STAT_ACCEPTED, POSEGRAPH_STAT_REJECTED, POSEGRAPH_STAT_PCG_ITERATIONS,
 POSEGRAPH_STAT_INITIAL_COST, POSEGRAPH_STAT_FINAL_COST, POSEGRAPH_STAT_LAMBDA, POSEGRAPH_STAT_SKIPPED,
 POSEGRAPH_STAT_CONVERGED, POSEGRAPH_STAT_STEP) = range(POSEGRAPH_STATS)
# include/nsc.h NSC_POSEGRAPH_KERNEL_*
POSEGRAPH_KERNELS = {None: 0, "huber": 1, "cauchy": 2, "geman_mcclure": 3}
# include/nsc.h NSC_POSEGRAPH_MAX_COV_NODES, NSC_POSEGRAPH_COV_TILE, NSC_POSEGRAPH_COV_STATS and NSC_POSEGRAPH_COV_STAT_*
POSEGRAPH_MAX_COV_NODES, POSEGRAPH_COV_TILE, POSEGRAPH_COV_STATS = 64, 16, 4
POSEGRAPH_COV_STAT_NAMES = ("skipped", "outside", "not_free", "not_converged")

GICP_MAX_KNN = 32
# include/nsc.h NSC_GICP_MAX_PAIRS, NSC_GICP_MAX_CLOUDS, NSC_GICP_MAX_PREPARED_PAIRS: the largest batch of one call
GICP_MAX_PAIRS, GICP_MAX_CLOUDS, GICP_MAX_PREPARED_PAIRS = 32767, 65535, 65535
# include/nsc.h NSC_YAW_GUARD_BINS, NSC_YAW_MAX_PAIRS
YAW_GUARD_BINS, YAW_MAX_PAIRS = 10, 4194304
# include/nsc.h NSC_PLANAR_MAX_HALF_BINS, NSC_PLANAR_MAX_PAIRS
PLANAR_MAX_HALF_BINS, PLANAR_MAX_PAIRS = 32, 65535


class GatGradLayer(C.Structure):
    """struct NscGatGradLayer"""
    _fields_ = [(n, C.c_void_p) for n in (
        "lin_w", "att_src", "att_dst", "lin_edge_w", "att_edge", "bias", "bn_w", "bn_b")]


class GatGrads(C.Structure):
    """struct NscGatGrads"""
    _fields_ = [(n, C.c_void_p) for n in ("in_w", "in_b", "in_bn_w", "in_bn_b", "out_w", "out_b", "x",
                                          "res_w", "res_b")] + [
        ("layers", GatGradLayer * GAT_MAX_LAYERS)]


_lib = None

# every symbol include/nsc.h declares: (restype, argtypes)
_vp, _i32, _i64, _sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
_pp = C.POINTER(EncParams)
SYMBOLS = {
    "nsc_abi_version": (C.c_int, []),
    "nsc_status_string": (C.c_char_p, [C.c_int]),
    "nsc_enc_default_params": (None, [_pp]),
    "nsc_encode_clouds_workspace_bytes": (_sz, [_i32, _i64, _pp]),
    "nsc_encode_clouds_path": (C.c_int, [_i32, _i64, _i32, _pp]),
    "nsc_encode_clouds": (C.c_int, [_vp, _vp, _i32, _i64, _i32, _pp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "nsc_project_intensity": (C.c_int, [_vp, _vp, _i32, _i64, _pp, _vp, _vp, _vp]),
    "nsc_scatter_clouds": (C.c_int, [_vp, _vp, _i32, _i64, _i32, _pp, _vp, _vp]),
    "nsc_finish_images": (C.c_int, [_vp, _i32, _pp, _vp, _vp, _vp, _vp, _vp]),
    "nsc_interpolate_range_images": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp]),
    "nsc_interpolate_range_images_ex": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _vp, _vp]),
    "nsc_encode_range_images": (C.c_int, [_vp, _i32, _i32, _pp, _vp, _vp, _vp]),
    "nsc_graph_workspace_bytes": (_sz, [_i32, _i64]),
    "nsc_graph_build_csr": (C.c_int, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "nsc_graph_band_entries": (C.c_int, [C.POINTER(Graph), _vp, _i32, _vp, _vp, _vp]),
    "nsc_gat_folded_floats": (_sz, [C.POINTER(GatModel)]),
    "nsc_gat_fold_weights": (C.c_int, [C.POINTER(GatModel), _vp, _vp]),
    "nsc_gat_workspace_bytes": (_sz, [C.POINTER(GatModel), _i32]),
    "nsc_gat_forward": (C.c_int, [C.POINTER(GatModel), C.POINTER(Graph), _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "nsc_gat_forward_ex": (C.c_int, [C.POINTER(GatModel), C.POINTER(Graph), _vp, _vp, _vp, _vp, _vp, _sz, C.c_uint32,
                                     _vp]),
    "nsc_gat_gemm_tile": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "nsc_graph_transpose_workspace_bytes": (_sz, [_i32]),
    "nsc_graph_transpose": (C.c_int, [C.POINTER(Graph), _vp, _vp, _vp, _vp, _sz, _vp]),
    "nsc_gat_train_workspace_bytes": (_sz, [C.POINTER(GatModel), C.POINTER(Graph)]),
    "nsc_gat_forward_train": (C.c_int, [C.POINTER(GatModel), C.POINTER(Graph), _vp, _vp, C.POINTER(GatTrainCfg),
                                        _vp, _vp, _sz, _vp]),
    "nsc_gat_backward": (C.c_int, [C.POINTER(GatModel), C.POINTER(Graph), _vp, _vp, C.POINTER(GatTrainCfg), _vp,
                                   C.POINTER(GatGrads), _vp, _sz, _vp]),
    "nsc_w1_cdf": (C.c_int, [_vp, _i32, _i32, C.c_float, _i32, _vp, _vp]),
    "nsc_w1_distances": (C.c_int, [_vp, _i32, _i32, C.c_float, _vp, _i32, _vp, _vp, C.c_float, _vp, _vp]),
    "nsc_w1_distances_cdf": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _vp, _vp, C.c_float, _vp, _vp]),
    "nsc_w1q_cdf": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp]),
    "nsc_w1q_distances": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp, C.c_float, _vp, _vp]),
    "nsc_revisit_queries": (C.c_int, [_vp, _i32, _i32, C.c_double, _vp, _vp]),
    "nsc_pairwise_l2": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "nsc_recall_rank": (C.c_int, [_vp, _vp, _vp, _i32, _i32, C.c_double, _vp, _vp]),
    "nsc_mine_triplets": (C.c_int, [_vp, _vp, _i32, _i32, C.POINTER(MineParams), _vp, _vp, _vp, _vp]),
    "nsc_mine_workspace_bytes": (_sz, [_i32, _i32]),
    "nsc_mine_triplets_ws": (C.c_int, [_vp, _vp, _i32, _i32, C.POINTER(MineParams), _vp, _vp, _vp, _vp, _sz, _vp]),
    "nsc_topk_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "nsc_topk_smallest": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "nsc_chain_graph_num_edges": (_i64, [_i32, _i32, _i32]),
    "nsc_build_chain_graph": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "nsc_quantize_descriptors": (C.c_int, [_vp, _i32, _i32, C.c_float, _vp, _vp]),
    "nsc_dequantize_descriptors": (C.c_int, [_vp, _i32, _i32, C.c_float, _vp, _vp]),
    "nsc_record_bytes": (_sz, [_i32]),
    "nsc_pack_records": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "nsc_unpack_records": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "nsc_voxel_overlap_workspace_bytes": (_sz, [_i64, _i64]),
    "nsc_voxel_overlap": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _vp, C.c_double, _vp, _vp,
                                    _vp, _sz, _vp]),
    "nsc_gicp_default_params": (None, [C.POINTER(GicpParams)]),
    "nsc_gicp_workspace_bytes": (_sz, [_i32, _i64, _i64]),
    "nsc_gicp_register": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i64, _i64, _i32, C.POINTER(GicpParams), _vp, _vp,
                                    _vp, _vp, _vp, C.POINTER(GicpStages), _vp, _sz, _vp]),
    "nsc_gicp_prepare_workspace_bytes": (_sz, [_i32, _i64]),
    "nsc_gicp_prepare": (C.c_int, [_vp, _vp, _i32, _i64, _i32, C.POINTER(GicpParams), C.POINTER(GicpCloudSet), _vp,
                                   _sz, _vp]),
    "nsc_gicp_register_prepared_workspace_bytes": (_sz, [_i32]),
    "nsc_gicp_register_prepared": (C.c_int, [C.POINTER(GicpCloudSet), C.POINTER(GicpCloudSet), _vp, _vp, _i32,
                                             C.POINTER(GicpParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "nsc_yaw_align": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "nsc_planar_default_params": (None, [C.POINTER(PlanarParams)]),
    "nsc_planar_align_workspace_bytes": (_sz, [_i32, _i32]),
    "nsc_planar_align": (C.c_int, [C.POINTER(GicpCloudSet), C.POINTER(GicpCloudSet), _vp, _vp, _i32, _vp, _i32,
                                   C.POINTER(PlanarParams), _vp, _vp, _vp, _vp, C.POINTER(PlanarStages), _vp, _sz,
                                   _vp]),
    "nsc_posegraph_default_params": (None, [C.POINTER(PoseGraphParams)]),
    "nsc_posegraph_workspace_bytes": (_sz, [_i32, _i32, C.POINTER(PoseGraphParams)]),
    "nsc_posegraph_linearize": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "nsc_posegraph_optimize": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _vp, C.POINTER(PoseGraphParams), _vp, _vp,
                                         _vp, _vp, _vp, _sz, _vp]),
    "nsc_posegraph_linearize_robust": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                                 _vp, _i32, _vp, _vp]),
    "nsc_posegraph_optimize_robust": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _vp, C.POINTER(PoseGraphParams), _vp,
                                                _vp, _vp, _vp, _vp, _sz, _vp, _i32, _vp, _vp, _vp]),
    "nsc_posegraph_coarse_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "nsc_posegraph_optimize_coarse": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _vp, C.POINTER(PoseGraphParams), _vp,
                                                _vp, _vp, _vp, _vp, _sz, _vp, _i32, _vp, _vp, _vp, _i32, _vp]),
    "nsc_posegraph_covariance_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "nsc_posegraph_covariance": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _vp, C.POINTER(PoseGraphParams), _vp, _i32,
                                           _vp, _vp, _vp, _vp, _vp, _sz, _vp, _i32, _vp, _i32, _vp]),
    "nsc_map_default_params": (None, [C.POINTER(MapParams)]),
    "nsc_map_workspace_bytes": (_sz, [_i64, _i64]),
    "nsc_map_build": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i64, _vp, _i32, _vp, C.POINTER(MapParams), _i64, _vp, _vp,
                                _vp, _vp, _vp, _sz, _vp]),
    "nsc_map_dist_default_params": (None, [C.POINTER(MapDistParams)]),
    "nsc_map_dist_workspace_bytes": (_sz, [_i64, _i64]),
    "nsc_map_build_dist": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i64, _vp, _i32, _vp, C.POINTER(MapParams),
                                     C.POINTER(MapDistParams), _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "nsc_map_insert_workspace_bytes": (_sz, [_i64]),
    "nsc_map_insert_dist": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i64, _vp, _i32, _vp, C.POINTER(MapParams),
                                      C.POINTER(MapDistParams), _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "nsc_map_remove_workspace_bytes": (_sz, [_i64]),
    "nsc_map_replace_workspace_bytes": (_sz, [_i64]),
    "nsc_map_remove_dist": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i64, _vp, _i32, _vp, C.POINTER(MapParams),
                                      C.POINTER(MapDistParams), _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "nsc_map_replace_dist": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i64, _vp, _vp, _i32, _vp, C.POINTER(MapParams),
                                       C.POINTER(MapDistParams), _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp,
                                       _vp, _sz, _vp]),
    "nsc_map_rehash_dist": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                      _vp, _vp, _vp, _vp]),
    "nsc_map_register_default_params": (None, [C.POINTER(MapRegisterParams)]),
    "nsc_map_register_workspace_bytes": (_sz, [_i32]),
    "nsc_map_register": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i64, _vp, _vp, _i64, C.POINTER(MapParams),
                                   C.POINTER(MapRegisterParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "nsc_map_robust_default_params": (None, [C.POINTER(MapRobustParams)]),
    "nsc_map_register_robust_workspace_bytes": (_sz, [_i32]),
    "nsc_map_register_robust": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i64, _vp, _vp, _i64, C.POINTER(MapParams),
                                          C.POINTER(MapRegisterParams), C.POINTER(MapRobustParams), _vp, _vp, _vp, _vp,
                                          _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "nsc_map_ray_default_params": (None, [C.POINTER(MapRayParams)]),
    "nsc_map_cast_rays": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i64, _vp, _i32, _vp, C.POINTER(MapParams), _vp, _vp, _i64,
                                    C.POINTER(MapRayParams), _vp, _vp, _vp]),
    "nsc_map_flag_rows": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i64, _vp, _i32, _vp, C.POINTER(MapParams), _vp, _vp, _vp,
                                    _i64, _i64, C.c_double, _vp, _vp, _vp]),
    "nsc_triplet_workspace_bytes": (_sz, [_i32]),
    "nsc_triplet_loss": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, C.c_float, C.c_float, _vp, _vp, _vp,
                                   _sz, _vp]),
}


# include/nsc_debug.h: diagnostics outside the product ABI, bound when the library exports them (nsc_debug_burn: development
# builds only)
DEBUG_SYMBOLS = {
    "nsc_debug_point_bins": (C.c_int, [_vp, _i64, _i32, _pp, _vp, _vp, _vp]),
    "nsc_debug_burn": (C.c_int, [_i32, _i32, _i32, _vp, _sz, _vp]),
}


def lib():
    """Load the HIP library (once).  Raises NscError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NscError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in DEBUG_SYMBOLS.items():
            fn = getattr(L, name, None)
            if fn is not None:
                fn.restype = res
                fn.argtypes = args
        if L.nsc_abi_version() != ABI_VERSION:
            raise NscError("libnsc_hip.so ABI version mismatch")
        _lib = L
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().nsc_status_string(status).decode()
        raise NscError(f"{what} failed: {msg} (status {status})")


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


STREAM = object()      # in call()'s arguments: where the hipStream_t goes (not always last: nsc_posegraph_*_robust)


def call(name, device, *args):
    """The one way into a launching ABI function: ``name`` runs with ``device`` current, on its current stream, and a
    non-zero status raises NscError("<name> failed: ...").  Tensors become device pointers, None a null pointer, ctypes
    structures go by reference, STREAM is replaced by the stream; anything else (numbers, ready-made pointers) passes as it
    is.  ``*_workspace_bytes`` and ``*_default_params`` launch nothing and are called directly."""
    fn = getattr(lib(), name)
    with torch.cuda.device(device):
        conv = [C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else stream_ptr(device) if a is STREAM
                else C.byref(a) if isinstance(a, C.Structure) else a for a in args]
        status = fn(*conv)
    check(status, name)


def capture(device, fn, stream=None):
    """Record the launches of ``fn()`` as a hipGraph (on ``stream``, or on torch's capture stream) and return
    (CUDAGraph, fn's result): nothing has run yet, ``replay()`` runs it.  Run ``fn`` once eagerly beforehand, so that no lazy
    set-up is recorded.  Thread-local error mode: HIP calls of OTHER threads (RCCL's proxy / watchdog) do not invalidate the
    capture.  What to do when this raises, and how long to keep the graph, is the caller's policy."""
    torch.cuda.synchronize(device)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg, stream=stream, capture_error_mode="thread_local"):
        result = fn()
    return cg, result


# Parameter epoch: bumped after every optimizer step of the process.  torch's fused Adam / AdamW / SGD write the parameters
# without bumping their version counters, so caches derived from parameter VALUES (the GNN's folded attention vectors, the
# encoder's bin LUT) carry this integer in their keys next to (data_ptr, _version).  Writes through ``.data`` bypass both.
param_epoch = 0


def _bump_param_epoch(optimizer, args, kwargs):
    global param_epoch
    param_epoch += 1


from torch.optim.optimizer import register_optimizer_step_post_hook  # noqa: E402

register_optimizer_step_post_hook(_bump_param_epoch)


def require_cuda(t, name):
    if not t.is_cuda:
        raise NscError(f"{name} must live on a HIP device (got {t.device}); the MI355X path has no "
                       "CPU fallback -- move the module/tensors to 'cuda'")


class ScratchCache:
    """Device scratch buffers of the Python layer (CSR build, GNN forward workspace, split encoder), one set per
    (device, stream, host thread, use): work on different streams may overlap and two host threads issuing on one stream
    interleave their launches, work issued by one thread on one stream is ordered.

    Bounded: at most ``cap`` keys, least recently used first, keys of host threads that no longer exist before
    any other.  A buffer is NEVER replaced by a bigger one -- a larger request adds a buffer to the key and the smaller
    ones stay, because a captured hipGraph replays the address it recorded; keys touched while a stream capture is open
    are pinned until ``release()`` (a replay does not come through here, so use-recency says nothing about them)."""

    def __init__(self, cap: int = 48):
        self.cap = cap
        self._lock = threading.Lock()
        self._d = collections.OrderedDict()          # key -> [pinned, [tensors, ascending size]]

    def get(self, device, nbytes: int, tag: str = ""):
        key = (str(device), torch.cuda.current_stream(device).cuda_stream, threading.get_ident(), tag)
        capturing = torch.cuda.is_current_stream_capturing()
        with self._lock:
            ent = self._d.get(key)
            if ent is None:
                ent = self._d[key] = [False, []]
            else:
                self._d.move_to_end(key)
            ent[0] = ent[0] or capturing
            for t in ent[1]:
                if t.numel() >= nbytes:
                    return t
            big = ent[1][-1].numel() if ent[1] else 0
            t = torch.empty(max(int(nbytes), 256, 2 * big if big else 0), dtype=torch.uint8, device=device)
            ent[1].append(t)
            if len(self._d) > self.cap:
                self._prune()
            return t

    def _prune(self):
        alive = {th.ident for th in threading.enumerate()}
        for dead_first in (True, False):
            for k in list(self._d):
                if len(self._d) <= self.cap:
                    return
                pinned = self._d[k][0]
                if pinned or (dead_first and k[2] in alive):
                    continue
                del self._d[k]

    def release(self, device=None):
        """Drop every buffer (of ``device``), pinned ones included: call when no captured hipGraph that ran through this
        cache will be replayed any more (e.g. after tearing down a ShardedDescriptorPath / GNNTrainer)."""
        with self._lock:
            for k in list(self._d):
                if device is None or k[0] == str(device):
                    del self._d[k]

    def __len__(self):
        return len(self._d)


scratch = ScratchCache()
