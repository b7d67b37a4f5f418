"""Mirror of the reference's ``retrieval`` package: stage-1 (Wasserstein) retrieval and stage-2 (GICP) verification."""
from .geometric_verification import GeometricVerifier, PreparedClouds, register_batch, register_prepared
from .two_stage_retrieval import (LoopClosureCandidate, ShardedTwoStageRetrieval, TwoStageRetrieval,
                                  batch_loop_closing, create_two_stage_retrieval)
from .yaw_alignment import YawImages, estimate_yaw
from .planar_alignment import estimate_planar, planar_info, yaw_table
from .pose_graph import (PoseGraphOptimizer, closure_edges, closure_mahalanobis, information_from_g2o,
                         information_to_g2o, odometry_edges, relative_covariance)
from .global_map import GlobalMap, revisited
from .map_localization import MapLocalizer
from .compressed import CompressedRetriever, quantized_cdf, w1_distances_quantized
from .wasserstein import (WassersteinRetriever, wasserstein_distance_1d_numpy, wasserstein_distance_1d_torch,
                          wasserstein_distance_batch_numpy, wasserstein_distance_batch_torch,
                          wasserstein_distance_matrix_numpy, wasserstein_distance_matrix_torch)

__all__ = ["CompressedRetriever", "quantized_cdf", "w1_distances_quantized", "GeometricVerifier", "PreparedClouds", "register_batch", "register_prepared", "YawImages", "estimate_yaw",
           "estimate_planar", "planar_info", "yaw_table",
           "PoseGraphOptimizer", "closure_edges", "closure_mahalanobis", "information_from_g2o", "information_to_g2o",
           "odometry_edges", "relative_covariance", "GlobalMap", "revisited", "MapLocalizer",
           "LoopClosureCandidate", "ShardedTwoStageRetrieval", "TwoStageRetrieval", "batch_loop_closing",
           "create_two_stage_retrieval", "WassersteinRetriever", "wasserstein_distance_1d_numpy", "wasserstein_distance_1d_torch",
           "wasserstein_distance_batch_numpy", "wasserstein_distance_batch_torch",
           "wasserstein_distance_matrix_numpy", "wasserstein_distance_matrix_torch"]
