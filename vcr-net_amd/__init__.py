"""vcr-net_amd: MI355X-native implementation of the VCR-Net registration hot path.

Only what the path needs lives here: ``csrc/`` (hand-written HIP kernels for gfx950
behind the C-ABI of ``include/vcr_hip.h``), ``native`` (ctypes binding of that ABI),
``module`` (the host-side mirror of the reference's ``VCRNet`` nn.Module contract),
``weights`` / ``synth`` (parameter inventory, deterministic weights, synthetic pairs),
``shard`` (process-per-GPU batch sharding) and ``evalmetrics`` (the reference's eval arithmetic).

The directory name carries a hyphen; import it as ``vcrnet_amd`` (see ``vcrnet_amd.py`` at
the repository root).
"""
from . import weights, synth  # noqa: F401

__all__ = ["weights", "synth", "farthest_point_sample", "register_sampled", "score_registration", "refine_registration",
           "estimate_normals", "voxel_down_sample", "remove_statistical_outlier", "remove_radius_outlier", "compute_fpfh_feature",
           "match_features", "ransac_correspondences", "register_features", "fast_global_registration", "centred",
           "uncentred_pose", "search_knn", "search_radius", "cluster_dbscan", "largest_cluster", "segment_plane",
           "split_by_plane", "segment_planes", "orient_normals_consistent_tangent_plane", "compute_iss_keypoints",
           "model_resolution", "compute_point_cloud_distance", "compute_color_gradient", "refine_registration_colored",
           "refine_registration_robust", "information_matrix", "optimize_pose_graph", "pose_graph_from_clouds",
           "register_multiway", "compute_boundary_points", "smooth_mls", "consistency_registration",
           "correspondence_consistency", "prune_correspondences", "ndt_map", "ndt_derivatives", "refine_registration_ndt",
           "coherent_point_drift", "cpd_expectation"]


def __getattr__(name):
    # resolved on first use: native / module load the HIP library's bindings, which `import vcrnet_amd` alone does not need
    if name == "farthest_point_sample":
        from .native import farthest_point_sample
        return farthest_point_sample
    if name == "register_sampled":
        from .module import register_sampled
        return register_sampled
    if name == "score_registration":
        from .score import score_registration
        return score_registration
    if name == "refine_registration":
        from .refine import refine_registration
        return refine_registration
    if name == "estimate_normals":
        from .plane import estimate_normals
        return estimate_normals
    if name == "voxel_down_sample":
        from .voxel import voxel_down_sample
        return voxel_down_sample
    if name in ("remove_statistical_outlier", "remove_radius_outlier"):
        from . import outlier
        return getattr(outlier, name)
    if name == "compute_fpfh_feature":
        from .fpfh import compute_fpfh_feature
        return compute_fpfh_feature
    if name in ("match_features", "ransac_correspondences", "register_features"):
        from . import match
        return getattr(match, name)
    if name == "fast_global_registration":
        from .fgr import fast_global_registration
        return fast_global_registration
    if name == "search_knn":
        from .grid import search_knn
        return search_knn
    if name == "search_radius":
        from .radius import search_radius
        return search_radius
    if name in ("cluster_dbscan", "largest_cluster"):
        from . import dbscan
        return getattr(dbscan, name)
    if name in ("segment_plane", "split_by_plane", "segment_planes"):
        from . import segment
        return getattr(segment, name)
    if name == "orient_normals_consistent_tangent_plane":
        from .orient import orient_normals_consistent_tangent_plane
        return orient_normals_consistent_tangent_plane
    if name in ("compute_iss_keypoints", "model_resolution"):
        from . import iss
        return getattr(iss, name)
    if name == "compute_point_cloud_distance":
        from .query import compute_point_cloud_distance
        return compute_point_cloud_distance
    if name in ("compute_color_gradient", "refine_registration_colored"):
        from . import colored
        return getattr(colored, name)
    if name in ("refine_registration_robust", "information_matrix"):
        from . import robust
        return getattr(robust, name)
    if name in ("optimize_pose_graph", "pose_graph_from_clouds", "register_multiway"):
        from . import posegraph
        return getattr(posegraph, name)
    if name == "compute_boundary_points":
        from .border import compute_boundary_points
        return compute_boundary_points
    if name == "smooth_mls":
        from .mls import smooth_mls
        return smooth_mls
    if name in ("consistency_registration", "correspondence_consistency", "prune_correspondences"):
        from . import consistency
        return getattr(consistency, name)
    if name in ("ndt_map", "ndt_derivatives", "refine_registration_ndt"):
        from . import ndt
        return getattr(ndt, name)
    if name in ("coherent_point_drift", "cpd_expectation"):
        from . import cpd
        return getattr(cpd, name)
    if name in ("centred", "uncentred_pose"):
        from . import centre
        return getattr(centre, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
