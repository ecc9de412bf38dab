"""plade_amd -- MI355X (gfx950) implementation of PLADE's registration hot path.

This package is a thin ctypes binding over the C ABI of ``libplade_hip.so`` (declared in
``include/plade_hip.h``).  There is no CPU fallback: importing the package is cheap, but creating
a :class:`Context` fails loudly when the HIP library or a GPU is missing.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libplade_hip.so")

PLADE_OK = 0
PLADE_EINVAL, PLADE_EDEVICE, PLADE_ECAP, PLADE_EFAIL, PLADE_ELIMIT = -1, -2, -3, -4, -5

# every symbol include/plade_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "plade_ctx_create", "plade_ctx_destroy", "plade_last_error", "plade_version", "plade_default_params",
    "plade_set_params", "plade_score_planes", "plade_extract_planes", "plade_match_descriptors",
    "plade_overlap_counts", "plade_average_spacing", "plade_voxel_downsample", "plade_registration_planes",
    "plade_registration", "plade_registration_minsupport", "plade_cloud_upload", "plade_cloud_free",
    "plade_registration_dev", "plade_dump_get", "plade_stats_get", "plade_kernel_time", "plade_plane_component",
    "plade_sort_pairs", "plade_host_pin", "plade_host_unpin", "plade_score_planes_subset", "plade_registration_next", "plade_cluster_transforms", "plade_device_synchronize", "plade_selftest_readback",
    "plade_registration_pairs", "plade_registration_pairs_dev", "plade_pair_ctx", "plade_set_candidate_shard", "plade_diag_launches", "plade_diag_cluster_order", "plade_diag_line_solver_host", "plade_sort_segments",
    "plade_closest_points", "plade_lines_meet", "plade_ply_read", "plade_ply_free",
    "plade_device_count", "plade_comm_unique_id", "plade_comm_create", "plade_comm_all_gather", "plade_comm_destroy", "plade_comm_last_error",
    "plade_set_candidate_shard_comm",
    "plade_estimate_normals", "plade_cloud_upload_xyz", "plade_ply_read_points",
    "plade_icp_default_params", "plade_refine_icp", "plade_refine_icp_dev", "plade_icp_linearize",
    "plade_cloud_distances", "plade_cloud_distances_dev",
    "plade_outlier_default_params", "plade_filter_outliers", "plade_cloud_filter_outliers_dev",
    "plade_merge_clouds", "plade_merge_clouds_dev", "plade_cloud_download",
    "plade_component_default_params", "plade_label_components", "plade_cloud_filter_components_dev",
    "plade_subsample_default_params", "plade_subsample_spacing", "plade_cloud_subsample_dev",
    "plade_orient_default_params", "plade_orient_normals", "plade_cloud_orient_normals_dev",
    "plade_smooth_default_params", "plade_smooth_cloud", "plade_cloud_smooth_dev",
    "plade_scale_default_params", "plade_cloud_scale_features", "plade_cloud_scale_normals_dev",
    "plade_gicp_default_params", "plade_refine_gicp", "plade_refine_gicp_dev", "plade_gicp_linearize",
    "plade_m3c2_default_params", "plade_cloud_m3c2", "plade_cloud_m3c2_dev",
    "plade_fpfh_default_params", "plade_cloud_fpfh", "plade_cloud_fpfh_dev", "plade_features_free",
    "plade_feature_match_default_params", "plade_match_features", "plade_match_features_dev",
    "plade_corr_pose_default_params", "plade_estimate_pose_corr", "plade_estimate_pose_corr_dev", "plade_corr_pose_moments",
    "plade_register_features", "plade_register_features_dev",
    "plade_iss_default_params", "plade_cloud_keypoints_iss", "plade_cloud_keypoints_iss_dev", "plade_features_select",
    "plade_register_keypoints", "plade_register_keypoints_dev",
    "plade_penetration_filter",
    "plade_dbscan_default_params", "plade_cluster_dbscan", "plade_cloud_cluster_dbscan_dev",
]

# plade_pen_item (include/plade_hip.h): one audited item of the penetration filter
PEN_ITEM = np.dtype([("k", np.uint32), ("i1", np.uint32), ("j1", np.uint32), ("plane1", np.float32, 4), ("start", np.float32, 3),
                     ("direc", np.float32, 3), ("length", np.float32), ("nsteps", np.int32), ("pos", np.int32, 2),
                     ("neg", np.int32, 2), ("gated", np.int32, 2), ("verdict", np.int32)])


class PladeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libplade_hip error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [("max_planes", C.c_int32), ("min_planes", C.c_int32), ("max_candidates", C.c_int32),
                ("init_min_support", C.c_int32), ("orient_normals", C.c_int32), ("dump", C.c_int32),
                ("ransac_seed", C.c_uint64), ("host_wait", C.c_int32), ("unoriented_normals", C.c_int32),
                ("ransac_topup", C.c_int32), ("match_window", C.c_int32), ("match_cell_budget", C.c_uint32),
                ("group_max_points", C.c_uint32), ("prepare_sides", C.c_int32), ("closest_point_mode", C.c_int32)]


class IcpParams(C.Structure):
    """plade_icp_params: 0 = the automatic value (source_leaf 0.005 D, max_dist 0.025 D, min_dist 0.0025 D, eps_translation 1e-6 D;
    D = the diagonal of the target's bounding box)."""
    _fields_ = [("source_leaf", C.c_double), ("max_dist", C.c_double), ("min_dist", C.c_double), ("eps_rotation", C.c_double),
                ("eps_translation", C.c_double), ("max_iterations", C.c_int32), ("min_correspondences", C.c_int32)]


class IcpResult(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("stages", C.c_int32), ("converged", C.c_int32), ("failure", C.c_int32),
                ("correspondences", C.c_uint32), ("samples", C.c_uint32), ("rmse", C.c_double), ("fitness", C.c_double),
                ("final_dist", C.c_double)]


class GicpParams(C.Structure):
    """plade_gicp_params: the seven fields of plade_icp_params with the same meaning and automatic values, and epsilon = the variance
    along the normal relative to 1 in the tangent plane (0: 1e-3; valid 0 < epsilon <= 1; 1 = point-to-point ICP)."""
    _fields_ = IcpParams._fields_ + [("epsilon", C.c_double)]


class GicpResult(C.Structure):
    """plade_gicp_result: the fields of plade_icp_result (rmse is point-to-point) and cost = sum e^T M e / count."""
    _fields_ = IcpResult._fields_ + [("cost", C.c_double)]


class DistanceSummary(C.Structure):
    """plade_distance_summary: count, fitness = count / n, rmse, mean and max of the distances of the correspondences, and the
    point-to-plane rmse over those with a finite target normal (NaN ratios when a count is 0)."""
    _fields_ = [("n", C.c_uint64), ("count", C.c_uint64), ("plane_count", C.c_uint64), ("fitness", C.c_double), ("rmse", C.c_double),
                ("mean", C.c_double), ("max", C.c_double), ("plane_rmse", C.c_double)]


class OutlierParams(C.Structure):
    """plade_outlier_params: mode (PLADE_OUTLIER_STATISTICAL / PLADE_OUTLIER_RADIUS), k and alpha of the statistical filter, radius
    and min_neighbours of the radius filter."""
    _fields_ = [("mode", C.c_int32), ("k", C.c_int32), ("alpha", C.c_double), ("radius", C.c_double), ("min_neighbours", C.c_int32),
                ("reserved", C.c_int32)]


class OutlierSummary(C.Structure):
    """plade_outlier_summary: n, kept, and mu, sigma, threshold = mu + alpha sigma of the statistical filter (NaN in radius mode)."""
    _fields_ = [("n", C.c_uint64), ("kept", C.c_uint64), ("mu", C.c_double), ("sigma", C.c_double), ("threshold", C.c_double)]


class MergeSummary(C.Structure):
    """plade_merge_summary: points in, rows out, rows seen by two or more clouds, the largest per-voxel count."""
    _fields_ = [("n_in", C.c_uint64), ("n_out", C.c_uint64), ("n_shared", C.c_uint64), ("max_count", C.c_uint32),
                ("reserved", C.c_uint32)]


class ComponentParams(C.Structure):
    """plade_component_params: radius of the edges, min_size / max_size (0: no bound) of a passing component, keep_largest (0: every
    passing component)."""
    _fields_ = [("radius", C.c_double), ("min_size", C.c_int32), ("max_size", C.c_int32), ("keep_largest", C.c_int32),
                ("reserved", C.c_int32)]


class DbscanParams(C.Structure):
    """plade_dbscan_params: radius of the neighbourhood, min_points (itself included) of a core point, min_size / max_size (0: no
    bound) of a passing cluster, keep_largest (0: every passing cluster)."""
    _fields_ = [("radius", C.c_double), ("min_points", C.c_int32), ("min_size", C.c_int32), ("max_size", C.c_int32),
                ("keep_largest", C.c_int32)]


class DbscanSummary(C.Structure):
    """plade_dbscan_summary: n, clusters, core, border, noise (points), kept_clusters, kept (points), largest (size)."""
    _fields_ = [("n", C.c_uint64), ("clusters", C.c_uint64), ("core", C.c_uint64), ("border", C.c_uint64), ("noise", C.c_uint64),
                ("kept_clusters", C.c_uint64), ("kept", C.c_uint64), ("largest", C.c_uint32), ("reserved", C.c_uint32)]


class ComponentSummary(C.Structure):
    """plade_component_summary: n, components, kept_components, kept (points), largest (size)."""
    _fields_ = [("n", C.c_uint64), ("components", C.c_uint64), ("kept_components", C.c_uint64), ("kept", C.c_uint64),
                ("largest", C.c_uint32), ("reserved", C.c_uint32)]


class SubsampleParams(C.Structure):
    """plade_subsample_params: the minimum spacing of the kept points (absolute, no default) and the seed of the priority keys."""
    _fields_ = [("spacing", C.c_double), ("seed", C.c_uint64)]


class SubsampleSummary(C.Structure):
    """plade_subsample_summary: n, kept, rounds (the synchronous rounds until every point was decided)."""
    _fields_ = [("n", C.c_uint32), ("kept", C.c_uint32), ("rounds", C.c_uint32)]


ORIENT_VOTE, ORIENT_EXTREME = 0, 1


class OrientParams(C.Structure):
    """plade_orient_params: the radius of the neighbour graph (absolute, no default), the anchor mode (ORIENT_VOTE with `viewpoint`,
    ORIENT_EXTREME with `direction`) and `inward`, which inverts the anchor's decision."""
    _fields_ = [("radius", C.c_double), ("mode", C.c_int32), ("inward", C.c_int32), ("viewpoint", C.c_float * 3),
                ("direction", C.c_float * 3)]


class OrientSummary(C.Structure):
    """plade_orient_summary: n, unoriented (invalid normals, left as they are), components, flipped, tree_edges, rounds and the
    sum of the forest's edge keys."""
    _fields_ = [("n", C.c_uint32), ("unoriented", C.c_uint32), ("components", C.c_uint32), ("flipped", C.c_uint32),
                ("tree_edges", C.c_uint32), ("rounds", C.c_uint32), ("tree_key_sum", C.c_uint64)]


class SmoothParams(C.Structure):
    """plade_smooth_params: radius of the neighbourhood (absolute, no default), min_neighbours of a fitted point (the point itself
    included), the viewpoint the fit's normals point toward."""
    _fields_ = [("radius", C.c_double), ("min_neighbours", C.c_int32), ("viewpoint", C.c_float * 3), ("reserved", C.c_int32)]


class SmoothSummary(C.Structure):
    """plade_smooth_summary: n, fitted, rms and max of |displacement| over the fitted points, max_count (the largest neighbourhood)."""
    _fields_ = [("n", C.c_uint64), ("fitted", C.c_uint64), ("rms", C.c_double), ("max", C.c_double), ("max_count", C.c_uint32),
                ("reserved", C.c_uint32)]


class ScaleParams(C.Structure):
    """plade_scale_params: the radii (the first `scales` of eight, absolute, fp32 squares strictly ascending), min_neighbours of a
    fitted scale (the point itself included), mode (0 the largest planarity, 1 the smallest surface variation), orient (0 toward the
    viewpoint, 1 along the rows' own normals) and the viewpoint."""
    _fields_ = [("radii", C.c_double * 8), ("scales", C.c_int32), ("min_neighbours", C.c_int32), ("mode", C.c_int32),
                ("orient", C.c_int32), ("viewpoint", C.c_float * 3), ("reserved", C.c_int32)]


class ScaleSummary(C.Structure):
    """plade_scale_summary: queries, fitted (queries with a chosen scale), chosen_hist (queries per chosen scale), max_count (the
    largest neighbourhood)."""
    _fields_ = [("queries", C.c_uint64), ("fitted", C.c_uint64), ("chosen_hist", C.c_uint32 * 8), ("max_count", C.c_uint32),
                ("reserved", C.c_uint32)]


class M3c2Params(C.Structure):
    """plade_m3c2_params: radius and depth (half-length) of the cylinder (absolute, no defaults), reg_error added to the level of
    detection, min_points per cloud of a valid core point."""
    _fields_ = [("radius", C.c_double), ("depth", C.c_double), ("reg_error", C.c_double), ("min_points", C.c_int32),
                ("reserved", C.c_int32)]


class M3c2Summary(C.Structure):
    """plade_m3c2_summary: m, valid, significant, the mean and rms of distance and the max of |distance| over the valid core points
    (NaN when there is none), max_count (the largest count of either cloud)."""
    _fields_ = [("m", C.c_uint64), ("valid", C.c_uint64), ("significant", C.c_uint64), ("mean", C.c_double), ("rms", C.c_double),
                ("max", C.c_double), ("max_count", C.c_uint32), ("reserved", C.c_uint32)]


class FpfhParams(C.Structure):
    """plade_fpfh_params: the radius of the neighbourhood (absolute, no default), min_pairs of a described point."""
    _fields_ = [("radius", C.c_double), ("min_pairs", C.c_int32), ("reserved", C.c_int32)]


class FpfhSummary(C.Structure):
    """plade_fpfh_summary: n, described, mean_pairs (over the described points), max_pairs (of any point)."""
    _fields_ = [("n", C.c_uint64), ("described", C.c_uint64), ("mean_pairs", C.c_double), ("max_pairs", C.c_uint32),
                ("reserved", C.c_uint32)]


class FeatureMatchParams(C.Structure):
    """plade_feature_match_params: mutual (0 / 1), max_ratio (0 = off)."""
    _fields_ = [("mutual", C.c_int32), ("max_ratio", C.c_float)]


class CorrPoseParams(C.Structure):
    """plade_corr_pose_params: inlier_dist (absolute, no default), edge_similarity of the prerejection, seed, hypotheses, min_inliers,
    refine_iterations."""
    _fields_ = [("inlier_dist", C.c_double), ("edge_similarity", C.c_double), ("seed", C.c_uint64), ("hypotheses", C.c_int32),
                ("min_inliers", C.c_int32), ("refine_iterations", C.c_int32), ("reserved", C.c_int32)]


class CorrPoseResult(C.Structure):
    """plade_corr_pose_result: hypotheses drawn and scored, the best one and its count, inliers / rmse / fitness under the final T,
    refinements (accepted refits), failure (0 or PLADE_CORR_POSE_*)."""
    _fields_ = [("hypotheses", C.c_uint32), ("scored", C.c_uint32), ("best_hypothesis", C.c_uint32), ("best_count", C.c_uint32),
                ("inliers", C.c_uint32), ("refinements", C.c_int32), ("failure", C.c_int32), ("reserved", C.c_int32),
                ("rmse", C.c_double), ("fitness", C.c_double), ("T", C.c_double * 12)]


class IssParams(C.Structure):
    """plade_iss_params: salient_radius (absolute, no default), non_max_radius (0: salient_radius), the eigenvalue ratio bounds
    gamma21 and gamma32, min_neighbours within non_max_radius of a keypoint."""
    _fields_ = [("salient_radius", C.c_double), ("non_max_radius", C.c_double), ("gamma21", C.c_double), ("gamma32", C.c_double),
                ("min_neighbours", C.c_int32), ("reserved", C.c_int32)]


class IssSummary(C.Structure):
    """plade_iss_summary: n, salient, keypoints, max_count (the largest neighbourhood within salient_radius)."""
    _fields_ = [("n", C.c_uint64), ("salient", C.c_uint64), ("keypoints", C.c_uint64), ("max_count", C.c_uint32),
                ("reserved", C.c_uint32)]


PLADE_CORR_POSE_TOO_FEW, PLADE_CORR_POSE_NONE_SCORED, PLADE_CORR_POSE_FEW_INLIERS = 1, 2, 3
CORR_POSE_FAILURES = {0: None, PLADE_CORR_POSE_TOO_FEW: "fewer than 3 correspondences", PLADE_CORR_POSE_NONE_SCORED: "nothing scored",
                      PLADE_CORR_POSE_FEW_INLIERS: "too few inliers"}
CORR_MOMENTS = 17    # corr_pose.h: n, mean S (3), mean Q (3), C (9), sum d2

FPFH_DIM = 33
FEAT_CHUNK = 512     # fpfh.h: the smallest number of targets one workgroup of the match takes

PLADE_OUTLIER_STATISTICAL, PLADE_OUTLIER_RADIUS = 0, 1
OUTLIER_MODES = {"statistical": PLADE_OUTLIER_STATISTICAL, "radius": PLADE_OUTLIER_RADIUS}

PLADE_ICP_TOO_FEW, PLADE_ICP_DEGENERATE = 1, 2
ICP_FAILURES = {0: None, PLADE_ICP_TOO_FEW: "too few correspondences", PLADE_ICP_DEGENERATE: "degenerate"}

EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_uint32, C.c_uint32)

_lib = None


def load_library(path=LIB_PATH):
    """Load libplade_hip.so; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} is missing: build it with `make lib` or __graft_entry__.build(); "
                                "plade_amd has no CPU fallback")
    L = C.CDLL(path)
    p, f, i32, u32, u64 = C.c_void_p, C.c_float, C.c_int32, C.c_uint32, C.c_uint64
    def sig(name, argtypes=None, restype=None):
        # a symbol missing from the library is reported by Context/_need, never silently replaced
        fn = getattr(L, name, None)
        if fn is None:
            return
        if argtypes is not None:
            fn.argtypes = argtypes
        if restype is not None:
            fn.restype = restype

    sig("plade_version", restype=C.c_char_p)
    sig("plade_last_error", restype=C.c_char_p)
    sig("plade_last_error", argtypes=[p])
    sig("plade_device_synchronize", argtypes=[C.c_int])
    sig("plade_ctx_create", argtypes=[C.c_int, C.POINTER(p)])
    sig("plade_ctx_destroy", argtypes=[p])
    sig("plade_default_params", argtypes=[C.POINTER(Params)])
    sig("plade_set_params", argtypes=[p, C.POINTER(Params)])
    sig("plade_score_planes", argtypes=[p, p, p, u32, p, u32, f, f, p, p, u32])
    sig("plade_score_planes_subset", argtypes=[p, p, p, u32, p, u32, p, u32, f, f, p, p])
    sig("plade_extract_planes", argtypes=[p, p, u32, u32, f, f, f, f, p, p, p, u32, p])
    sig("plade_match_descriptors", argtypes=[p, p, u32, p, u32, f, p, p, p, u64, p])
    sig("plade_cluster_transforms", argtypes=[p, p, p, u32, f, f, p, p])
    sig("plade_penetration_filter", argtypes=[p, p, u32, p, p, p, p, p, u32, p, p, p, p, p, u32, f, f, p, p, u64, p])
    sig("plade_overlap_counts", argtypes=[p, p, u32, p, u32, p, u32, p, f, f, p])
    sig("plade_average_spacing", argtypes=[p, p, u32, u32, u32, u32, p])
    sig("plade_voxel_downsample", argtypes=[p, p, u32, u32, f, p, p])
    sig("plade_registration_planes", argtypes=[p, p, u32, p, u32, p, p, p, u32, p, p, p, u32, p])
    sig("plade_registration", argtypes=[p, p, u32, p, u32, p])
    sig("plade_registration_next", argtypes=[p, p, u32, p, u32, p, u32, p, u32, p])
    sig("plade_registration_pairs", argtypes=[p, u32, p, p, p, p, u32, p, p, p, p, p, p])
    sig("plade_registration_pairs_dev", argtypes=[p, u32, p, p, p, p])
    sig("plade_pair_ctx", argtypes=[p, u32], restype=p)
    sig("plade_closest_points", argtypes=[p, i32, p, p, p, p, u32, p, p, p, p])
    sig("plade_lines_meet", argtypes=[p, i32, p, p, p, p, u32, p, p])
    sig("plade_diag_launches", argtypes=[p, u32, u32, u32])
    sig("plade_diag_cluster_order", argtypes=[p, u32, i32, i32, p])
    sig("plade_diag_line_solver_host", argtypes=[i32, p, p, p, p, u32, p, p, p])
    sig("plade_ply_read", argtypes=[C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(u64), C.c_char_p, C.c_size_t])
    sig("plade_ply_free", argtypes=[C.POINTER(C.c_float)], restype=None)
    sig("plade_ply_read_points", argtypes=[C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(u64), C.POINTER(i32), C.c_char_p,
                                           C.c_size_t])
    sig("plade_estimate_normals", argtypes=[p, p, u32, u32, i32, p, p, p, p])
    sig("plade_cloud_upload_xyz", argtypes=[p, p, u32, u32, i32, p, C.POINTER(p)])
    sig("plade_icp_default_params", argtypes=[C.POINTER(IcpParams)], restype=None)
    sig("plade_refine_icp", argtypes=[p, p, u32, p, u32, p, C.POINTER(IcpParams), p, C.POINTER(IcpResult)])
    sig("plade_refine_icp_dev", argtypes=[p, p, p, p, C.POINTER(IcpParams), p, C.POINTER(IcpResult)])
    sig("plade_icp_linearize", argtypes=[p, p, u32, p, u32, u32, p, p, f, p, p])
    sig("plade_gicp_default_params", argtypes=[C.POINTER(GicpParams)], restype=None)
    sig("plade_refine_gicp", argtypes=[p, p, u32, p, u32, p, C.POINTER(GicpParams), p, C.POINTER(GicpResult)])
    sig("plade_refine_gicp_dev", argtypes=[p, p, p, p, C.POINTER(GicpParams), p, C.POINTER(GicpResult)])
    sig("plade_gicp_linearize", argtypes=[p, p, u32, p, u32, p, p, f, C.c_double, p, p])
    sig("plade_cloud_distances", argtypes=[p, p, u32, p, u32, u32, p, f, p, p, p, C.POINTER(DistanceSummary)])
    sig("plade_cloud_distances_dev", argtypes=[p, p, p, p, f, p, p, p, C.POINTER(DistanceSummary)])
    sig("plade_outlier_default_params", argtypes=[C.POINTER(OutlierParams)], restype=None)
    sig("plade_filter_outliers", argtypes=[p, p, u32, u32, C.POINTER(OutlierParams), p, p, p, p, p, C.POINTER(OutlierSummary)])
    sig("plade_cloud_filter_outliers_dev", argtypes=[p, p, C.POINTER(OutlierParams), C.POINTER(p), p, p, C.POINTER(OutlierSummary)])
    sig("plade_merge_clouds", argtypes=[p, u32, p, p, p, f, p, p, p, C.POINTER(MergeSummary)])
    sig("plade_merge_clouds_dev", argtypes=[p, u32, p, p, f, C.POINTER(p), p, p, C.POINTER(MergeSummary)])
    sig("plade_cloud_download", argtypes=[p, p, p, u32, C.POINTER(u32)])
    sig("plade_component_default_params", argtypes=[C.POINTER(ComponentParams)], restype=None)
    sig("plade_label_components", argtypes=[p, p, u32, u32, C.POINTER(ComponentParams), p, p, p, p, p, C.POINTER(ComponentSummary)])
    sig("plade_cloud_filter_components_dev", argtypes=[p, p, C.POINTER(ComponentParams), C.POINTER(p), p, p, C.POINTER(ComponentSummary)])
    sig("plade_dbscan_default_params", argtypes=[C.POINTER(DbscanParams)], restype=None)
    sig("plade_cluster_dbscan", argtypes=[p, p, u32, u32, C.POINTER(DbscanParams), p, p, p, p, p, p, C.POINTER(DbscanSummary)])
    sig("plade_cloud_cluster_dbscan_dev", argtypes=[p, p, C.POINTER(DbscanParams), C.POINTER(p), p, p, p, C.POINTER(DbscanSummary)])
    sig("plade_subsample_default_params", argtypes=[C.POINTER(SubsampleParams)], restype=None)
    sig("plade_subsample_spacing", argtypes=[p, p, u32, u32, C.POINTER(SubsampleParams), p, p, p, p, C.POINTER(SubsampleSummary)])
    sig("plade_cloud_subsample_dev", argtypes=[p, p, C.POINTER(SubsampleParams), C.POINTER(p), p, p, C.POINTER(SubsampleSummary)])
    sig("plade_orient_default_params", argtypes=[C.POINTER(OrientParams)], restype=None)
    sig("plade_orient_normals", argtypes=[p, p, u32, C.POINTER(OrientParams), p, p, p, C.POINTER(OrientSummary)])
    sig("plade_cloud_orient_normals_dev", argtypes=[p, p, C.POINTER(OrientParams), C.POINTER(p), p, p, C.POINTER(OrientSummary)])
    sig("plade_smooth_default_params", argtypes=[C.POINTER(SmoothParams)], restype=None)
    sig("plade_smooth_cloud", argtypes=[p, p, u32, u32, C.POINTER(SmoothParams), p, p, p, p, p, p, p, C.POINTER(SmoothSummary)])
    sig("plade_cloud_smooth_dev", argtypes=[p, p, C.POINTER(SmoothParams), i32, C.POINTER(p), C.POINTER(SmoothSummary)])
    sig("plade_scale_default_params", argtypes=[C.POINTER(ScaleParams)], restype=None)
    sig("plade_cloud_scale_features", argtypes=[p, p, u32, u32, p, u32, C.POINTER(ScaleParams), p, p, p, p, p, p, p, p,
                                                C.POINTER(ScaleSummary)])
    sig("plade_cloud_scale_normals_dev", argtypes=[p, p, p, u32, C.POINTER(ScaleParams), C.POINTER(p), C.POINTER(ScaleSummary)])
    sig("plade_m3c2_default_params", argtypes=[C.POINTER(M3c2Params)], restype=None)
    sig("plade_cloud_m3c2", argtypes=[p, p, u32, p, u32, u32, p, u32, u32, p, C.POINTER(M3c2Params), p, p, p, p, p, p,
                                      C.POINTER(M3c2Summary)])
    sig("plade_cloud_m3c2_dev", argtypes=[p, p, p, p, p, C.POINTER(M3c2Params), p, p, p, p, p, p, C.POINTER(M3c2Summary)])
    sig("plade_fpfh_default_params", argtypes=[C.POINTER(FpfhParams)], restype=None)
    sig("plade_cloud_fpfh", argtypes=[p, p, u32, C.POINTER(FpfhParams), p, p, p, p, p, C.POINTER(FpfhSummary)])
    sig("plade_cloud_fpfh_dev", argtypes=[p, p, C.POINTER(FpfhParams), p, p, p, p, p, C.POINTER(p), C.POINTER(FpfhSummary)])
    sig("plade_features_free", argtypes=[p], restype=None)
    sig("plade_feature_match_default_params", argtypes=[C.POINTER(FeatureMatchParams)], restype=None)
    sig("plade_match_features", argtypes=[p, p, u32, p, u32, C.POINTER(FeatureMatchParams), p, p, p, p, C.c_uint64,
                                          C.POINTER(C.c_uint64)])
    sig("plade_match_features_dev", argtypes=[p, p, p, C.POINTER(FeatureMatchParams), p, p, p, p, C.c_uint64, C.POINTER(C.c_uint64)])
    sig("plade_corr_pose_default_params", argtypes=[C.POINTER(CorrPoseParams)], restype=None)
    sig("plade_estimate_pose_corr", argtypes=[p, p, u32, u32, p, u32, u32, p, u64, C.POINTER(CorrPoseParams), p, p, p, p, p, p,
                                              C.POINTER(CorrPoseResult)])
    sig("plade_estimate_pose_corr_dev", argtypes=[p, p, p, p, u64, C.POINTER(CorrPoseParams), p, p, p, p, p, p, C.POINTER(CorrPoseResult)])
    sig("plade_corr_pose_moments", argtypes=[p, p, u32, u32, p, u32, u32, p, u64, p, C.c_double, p, p])
    sig("plade_register_features", argtypes=[p, p, u32, p, u32, C.POINTER(FpfhParams), C.POINTER(FeatureMatchParams),
                                             C.POINTER(CorrPoseParams), p, C.POINTER(FpfhSummary), C.POINTER(FpfhSummary),
                                             C.POINTER(CorrPoseResult), p, u64, C.POINTER(u64)])
    sig("plade_register_features_dev", argtypes=[p, p, p, C.POINTER(FpfhParams), C.POINTER(FeatureMatchParams),
                                                 C.POINTER(CorrPoseParams), p, C.POINTER(FpfhSummary), C.POINTER(FpfhSummary),
                                                 C.POINTER(CorrPoseResult), p, u64, C.POINTER(u64)])
    sig("plade_iss_default_params", argtypes=[C.POINTER(IssParams)], restype=None)
    sig("plade_cloud_keypoints_iss", argtypes=[p, p, u32, u32, C.POINTER(IssParams), p, p, u64, C.POINTER(u64), p, p, p, p, p,
                                               C.POINTER(IssSummary)])
    sig("plade_cloud_keypoints_iss_dev", argtypes=[p, p, C.POINTER(IssParams), p, p, u64, C.POINTER(u64), p, p, p, p, p,
                                                   C.POINTER(IssSummary)])
    sig("plade_features_select", argtypes=[p, p, p, u32, C.POINTER(p)])
    sig("plade_register_keypoints", argtypes=[p, p, u32, p, u32, C.POINTER(IssParams), C.POINTER(FpfhParams),
                                              C.POINTER(FeatureMatchParams), C.POINTER(CorrPoseParams), p, C.POINTER(IssSummary),
                                              C.POINTER(FpfhSummary), C.POINTER(FpfhSummary), C.POINTER(CorrPoseResult), p, u64,
                                              C.POINTER(u64)])
    sig("plade_register_keypoints_dev", argtypes=[p, p, p, C.POINTER(IssParams), C.POINTER(FpfhParams), C.POINTER(FeatureMatchParams),
                                                  C.POINTER(CorrPoseParams), p, C.POINTER(IssSummary), C.POINTER(FpfhSummary),
                                                  C.POINTER(FpfhSummary), C.POINTER(CorrPoseResult), p, u64, C.POINTER(u64)])
    sig("plade_sort_segments", argtypes=[p, p, p, p, u32, C.c_int, p, p])
    sig("plade_set_candidate_shard", argtypes=[p, u32, u32, u32, EXCHANGE_FN, p])
    sig("plade_registration_minsupport", argtypes=[p, p, u32, p, u32, i32, i32, p])
    sig("plade_cloud_upload", argtypes=[p, p, u32, C.POINTER(p)])
    sig("plade_cloud_free", argtypes=[p, p])
    sig("plade_registration_dev", argtypes=[p, p, p, p])
    sig("plade_dump_get", argtypes=[p, C.c_char_p, C.POINTER(p), C.POINTER(C.c_int64)])
    sig("plade_stats_get", argtypes=[p, C.POINTER(C.c_char_p), C.POINTER(C.POINTER(C.c_double)), C.POINTER(i32)])
    sig("plade_kernel_time", argtypes=[p, C.c_char_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)])
    sig("plade_plane_component", argtypes=[p, p, u32, p, p, p, u32, f, C.c_int, f, p, p, p, p])
    sig("plade_sort_pairs", argtypes=[p, p, p, u32, C.c_int, C.c_int, p, p])
    sig("plade_selftest_readback", argtypes=[p, u32, u32, C.POINTER(u32)])
    sig("plade_host_pin", argtypes=[p, p, C.c_size_t])
    sig("plade_host_unpin", argtypes=[p, p])
    _lib = L
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# name -> dtype of the intermediates plade_dump_get can return (same names as the oracle's dump)
DUMP_FIELDS = {
    "average_spacing": np.float32, "scale": np.float32,
    "tgt_ds": np.float32, "src_ds": np.float32, "tgt_bcenter": np.float32, "src_bcenter": np.float32,
    "tgt_radius": np.float64, "src_radius": np.float64,
    "tgt_plane_center_radius": np.float32, "src_plane_center_radius": np.float32,
    "tgt_plane_four": np.float32, "src_plane_four": np.float32,
    "tgt_plane_ds_offsets": np.int32, "src_plane_ds_offsets": np.int32,
    "tgt_plane_ds": np.float32, "src_plane_ds": np.float32,
    "tgt_lines": np.float32, "src_lines": np.float32,
    "tgt_desc": np.float32, "src_desc": np.float32,
    "match_offsets": np.int64, "match_nbr": np.int32, "match_dist2": np.float64,
    "initial_RT": np.float32, "cluster_sizes": np.int32, "cluster_seeds": np.int32,
    "plane_match_counts": np.int32, "pen_tested": np.int32, "pen_flags": np.int32, "pen_candidates": np.float32,
    "candidates": np.float32, "candidate_centers": np.float32, "overlap_counts": np.int32,
    "scores": np.float32, "best_index": np.int32,
    "tgt_planes": np.float32, "tgt_plane_offsets": np.int32, "tgt_plane_idx": np.int32,
    "src_planes": np.float32, "src_plane_offsets": np.int32, "src_plane_idx": np.int32,
}
# the acceptance chains of the last detect call of a cloud (ransac.h: ExtractTrace; replayed by tests/extract_replay.py):
# untagged after extract_planes, tgt_ / src_ after a registration
EXTRACT_TRACE_FIELDS = {"call_u": np.uint32, "call_f": np.float32, "entry": np.int32, "cand": np.float32,
                        "slot_f": np.float32, "slot_u": np.uint32, "slot_w": np.float64}
for _tag in ("", "tgt_", "src_"):
    for _k, _dt in EXTRACT_TRACE_FIELDS.items():
        DUMP_FIELDS[f"{_tag}extract_trace_{_k}"] = _dt


def device_synchronize(device=0):
    """hipDeviceSynchronize on `device` through the library (no torch needed in a single-GPU process)."""
    rc = load_library().plade_device_synchronize(int(device))
    if rc != 0:
        raise PladeError(rc, "plade_device_synchronize failed")


# the params struct -> the library's function that fills in its defaults
_DEFAULTS = {Params: "plade_default_params",
             IcpParams: "plade_icp_default_params",
             OutlierParams: "plade_outlier_default_params",
             ComponentParams: "plade_component_default_params",
             DbscanParams: "plade_dbscan_default_params",
             SubsampleParams: "plade_subsample_default_params",
             OrientParams: "plade_orient_default_params",
             SmoothParams: "plade_smooth_default_params",
             ScaleParams: "plade_scale_default_params",
             M3c2Params: "plade_m3c2_default_params",
             FpfhParams: "plade_fpfh_default_params",
             FeatureMatchParams: "plade_feature_match_default_params",
             CorrPoseParams: "plade_corr_pose_default_params",
             IssParams: "plade_iss_default_params",
             GicpParams: "plade_gicp_default_params"}


def _defaults(struct):
    prm = struct()
    getattr(load_library(), _DEFAULTS[struct])(C.byref(prm))
    return prm


def _defaults_dict(struct):
    """the defaults of a params struct as a dict of its fields (without `reserved`; an array field as a tuple)"""
    prm = _defaults(struct)
    vals = ((k, getattr(prm, k)) for k, _ in struct._fields_ if k != "reserved")
    return {k: tuple(v) if isinstance(v, C.Array) else v for k, v in vals}


def default_params():
    """plade_default_params (pure: needs no GPU): the library's shipped defaults = the reference's behaviour."""
    return _defaults(Params)


def icp_default_params():
    """plade_icp_default_params (pure: needs no GPU) as a dict of the plade_icp_params fields."""
    return _defaults_dict(IcpParams)


def outlier_default_params():
    """plade_outlier_default_params (pure: needs no GPU) as a dict of the plade_outlier_params fields."""
    return _defaults_dict(OutlierParams)


def _outlier_params(mode, k, alpha, radius, min_neighbours):
    prm = _defaults(OutlierParams)
    if mode not in OUTLIER_MODES:
        raise ValueError(f"mode: 'statistical' or 'radius', got {mode!r}")
    prm.mode = OUTLIER_MODES[mode]
    if k is not None:
        prm.k = int(k)
    if alpha is not None:
        prm.alpha = float(alpha)
    if radius is not None:
        prm.radius = float(radius)
    if min_neighbours is not None:
        prm.min_neighbours = int(min_neighbours)
    return prm


def _outlier_info(summ, keep):
    info = {k: getattr(summ, k) for k, _ in OutlierSummary._fields_}
    info["keep"] = keep.view(np.bool_)
    return info


def component_default_params():
    """plade_component_default_params (pure: needs no GPU) as a dict of the plade_component_params fields."""
    return _defaults_dict(ComponentParams)


def _component_params(radius, min_size, max_size, keep_largest):
    prm = _defaults(ComponentParams)
    prm.radius = float(radius)
    prm.min_size, prm.max_size, prm.keep_largest = int(min_size), int(max_size), int(keep_largest)
    return prm


def _component_info(summ, label, size, keep):
    info = {k: getattr(summ, k) for k, _ in ComponentSummary._fields_ if k != "reserved"}
    info["label"] = label
    if size is not None:
        info["size"] = size[:summ.components].copy()
    if keep is not None:
        info["keep"] = keep.view(np.bool_)
    return info


def dbscan_default_params():
    """plade_dbscan_default_params (pure: needs no GPU) as a dict of the plade_dbscan_params fields."""
    return _defaults_dict(DbscanParams)


def _dbscan_params(radius, min_points, min_size, max_size, keep_largest):
    prm = _defaults(DbscanParams)
    prm.radius = float(radius)
    prm.min_points, prm.min_size, prm.max_size, prm.keep_largest = int(min_points), int(min_size), int(max_size), int(keep_largest)
    return prm


def _dbscan_info(summ, label, kind, size, keep):
    info = {k: getattr(summ, k) for k, _ in DbscanSummary._fields_ if k != "reserved"}
    info["label"] = label
    info["kind"] = kind
    if size is not None:
        info["size"] = size[:summ.clusters].copy()
    if keep is not None:
        info["keep"] = keep.view(np.bool_)
    return info


def subsample_default_params():
    """plade_subsample_default_params (pure: needs no GPU) as a dict of the plade_subsample_params fields."""
    return _defaults_dict(SubsampleParams)


def _subsample_params(spacing, seed):
    prm = _defaults(SubsampleParams)
    prm.spacing = float(spacing)
    prm.seed = int(seed)
    return prm


def _subsample_info(summ, keep, rnd):
    info = {k: getattr(summ, k) for k, _ in SubsampleSummary._fields_}
    if keep is not None:
        info["keep"] = keep.view(np.bool_)
    if rnd is not None:
        info["round"] = rnd
    return info


def orient_default_params():
    """plade_orient_default_params (pure: needs no GPU) as a dict of the plade_orient_params fields."""
    return _defaults_dict(OrientParams)


def _orient_params(radius, mode, inward, viewpoint, direction):
    prm = _defaults(OrientParams)
    prm.radius = float(radius)
    prm.mode = int(mode)
    prm.inward = int(inward)
    prm.viewpoint[:] = [float(x) for x in _viewpoint(viewpoint)]
    prm.direction[:] = [float(x) for x in _viewpoint(direction)]
    return prm


def _orient_info(summ, flip, label):
    info = {k: getattr(summ, k) for k, _ in OrientSummary._fields_}
    if flip is not None:
        info["flip"] = flip.view(np.bool_)
        info["label"] = label
    return info


def smooth_default_params():
    """plade_smooth_default_params (pure: needs no GPU) as a dict of the plade_smooth_params fields."""
    return _defaults_dict(SmoothParams)


def _smooth_params(radius, min_neighbours, viewpoint):
    prm = _defaults(SmoothParams)
    prm.radius = float(radius)
    if min_neighbours is not None:
        prm.min_neighbours = int(min_neighbours)
    prm.viewpoint[:] = [float(x) for x in _viewpoint(viewpoint)]
    return prm


def _smooth_info(summ):
    return {k: getattr(summ, k) for k, _ in SmoothSummary._fields_ if k != "reserved"}


def scale_default_params():
    """plade_scale_default_params (pure: needs no GPU) as a dict of the plade_scale_params fields."""
    return _defaults_dict(ScaleParams)


def _scale_params(radii, mode, min_neighbours, viewpoint, orient):
    prm = _defaults(ScaleParams)
    r = [float(x) for x in np.asarray(radii, np.float64).reshape(-1)]
    prm.scales = len(r)              # (the library refuses a number outside 1 .. 8)
    prm.radii[:] = (r + [0.0] * 8)[:8]
    prm.mode, prm.orient = int(mode), int(orient)
    if min_neighbours is not None:
        prm.min_neighbours = int(min_neighbours)
    prm.viewpoint[:] = [float(x) for x in _viewpoint(viewpoint)]
    return prm


def _scale_queries(query_index):
    """(the list as a C-contiguous uint32 array or None, its length)"""
    if query_index is None:
        return None, 0
    q = np.ascontiguousarray(query_index, dtype=np.uint32).reshape(-1)
    return q, len(q)


def _scale_info(summ, scales):
    info = {k: getattr(summ, k) for k, _ in ScaleSummary._fields_ if k not in ("reserved", "chosen_hist")}
    info["chosen_hist"] = tuple(summ.chosen_hist)[:max(0, min(scales, 8))]
    return info


def m3c2_default_params():
    """plade_m3c2_default_params (pure: needs no GPU) as a dict of the plade_m3c2_params fields."""
    return _defaults_dict(M3c2Params)


def _m3c2_params(radius, depth, min_points, reg_error):
    prm = _defaults(M3c2Params)
    prm.radius, prm.depth, prm.reg_error = float(radius), float(depth), float(reg_error)
    if min_points is not None:
        prm.min_points = int(min_points)
    return prm


def fpfh_default_params():
    """plade_fpfh_default_params (pure: needs no GPU) as a dict of the plade_fpfh_params fields."""
    return _defaults_dict(FpfhParams)


def feature_match_default_params():
    """plade_feature_match_default_params (pure: needs no GPU) as a dict."""
    return _defaults_dict(FeatureMatchParams)


def corr_pose_default_params():
    """plade_corr_pose_default_params (pure: needs no GPU) as a dict of the plade_corr_pose_params fields."""
    return _defaults_dict(CorrPoseParams)


def iss_default_params():
    """plade_iss_default_params (pure: needs no GPU) as a dict of the plade_iss_params fields."""
    return _defaults_dict(IssParams)


def _iss_params(salient_radius, non_max_radius, gamma21, gamma32, min_neighbours):
    prm = _defaults(IssParams)
    prm.salient_radius, prm.non_max_radius = float(salient_radius), float(non_max_radius)
    if gamma21 is not None:
        prm.gamma21 = float(gamma21)
    if gamma32 is not None:
        prm.gamma32 = float(gamma32)
    if min_neighbours is not None:
        prm.min_neighbours = int(min_neighbours)
    return prm


def _corr_pose_params(inlier_dist, kw):
    prm = _defaults(CorrPoseParams)
    prm.inlier_dist = float(inlier_dist)
    known = {k for k, _ in CorrPoseParams._fields_} - {"reserved", "inlier_dist"}
    for k, v in kw.items():
        if k not in known:
            raise TypeError(f"unknown pose parameter {k!r} (known: {sorted(known)})")
        if v is not None:
            setattr(prm, k, v)
    return prm


def _corr_pose_info(res):
    """the fields of a plade_corr_pose_result as a dict; its T as the (3, 4) float64 array T64"""
    info = {k: getattr(res, k) for k, _ in CorrPoseResult._fields_ if k not in ("reserved", "T")}
    info["T64"] = np.array(res.T[:], np.float64).reshape(3, 4)
    return info


def _corr_list(corr, what):
    c = _i32(corr)
    if c.ndim != 2 or c.shape[1] != 2:
        raise ValueError(f"{what}: an (M, 2) int32 array of (source, target) indices is required, got shape {c.shape}")
    return c


def _fpfh_params(radius, min_pairs):
    prm = _defaults(FpfhParams)
    prm.radius = float(radius)
    if min_pairs is not None:
        prm.min_pairs = int(min_pairs)
    return prm


def _feature_match_params(mutual, max_ratio):
    prm = _defaults(FeatureMatchParams)
    prm.mutual, prm.max_ratio = int(bool(mutual)), float(max_ratio)
    return prm


def _feature_table(a, what):
    a = _f32(a)
    if a.ndim != 2 or a.shape[1] != FPFH_DIM:
        raise ValueError(f"{what}: an (N, 33) array of descriptors is required, got shape {a.shape}")
    return a


def gicp_default_params():
    """plade_gicp_default_params (pure: needs no GPU) as a dict of the plade_gicp_params fields."""
    return _defaults_dict(GicpParams)


# the two refinements: the params and result structs and the name in the messages
_ICP, _GICP = (IcpParams, IcpResult, "ICP"), (GicpParams, GicpResult, "GICP")


def _refine_params(kw, model):
    prm = _defaults(model[0])
    for k, v in kw.items():
        if k not in dict(model[0]._fields_):
            raise TypeError(f"unknown {model[2]} parameter {k!r}")
        setattr(prm, k, v)
    return prm


def _refine_info(res):
    info = {k: getattr(res, k) for k, _ in res._fields_}
    info["converged"] = bool(info["converged"])
    info["reason"] = ICP_FAILURES.get(info["failure"], "unknown")
    return info


def read_ply(path):
    """plade_ply_read (no GPU): the CLI's PLY ingest -> (N, 6) float32 array x y z nx ny nz; raises PladeError with the
    reader's message where the reference's load_ply_cloud (code/PLADE/util.cpp:1505-1546) returns false."""
    L = load_library()
    ptr, n = C.POINTER(C.c_float)(), C.c_uint64(0)
    err = C.create_string_buffer(512)
    rc = L.plade_ply_read(os.fsencode(path), C.byref(ptr), C.byref(n), err, len(err))
    if rc != 0:
        raise PladeError(rc, err.value.decode(errors="replace"))
    try:
        return np.ctypeslib.as_array(ptr, shape=(n.value, 6)).copy()
    finally:
        L.plade_ply_free(ptr)


def read_ply_points(path):
    """plade_ply_read_points (no GPU): read_ply that also accepts a vertex element without nx ny nz.  Returns (array, has_normals):
    the (N, 6) float32 array x y z nx ny nz -- NaN normal columns when has_normals is False (estimate them with
    Context.estimate_normals(array[:, :3]) or Context.upload_xyz) -- and whether the file had normals.  Every other failure
    raises PladeError with read_ply's message."""
    L = load_library()
    ptr, n, has = C.POINTER(C.c_float)(), C.c_uint64(0), C.c_int32(0)
    err = C.create_string_buffer(512)
    rc = L.plade_ply_read_points(os.fsencode(path), C.byref(ptr), C.byref(n), C.byref(has), err, len(err))
    if rc != 0:
        raise PladeError(rc, err.value.decode(errors="replace"))
    try:
        return np.ctypeslib.as_array(ptr, shape=(n.value, 6)).copy(), bool(has.value)
    finally:
        L.plade_ply_free(ptr)


def _xyz_view(xyz):
    """(N, >= 3) float32 array -> (C-contiguous array, n, stride in floats) for the xyz entry points (no copy of an N x 6 cloud)."""
    a = _f32(xyz)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError(f"an (N, 3) array x y z (or wider rows whose first three columns are x y z) is required, got shape {a.shape}")
    return a, len(a), a.shape[1]


def _viewpoint(viewpoint):
    v = _f32(viewpoint).reshape(-1)
    if v.shape != (3,):
        raise ValueError("viewpoint: three coordinates")
    return v


def line_solver_host(kind, a, b, c, d):
    """Host seam (no GPU): the register form of the reference's SVD solver as the kernels inline it -- kind 0: closest points of
    n line pairs -> (q1, q2, ok), kind 1: meeting points -> (point, ok); ok 1 solved / 0 rank-deficient / -1 guard fired."""
    a, b, c, d = (_f32(x).reshape(-1, 3) for x in (a, b, c, d))
    n = len(a)
    o1, o2, ok = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
    rc = load_library().plade_diag_line_solver_host(int(kind), _ptr(a), _ptr(b), _ptr(c), _ptr(d), n, _ptr(o1), _ptr(o2), _ptr(ok))
    if rc != 0:
        raise PladeError(rc, "plade_diag_line_solver_host failed")
    return (o1, o2, ok) if kind == 0 else (o1, ok)


def cluster_order(sizes, mode=0, depth_limit=-1):
    """Host seam: the order std::sort(..., myCompareGreater) (util.cpp:335-345) gives clusters of these sizes -- mode 0: the
    library's implementation, 1: std::sort, 2 / 3: block-wise / sequential partition at a given recursion depth limit."""
    a = _f32(sizes).reshape(-1)
    out = np.zeros(len(a), np.int32)
    rc = load_library().plade_diag_cluster_order(a.ctypes.data_as(C.c_void_p), len(a), int(mode), int(depth_limit),
                                                 out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PladeError(rc, "plade_diag_cluster_order failed")
    return out


class Cloud:
    """Device-resident oriented point cloud (plade_cloud)."""

    def __init__(self, ctx, pos_nrm, handle=None):
        self.ctx = ctx
        if handle is not None:          # a cloud the library made (Context.upload_xyz)
            self.n, self.h = handle
            return
        a = _f32(pos_nrm)
        if a.ndim != 2 or a.shape[1] != 6:
            raise ValueError(f"Cloud: an (N, 6) array x y z nx ny nz is required, got shape {a.shape}")
        self.n = len(a)
        self.h = C.c_void_p()
        ctx._check(ctx.L.plade_cloud_upload(ctx.h, _ptr(a), self.n, C.byref(self.h)))

    def download(self):
        """plade_cloud_download: the cloud's rows x y z nx ny nz as an (N, 6) float32 array, whichever call made the cloud."""
        n = C.c_uint32(0)
        self.ctx._check(self.ctx.L.plade_cloud_download(self.ctx.h, self.h, None, 0, C.byref(n)))
        rows = np.empty((n.value, 6), np.float32)
        self.ctx._check(self.ctx.L.plade_cloud_download(self.ctx.h, self.h, _ptr(rows), n.value, C.byref(n)))
        return rows

    def free(self):
        if self.h:
            self.ctx.L.plade_cloud_free(self.ctx.h, self.h)
            self.h = C.c_void_p()


class Features:
    """Device-resident descriptor table (plade_features), made by Context.fpfh_dev(..., resident=True)."""

    def __init__(self, ctx, n, handle):
        self.ctx, self.n, self.h = ctx, n, handle

    def select(self, index):
        """plade_features_select: the rows `index` (ints below n) as a new resident table (free() it too)."""
        return self.ctx.select_features(self, index)

    def free(self):
        if self.h:
            self.ctx.L.plade_features_free(self.h)
            self.h = C.c_void_p()


class Context:
    """One HIP stream + scratch pools on one GPU (plade_ctx)."""

    def __init__(self, device=0, **params):
        self.L = load_library()
        self.h = C.c_void_p()
        rc = self.L.plade_ctx_create(device, C.byref(self.h))
        if rc != 0:
            raise PladeError(rc, "plade_ctx_create failed (no gfx950 device visible?)")
        self.params = Params()
        self.L.plade_default_params(C.byref(self.params))
        if params:
            self.set_params(**params)

    def close(self):
        if self.h:
            self.L.plade_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, allow=()):
        if rc != 0 and rc not in allow:
            raise PladeError(rc, self.L.plade_last_error(self.h).decode(errors="replace"))
        return rc

    def set_params(self, **kw):
        for k, v in kw.items():
            setattr(self.params, k, v)
        self._check(self.L.plade_set_params(self.h, C.byref(self.params)))

    def closest_points(self, u1, p1, u2, p2, mode=0):
        """Seam of ComputeNearstTwoPointsOfTwo3DLine (util.cpp:1167-1229) for n line pairs; mode 0 closed form, 1 / "svd_fp32"
        the reference's 9 x 9 float SVD solve.  Returns q1, q2 (n x 3), len (n, float64), ok (n, int32)."""
        u1, p1, u2, p2 = (_f32(a).reshape(-1, 3) for a in (u1, p1, u2, p2))
        n = len(u1)
        if not (len(p1) == len(u2) == len(p2) == n):
            raise ValueError("closest_points: the four arrays must hold the same number of rows")
        q1, q2 = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        ln, ok = np.zeros(n, np.float64), np.zeros(n, np.int32)
        self._check(self.L.plade_closest_points(self.h, 1 if mode in (1, "svd_fp32") else 0, _ptr(u1), _ptr(p1), _ptr(u2), _ptr(p2), n,
                                                _ptr(q1), _ptr(q2), _ptr(ln), _ptr(ok)))
        return q1, q2, ln, ok

    def lines_meet(self, v1, p1, v2, p2, mode=0):
        """Seam of ComputeIntersectionPointOf23DLine (util.cpp:1461-1500); returns points (n x 3), ok (n)."""
        v1, p1, v2, p2 = (_f32(a).reshape(-1, 3) for a in (v1, p1, v2, p2))
        n = len(v1)
        if not (len(p1) == len(v2) == len(p2) == n):
            raise ValueError("lines_meet: the four arrays must hold the same number of rows")
        out, ok = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        self._check(self.L.plade_lines_meet(self.h, 1 if mode in (1, "svd_fp32") else 0, _ptr(v1), _ptr(p1), _ptr(v2), _ptr(p2), n, _ptr(out), _ptr(ok)))
        return out, ok

    def sort_pairs(self, keys, vals, bits=None):
        """Diagnostic seam: the device-wide stable radix sort (radix_sort.hip).  keys uint32 or uint64."""
        k = np.ascontiguousarray(keys)
        assert k.dtype in (np.uint32, np.uint64)
        v = np.ascontiguousarray(vals, np.uint32)
        kb = k.dtype.itemsize
        ko, vo = np.empty_like(k), np.empty_like(v)
        self._check(self.L.plade_sort_pairs(self.h, k.ctypes.data_as(C.c_void_p), _ptr(v), len(k), kb,
                                            int(bits if bits is not None else 8 * kb), ko.ctypes.data_as(C.c_void_p), _ptr(vo)))
        return ko, vo

    def sort_segments(self, keys, vals, seg_off, bits=32):
        """The radix sort over up to 16 independent arrays in one launch sequence: segment s = [seg_off[s], seg_off[s + 1])."""
        k = np.ascontiguousarray(keys, np.uint32)
        v = np.ascontiguousarray(vals, np.uint32)
        so = np.ascontiguousarray(seg_off, np.uint32)
        ko, vo = np.empty_like(k), np.empty_like(v)
        self._check(self.L.plade_sort_segments(self.h, _ptr(k), _ptr(v), _ptr(so), len(so) - 1, int(bits), _ptr(ko), _ptr(vo)))
        return ko, vo

    def selftest_readback(self, n_ranges, words):
        """Test seam: n_ranges device arrays of `words` words through the library's device -> host hand-over; returns the number
        of words that arrived wrong."""
        bad = C.c_uint32(0)
        self._check(self.L.plade_selftest_readback(self.h, int(n_ranges), int(words), C.byref(bad)))
        return int(bad.value)

    # ---- seams -----------------------------------------------------------------------------
    def score_planes(self, pos_nrm, shape_index, planes, eps, cos_thresh, want_indices=False):
        pn = _f32(pos_nrm)
        pl = _f32(planes).reshape(-1, 4)
        si = _i32(shape_index) if shape_index is not None else None
        n, h = len(pn), len(pl)
        counts = np.zeros(h, np.uint32)
        idx = np.zeros((h, n), np.uint32) if want_indices else None
        self._check(self.L.plade_score_planes(self.h, _ptr(pn), _ptr(si), n, _ptr(pl), h, eps, cos_thresh,
                                              _ptr(counts), _ptr(idx), n if want_indices else 0))
        if want_indices:
            return counts, [idx[j, : counts[j]].astype(np.int32) for j in range(h)]
        return counts

    def score_planes_subset(self, pos_nrm, shape_index, sub_index, planes, eps, cos_thresh):
        """Seam S1a on a subset (k_r_score_sub): (counts per hypothesis, unassigned subset points)."""
        pn = _f32(pos_nrm)
        pl = _f32(planes).reshape(-1, 4)
        si = _i32(shape_index) if shape_index is not None else None
        sub = np.ascontiguousarray(sub_index, dtype=np.uint32)
        counts = np.zeros(len(pl), np.uint32)
        un = C.c_uint32()
        self._check(self.L.plade_score_planes_subset(self.h, _ptr(pn), _ptr(si), len(pn), _ptr(sub), len(sub), _ptr(pl), len(pl),
                                                     eps, cos_thresh, _ptr(counts), C.byref(un)))
        return counts, un.value

    def plane_component(self, pos_nrm, normal, point, idx, bitmap_eps, closing_filter, w_eps):
        """Seam S1c: (kept indices, LS fit[7], weighted score) of one plane candidate's score list."""
        pn, nn, pp, ii = _f32(pos_nrm), _f32(normal), _f32(point), _i32(idx)
        kept = np.zeros(max(len(ii), 1), np.int32)
        nk = C.c_uint32()
        fit = np.zeros(7, np.float32)
        ws = C.c_double()
        self._check(self.L.plade_plane_component(self.h, _ptr(pn), len(pn), _ptr(nn), _ptr(pp), _ptr(ii), len(ii),
                                                 C.c_float(bitmap_eps), int(closing_filter), C.c_float(w_eps), _ptr(kept),
                                                 C.byref(nk), _ptr(fit), C.byref(ws)))
        return kept[: nk.value].copy(), fit, ws.value

    def extract_planes(self, pos_nrm, min_support, dist_rel=0.005, bitmap_rel=0.02, cos_thresh=0.8,
                       overlook=0.001, max_planes=256):
        pn = _f32(pos_nrm)
        n = len(pn)
        planes = np.zeros((max_planes, 4), np.float32)
        offs = np.zeros(max_planes + 1, np.int32)
        idx = np.zeros(n, np.int32)
        npl = C.c_uint32()
        self._check(self.L.plade_extract_planes(self.h, _ptr(pn), n, min_support, dist_rel, bitmap_rel, cos_thresh,
                                                overlook, _ptr(planes), _ptr(offs), _ptr(idx), max_planes,
                                                C.byref(npl)))
        p = npl.value
        return planes[:p].copy(), offs[: p + 1].copy(), idx[: offs[p]].copy()

    def match_descriptors(self, qry, tgt, radius=0.04):
        q = _f32(qry).reshape(-1, 8)
        t = _f32(tgt).reshape(-1, 8)
        off = np.zeros(len(q) + 1, np.int64)
        total = C.c_uint64()
        self._check(self.L.plade_match_descriptors(self.h, _ptr(q), len(q), _ptr(t), len(t), radius, _ptr(off), None,
                                                   None, 0, C.byref(total)))
        m = total.value
        nbr = np.zeros(max(m, 1), np.uint32)
        d2 = np.zeros(max(m, 1), np.float64)
        self._check(self.L.plade_match_descriptors(self.h, _ptr(q), len(q), _ptr(t), len(t), radius, _ptr(off),
                                                   _ptr(nbr), _ptr(d2), m, C.byref(total)))
        return off, nbr[:m].astype(np.int32), d2[:m]

    def cluster_transforms(self, t_xyz, euler, dist_threshold, angle_gate):
        """Seam of the clustering stage (util.cpp:1245-1277): (cluster index per candidate, number of clusters)."""
        t, e = _f32(t_xyz).reshape(-1, 3), _f32(euler).reshape(-1, 3)
        out = np.full(len(t), -1, np.int32)
        n = C.c_uint32()
        self._check(self.L.plade_cluster_transforms(self.h, _ptr(t), _ptr(e), len(t), dist_threshold, angle_gate, _ptr(out), C.byref(n)))
        return out, n.value

    def penetration_filter(self, cand, src, tgt, length_threshold, angle_threshold, audit=False):
        """Seam of the penetration filter (util.cpp:450-519).  cand: K x 12 (R row-major, T); src / tgt: (coef P x 4, center P x 3,
        four P x 12, pts N x 3, off P + 1).  Returns the K flags; with audit=True (flags, items) with one PEN_ITEM record per item
        that reached the walks, every one evaluated in full."""
        cand = _f32(cand).reshape(-1, 12)
        K = len(cand)
        sides = []
        for coef, center, four, pts, off in (src, tgt):
            coef = _f32(coef).reshape(-1, 4)
            off = np.ascontiguousarray(off, np.uint32)
            if len(off) != len(coef) + 1:
                raise ValueError("penetration_filter: off must hold P + 1 offsets")
            pts = _f32(pts).reshape(-1, 3)
            if len(pts) < int(off[-1]):
                raise ValueError("penetration_filter: offsets reach past the plane clouds")
            sides.append((coef, _f32(center).reshape(len(coef), 3), _f32(four).reshape(len(coef), 12), pts, off))
        (sc, sce, sf, sp, so), (tc, tce, tf, tp, to) = sides
        flags = np.zeros(K, np.int32)
        cap = K * len(sc) * len(tc) if audit else 0
        items = np.zeros(max(cap, 1), PEN_ITEM) if audit else None
        n = C.c_uint64()
        self._check(self.L.plade_penetration_filter(self.h, _ptr(cand), K, _ptr(sc), _ptr(sce), _ptr(sf), _ptr(sp), _ptr(so), len(sc),
                                                    _ptr(tc), _ptr(tce), _ptr(tf), _ptr(tp), _ptr(to), len(tc),
                                                    C.c_float(length_threshold), C.c_float(angle_threshold), _ptr(flags),
                                                    _ptr(items) if audit else None, cap, C.byref(n)))
        return (flags, items[: n.value].copy()) if audit else flags

    def overlap_counts(self, src_ds, tgt_ds, T, centers, src_radius, inlier_dist):
        s, t = _f32(src_ds), _f32(tgt_ds)
        T = _f32(T).reshape(-1, 16)
        c = _f32(centers).reshape(-1, 3)
        counts = np.zeros(len(T), np.int32)
        self._check(self.L.plade_overlap_counts(self.h, _ptr(s), len(s), _ptr(t), len(t), _ptr(T), len(T), _ptr(c),
                                                src_radius, inlier_dist, _ptr(counts)))
        return counts

    def average_spacing(self, pts, k=6, samples=10000):
        a = _f32(pts)
        out = C.c_float()
        self._check(self.L.plade_average_spacing(self.h, _ptr(a), len(a), a.shape[1], k, samples, C.byref(out)))
        return np.float32(out.value)

    def voxel_downsample(self, pts, leaf):
        a = _f32(pts)
        out = np.zeros((len(a), 3), np.float32)
        n = C.c_uint32()
        self._check(self.L.plade_voxel_downsample(self.h, _ptr(a), len(a), a.shape[1], leaf, _ptr(out), C.byref(n)))
        return out[: n.value].copy()

    # ---- registration() overloads (code/PLADE/plade.h) --------------------------------------
    def registration_planes(self, tgt, src, tgt_planes, src_planes):
        """plade.h:74.  Returns (ok, T 4x4)."""
        tgt, src = _f32(tgt), _f32(src)
        tc, to, ti = _f32(tgt_planes[0]), _i32(tgt_planes[1]), _i32(tgt_planes[2])
        sc, so, si = _f32(src_planes[0]), _i32(src_planes[1]), _i32(src_planes[2])
        T = np.zeros((4, 4), np.float32)
        rc = self._check(self.L.plade_registration_planes(self.h, _ptr(tgt), len(tgt), _ptr(src), len(src), _ptr(tc),
                                                          _ptr(to), _ptr(ti), len(tc), _ptr(sc), _ptr(so), _ptr(si),
                                                          len(sc), _ptr(T)), allow=(PLADE_EFAIL,))
        return rc == 0, T

    def registration(self, tgt, src):
        """plade.h:58.  Returns (ok, T 4x4)."""
        tgt, src = _f32(tgt), _f32(src)
        self._check_cloud(tgt, "registration"); self._check_cloud(src, "registration")
        T = np.zeros((4, 4), np.float32)
        rc = self._check(self.L.plade_registration(self.h, _ptr(tgt), len(tgt), _ptr(src), len(src), _ptr(T)),
                         allow=(PLADE_EFAIL,))
        return rc == 0, T

    def registration_next(self, tgt, src, next_tgt=None, next_src=None):
        """plade.h:58 in batch mode: registers (tgt, src) and starts the upload of the pair the next call will be handed.
        The arrays must be C-contiguous float32 and stay alive and unchanged until that call."""
        for a in (tgt, src, next_tgt, next_src):
            if a is not None:
                self._check_cloud(a, "registration_next")
        T = np.zeros((4, 4), np.float32)
        nt, ns = (next_tgt, next_src) if next_tgt is not None and next_src is not None else (None, None)
        self._announced = [(nt, ns)] if nt is not None else None      # alive until the next call consumes or drops them
        rc = self._check(self.L.plade_registration_next(self.h, _ptr(tgt), len(tgt), _ptr(src), len(src), _ptr(nt),
                                                        len(nt) if nt is not None else 0, _ptr(ns),
                                                        len(ns) if ns is not None else 0, _ptr(T)), allow=(PLADE_EFAIL,))
        return rc == 0, T

    @staticmethod
    def _cloud_table(arrs):
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        ns = (C.c_uint32 * len(arrs))(*[len(a) for a in arrs])
        return ptrs, ns

    @staticmethod
    def _check_cloud(a, what):
        """The library reads len(a) x 6 floats behind the pointer: anything else than a C-contiguous (N, 6) float32 array would
        make it read past the buffer (python -O strips asserts, so this raises)."""
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != 6 or not a.flags["C_CONTIGUOUS"]:
            raise ValueError(f"{what}: a C-contiguous float32 array of shape (N, 6) is required, got "
                             f"{getattr(a, 'dtype', type(a))} {getattr(a, 'shape', '')}")
        if len(a) == 0:
            raise ValueError(f"{what}: empty cloud")

    def registration_pairs(self, pairs, next_pairs=None, raise_on_error=True):
        """plade.h:58 in batch mode, one GROUP of 1..8 pairs per call (plade_registration_pairs): pairs = [(tgt, src), ...];
        next_pairs = the pairs the next call on this context will be handed (their upload is started now).  The arrays must be
        C-contiguous (N, 6) float32 and stay alive and UNCHANGED until that call (the context keeps a reference to them until
        then; changing their contents meanwhile is the caller's race).  Returns [(ok, T 4x4), ...]; with raise_on_error=False a
        pair the library refused (status other than OK / EFAIL) does not raise: [(status, T), ...] with the PLADE_E* codes."""
        if not 1 <= len(pairs) <= 8 or (next_pairs and len(next_pairs) > 8):
            raise ValueError("registration_pairs: a group holds 1..8 pairs")
        for pr in list(pairs) + list(next_pairs or []):
            for a in pr[:2]:
                self._check_cloud(a, "registration_pairs")
        self._announced = [(p[0], p[1]) for p in next_pairs] if next_pairs else None   # alive until the next call consumes or drops them
        k = len(pairs)
        tp, tn = self._cloud_table([p[0] for p in pairs])
        sp, sn = self._cloud_table([p[1] for p in pairs])
        nk = len(next_pairs) if next_pairs else 0
        if nk:
            ntp, ntn = self._cloud_table([p[0] for p in next_pairs])
            nsp, nsn = self._cloud_table([p[1] for p in next_pairs])
        else:
            ntp = ntn = nsp = nsn = None
        T = np.zeros((k, 4, 4), np.float32)
        st = np.zeros(k, np.int32)
        self._check(self.L.plade_registration_pairs(self.h, k, tp, tn, sp, sn, nk, ntp, ntn, nsp, nsn, _ptr(T), _ptr(st)))
        if not raise_on_error:
            return [(int(st[i]), T[i].copy()) for i in range(k)]
        for i in range(k):
            if st[i] not in (0, PLADE_EFAIL):
                raise PladeError(int(st[i]), self.pair_error(i))
        return [(bool(st[i] == 0), T[i].copy()) for i in range(k)]

    def registration_pairs_dev(self, clouds, raise_on_error=True):
        """The same group call on resident clouds: clouds = [(tgt Cloud, src Cloud), ...]."""
        k = len(clouds)
        if not 1 <= k <= 8:
            raise ValueError("registration_pairs_dev: a group holds 1..8 pairs")
        tp = (C.c_void_p * k)(*[c[0].h.value for c in clouds])
        sp = (C.c_void_p * k)(*[c[1].h.value for c in clouds])
        T = np.zeros((k, 4, 4), np.float32)
        st = np.zeros(k, np.int32)
        self._check(self.L.plade_registration_pairs_dev(self.h, k, tp, sp, _ptr(T), _ptr(st)))
        if not raise_on_error:
            return [(int(st[i]), T[i].copy()) for i in range(k)]
        for i in range(k):
            if st[i] not in (0, PLADE_EFAIL):
                raise PladeError(int(st[i]), self.pair_error(i))
        return [(bool(st[i] == 0), T[i].copy()) for i in range(k)]

    def set_candidate_shard(self, rank, world, exchange=None, min_candidates=0):
        """Second sharding axis (plade_set_candidate_shard): with world > 1 this context scores only candidates k % world == rank
        of a registration's verification and calls exchange(values: int32 numpy view of all words, rank, world), which must fill
        in the other ranks' words (an all-gather).  world <= 1 switches it off."""
        if world <= 1 or exchange is None:
            self._shard_cb = None
            self._check(self.L.plade_set_candidate_shard(self.h, 0, 1, 0, EXCHANGE_FN(0), None))
            return

        def cb(user, values, count, r, w):
            try:
                exchange(np.ctypeslib.as_array(values, shape=(count,)), int(r), int(w))
                return 0
            except Exception:      # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return -1
        self._shard_cb = EXCHANGE_FN(cb)      # keep the trampoline alive
        self._check(self.L.plade_set_candidate_shard(self.h, int(rank), int(world), int(min_candidates), self._shard_cb, None))

    def diag_launches(self, count, blocks=1, mbytes=0):
        """Diagnostic: `count` launches of an empty (or memory-streaming) kernel on this context's stream, then a wait."""
        self._check(self.L.plade_diag_launches(self.h, int(count), int(blocks), int(mbytes)))

    def _pair_handle(self, index):
        h = self.L.plade_pair_ctx(self.h, int(index))
        if not h:
            raise PladeError(PLADE_EINVAL, f"no pair {index} on this context")
        return C.c_void_p(h)

    def pair_error(self, index):
        return self.L.plade_last_error(self._pair_handle(index)).decode(errors="replace")

    def registration_minsupport(self, tgt, src, ms_t, ms_s):
        """plade.h:91."""
        tgt, src = _f32(tgt), _f32(src)
        T = np.zeros((4, 4), np.float32)
        rc = self._check(self.L.plade_registration_minsupport(self.h, _ptr(tgt), len(tgt), _ptr(src), len(src), ms_t,
                                                              ms_s, _ptr(T)), allow=(PLADE_EFAIL,))
        return rc == 0, T

    def upload(self, pos_nrm):
        return Cloud(self, pos_nrm)

    # ---- clouds without normals -------------------------------------------------------------
    def estimate_normals(self, xyz, k=16, viewpoint=(0.0, 0.0, 0.0), curvature=False, neighbours=False):
        """plade_estimate_normals: k-nearest-neighbour PCA normals of an (N, 3) cloud (or the x y z columns of wider rows),
        oriented toward `viewpoint`.  Returns the (N, 6) float32 array x y z nx ny nz; with curvature / neighbours also the
        (N,) float32 curvature and the (N, k) int32 neighbour lists (ascending (distance, index), the point itself included;
        -1 behind the min(k, N) entries).  NaN normal and curvature where fewer than 3 points or only coincident points are
        the neighbourhood."""
        a, n, stride = _xyz_view(xyz)
        v = _viewpoint(viewpoint)
        out = np.empty((n, 6), np.float32)
        curv = np.empty(n, np.float32) if curvature else None
        nbr = np.empty((n, max(int(k), 0)), np.int32) if neighbours else None
        self._check(self.L.plade_estimate_normals(self.h, _ptr(a), n, stride, int(k), _ptr(v), _ptr(out), _ptr(curv), _ptr(nbr)))
        res = (out,) + ((curv,) if curvature else ()) + ((nbr,) if neighbours else ())
        return res[0] if len(res) == 1 else res

    def upload_xyz(self, xyz, k=16, viewpoint=(0.0, 0.0, 0.0)):
        """plade_cloud_upload_xyz: upload an (N, 3) cloud and estimate its normals into a resident Cloud (the point data makes no host round
        trip) for registration_dev / registration_pairs_dev."""
        a, n, stride = _xyz_view(xyz)
        v = _viewpoint(viewpoint)
        h = C.c_void_p()
        self._check(self.L.plade_cloud_upload_xyz(self.h, _ptr(a), n, stride, int(k), _ptr(v), C.byref(h)))
        return Cloud(self, None, handle=(n, h))

    # ---- fine alignment ----------------------------------------------------------------------
    def _refine(self, call, T, params, model):
        T_in = _f32(T).reshape(4, 4).copy()
        prm = _refine_params(params, model)
        T_out = np.zeros((4, 4), np.float32)
        res = model[1]()
        rc = call(T_in, prm, T_out, res)
        info = _refine_info(res)
        if rc != 0:
            err = PladeError(rc, self.L.plade_last_error(self.h).decode(errors="replace"))
            err.info, err.T = info, T_out
            raise err
        return T_out, info

    def refine_icp(self, tgt, src, T, **icp_params):
        """plade_refine_icp: point-to-plane ICP of the (N, 6) source onto the (M, 6) target from the 4 x 4 source -> target T.
        Returns (T_out, info), info = the plade_icp_result fields as a dict plus `reason` (None, "too few correspondences",
        "degenerate").  A failed refinement raises PladeError (code PLADE_EFAIL, with .info and .T = T_in)."""
        tgt, src = _f32(tgt), _f32(src)
        self._check_cloud(tgt, "refine_icp"); self._check_cloud(src, "refine_icp")
        return self._refine(lambda T_in, prm, T_out, res: self.L.plade_refine_icp(
            self.h, _ptr(tgt), len(tgt), _ptr(src), len(src), _ptr(T_in), C.byref(prm), _ptr(T_out), C.byref(res)), T, icp_params, _ICP)

    def refine_icp_dev(self, tgt_cloud, src_cloud, T, **icp_params):
        """plade_refine_icp_dev: refine_icp on resident clouds (upload, upload_xyz); bit-identical to refine_icp."""
        return self._refine(lambda T_in, prm, T_out, res: self.L.plade_refine_icp_dev(
            self.h, tgt_cloud.h, src_cloud.h, _ptr(T_in), C.byref(prm), _ptr(T_out), C.byref(res)), T, icp_params, _ICP)

    def icp_linearize(self, tgt, src_xyz, T, dist, center=None):
        """plade_icp_linearize (test seam): one match + linearise pass of the ICP at stage distance `dist` with the fp64 4 x 4 T on
        every point of src_xyz (no sample), J about the fp64 point `center` (None: the origin, J = [p x n, n]; the refinement
        linearises about c_k = T_k s-bar, s-bar = the fp64 mean of its sample).  Returns (corr, moments): corr (N,) int32 = the target index or -1, moments (29,)
        float64 = J^T J (upper triangle, row-major), J^T r, sum r^2, count."""
        tgt = _f32(tgt)
        self._check_cloud(tgt, "icp_linearize")
        a, n, stride = _xyz_view(src_xyz)
        T64 = np.ascontiguousarray(T, dtype=np.float64).reshape(4, 4)
        c64 = np.ascontiguousarray((0.0, 0.0, 0.0) if center is None else center, dtype=np.float64).reshape(3)
        corr = np.empty(n, np.int32)
        mom = np.zeros(29, np.float64)
        self._check(self.L.plade_icp_linearize(self.h, _ptr(tgt), len(tgt), _ptr(a), n, stride, _ptr(T64), _ptr(c64), float(dist),
                                               _ptr(corr), _ptr(mom)))
        return corr, mom

    def refine_gicp(self, tgt, src, T, **gicp_params):
        """plade_refine_gicp: plane-to-plane (generalized) ICP of the (N, 6) source onto the (M, 6) target from the 4 x 4 source ->
        target T; both clouds' normals are read.  Parameters: those of refine_icp and epsilon (1: point-to-point ICP).  Returns
        (T_out, info), info = the plade_gicp_result fields as a dict plus `reason` (None, "too few correspondences", "degenerate").
        A failed refinement raises PladeError (code PLADE_EFAIL, with .info and .T = T_in)."""
        tgt, src = _f32(tgt), _f32(src)
        self._check_cloud(tgt, "refine_gicp"); self._check_cloud(src, "refine_gicp")
        return self._refine(lambda T_in, prm, T_out, res: self.L.plade_refine_gicp(
            self.h, _ptr(tgt), len(tgt), _ptr(src), len(src), _ptr(T_in), C.byref(prm), _ptr(T_out), C.byref(res)), T, gicp_params, _GICP)

    def refine_gicp_dev(self, tgt_cloud, src_cloud, T, **gicp_params):
        """plade_refine_gicp_dev: refine_gicp on resident clouds (upload, upload_xyz); bit-identical to refine_gicp."""
        return self._refine(lambda T_in, prm, T_out, res: self.L.plade_refine_gicp_dev(
            self.h, tgt_cloud.h, src_cloud.h, _ptr(T_in), C.byref(prm), _ptr(T_out), C.byref(res)), T, gicp_params, _GICP)

    def gicp_linearize(self, tgt, src, T, dist, epsilon=0.0, center=None):
        """plade_gicp_linearize (test seam): one match + linearise pass of the plane-to-plane ICP at stage distance `dist` with the
        fp64 4 x 4 T on every row of the (N, 6) source (no sample), J about the fp64 point `center` (None: the origin); epsilon 0 =
        1e-3.  Returns (corr, moments): corr (N,) int32 = the target index or -1, moments (30,) float64 = J^T M J (upper triangle,
        row-major), J^T M e, sum e^T M e, sum e . e, count."""
        tgt, src = _f32(tgt), _f32(src)
        self._check_cloud(tgt, "gicp_linearize"); self._check_cloud(src, "gicp_linearize")
        T64 = np.ascontiguousarray(T, dtype=np.float64).reshape(4, 4)
        c64 = np.ascontiguousarray((0.0, 0.0, 0.0) if center is None else center, dtype=np.float64).reshape(3)
        corr = np.empty(len(src), np.int32)
        mom = np.zeros(30, np.float64)
        self._check(self.L.plade_gicp_linearize(self.h, _ptr(tgt), len(tgt), _ptr(src), len(src), _ptr(T64), _ptr(c64), float(dist),
                                                float(epsilon), _ptr(corr), _ptr(mom)))
        return corr, mom

    # ---- cloud-to-cloud distances ------------------------------------------------------------
    def _distances(self, call, n, max_dist, T, per_point):
        T_in = None if T is None else _f32(T).reshape(4, 4).copy()
        idx = np.empty(n, np.int32) if per_point else None
        d2 = np.empty(n, np.float32) if per_point else None
        plane = np.empty(n, np.float32) if per_point else None
        summ = DistanceSummary()
        self._check(call(_ptr(T_in), float(max_dist), _ptr(idx), _ptr(d2), _ptr(plane), C.byref(summ)))
        return idx, d2, plane, {k: getattr(summ, k) for k, _ in DistanceSummary._fields_}

    def cloud_distances(self, tgt, src, max_dist, T=None, per_point=True):
        """plade_cloud_distances: the exact nearest (M, 6) target point of every point of src (N x 3, or the x y z columns of
        wider rows) after the 4 x 4 source -> target T (None: the identity), bounded by max_dist.  Returns (idx, d2, plane,
        summary): idx (N,) int32 (-1: nothing closer than max_dist), d2 (N,) float32 squared distances (+inf), plane (N,) float32
        signed point-to-plane distances (NaN), all None when per_point is False, and the plade_distance_summary fields as a dict."""
        tgt = _f32(tgt)
        self._check_cloud(tgt, "cloud_distances")
        a, n, stride = _xyz_view(src)
        return self._distances(lambda T_in, d, i, d2, pl, summ: self.L.plade_cloud_distances(
            self.h, _ptr(tgt), len(tgt), _ptr(a), n, stride, T_in, d, i, d2, pl, summ), n, max_dist, T, per_point)

    def cloud_distances_dev(self, tgt_cloud, src_cloud, max_dist, T=None, per_point=True):
        """plade_cloud_distances_dev: cloud_distances on resident clouds (upload, upload_xyz); bit-identical results."""
        return self._distances(lambda T_in, d, i, d2, pl, summ: self.L.plade_cloud_distances_dev(
            self.h, tgt_cloud.h, src_cloud.h, T_in, d, i, d2, pl, summ), src_cloud.n, max_dist, T, per_point)

    def evaluate_registration(self, tgt, src, T, max_dist):
        """Registration quality of T (source -> target) at max_dist: the summary dict of cloud_distances, with no per-point
        outputs (fitness = the share of source points within max_dist of the target, rmse of their distances, ...)."""
        return self.cloud_distances(tgt, src, max_dist, T=T, per_point=False)[3]

    # ---- outlier removal -------------------------------------------------------------------------
    def remove_outliers(self, points, mode="statistical", k=None, alpha=None, radius=None, min_neighbours=None, per_point=True):
        """plade_filter_outliers: the statistical (k nearest neighbours, threshold mu + alpha sigma of their mean distances;
        defaults k = 16, alpha = 1) or radius (at least min_neighbours other points closer than radius) outlier filter of an
        (N, >= 3) float32 array whose first three columns are x y z.  Returns (filtered, kept_index, info): the kept rows in
        their original order with every column copied bit for bit, their original indices (uint32, ascending), and a dict with
        n, kept, mu, sigma, threshold (NaN in radius mode), keep (N bools) and -- with per_point -- mean_dist (N float64,
        statistical) or count (N uint32, radius; without per_point a count may stop at min_neighbours)."""
        a, n, stride = _xyz_view(points)
        prm = _outlier_params(mode, k, alpha, radius, min_neighbours)
        stat = prm.mode == PLADE_OUTLIER_STATISTICAL
        keep = np.zeros(n, np.uint8)
        kept = np.empty(n, np.uint32)
        rows = np.empty((n, stride), np.float32)
        mean = np.empty(n, np.float64) if per_point and stat else None
        count = np.empty(n, np.uint32) if per_point and not stat else None
        summ = OutlierSummary()
        self._check(self.L.plade_filter_outliers(self.h, _ptr(a), n, stride, C.byref(prm), _ptr(keep), _ptr(kept), _ptr(rows),
                                                 _ptr(mean), _ptr(count), C.byref(summ)))
        info = _outlier_info(summ, keep)
        if mean is not None:
            info["mean_dist"] = mean
        if count is not None:
            info["count"] = count
        return rows[:summ.kept].copy(), kept[:summ.kept].copy(), info

    def remove_outliers_dev(self, cloud, mode="statistical", k=None, alpha=None, radius=None, min_neighbours=None, info=False):
        """plade_cloud_filter_outliers_dev: remove_outliers on a resident cloud (upload, upload_xyz) into a new resident Cloud;
        the point data makes no host round trip.  With info also (kept_index, info dict) as remove_outliers gives them (no
        per-point values): the same bits.  Raises PladeError (PLADE_EFAIL) when nothing is kept."""
        prm = _outlier_params(mode, k, alpha, radius, min_neighbours)
        keep = np.zeros(cloud.n, np.uint8) if info else None
        kept = np.empty(cloud.n, np.uint32) if info else None
        summ = OutlierSummary()
        h = C.c_void_p()
        self._check(self.L.plade_cloud_filter_outliers_dev(self.h, cloud.h, C.byref(prm), C.byref(h), _ptr(keep), _ptr(kept), C.byref(summ)))
        out = Cloud(self, None, handle=(int(summ.kept), h))
        return (out, kept[:summ.kept].copy(), _outlier_info(summ, keep)) if info else out

    # ---- connected components --------------------------------------------------------------------
    def connected_components(self, points, radius, min_size=1, max_size=0, keep_largest=0):
        """plade_label_components: the connected components of the graph "closer than radius" (fp32 squared distance, strict <)
        of an (N, >= 3) float32 array whose first three columns are x y z, and the points of the components that pass min_size <=
        size <= max_size (0: no upper bound), with keep_largest = m > 0 only of the m largest passing ones (ties: the smaller id).
        Returns (filtered, kept_index, info): the kept rows in their original order with every column copied bit for bit, their
        original indices (uint32, ascending), and a dict with n, components, kept_components, kept, largest, label (N int32: ids
        in ascending order of a component's smallest index), size (components uint32) and keep (N bools)."""
        a, n, stride = _xyz_view(points)
        prm = _component_params(radius, min_size, max_size, keep_largest)
        label = np.empty(n, np.int32)
        size = np.empty(n, np.uint32)
        keep = np.zeros(n, np.uint8)
        kept = np.empty(n, np.uint32)
        rows = np.empty((n, stride), np.float32)
        summ = ComponentSummary()
        self._check(self.L.plade_label_components(self.h, _ptr(a), n, stride, C.byref(prm), _ptr(label), _ptr(size), _ptr(keep),
                                                  _ptr(kept), _ptr(rows), C.byref(summ)))
        return rows[:summ.kept].copy(), kept[:summ.kept].copy(), _component_info(summ, label, size, keep)

    def filter_components_dev(self, cloud, radius, min_size=1, max_size=0, keep_largest=0, info=False):
        """plade_cloud_filter_components_dev: connected_components on a resident cloud (upload, upload_xyz) into a new resident
        Cloud of the kept points; the point data makes no host round trip.  With info also (kept_index, info dict): the same
        bits as connected_components gives (label, no size and keep arrays).  Raises PladeError (PLADE_EFAIL) when nothing is
        kept."""
        prm = _component_params(radius, min_size, max_size, keep_largest)
        label = np.empty(cloud.n, np.int32) if info else None
        kept = np.empty(cloud.n, np.uint32) if info else None
        summ = ComponentSummary()
        h = C.c_void_p()
        self._check(self.L.plade_cloud_filter_components_dev(self.h, cloud.h, C.byref(prm), C.byref(h), _ptr(label), _ptr(kept),
                                                             C.byref(summ)))
        out = Cloud(self, None, handle=(int(summ.kept), h))
        return (out, kept[:summ.kept].copy(), _component_info(summ, label, None, None)) if info else out

    # ---- DBSCAN ----------------------------------------------------------------------------------
    def dbscan(self, points, radius, min_points=4, min_size=1, max_size=0, keep_largest=0):
        """plade_cluster_dbscan: the DBSCAN clusters of an (N, >= 3) float32 array whose first three columns are x y z.  A point
        with at least min_points points closer than radius (fp32 squared distance, strict <, itself included) is a core point; the
        clusters are the connected components of the core points; a non-core point with a core point closer than radius is a
        border point and joins the cluster of the core neighbour with the smallest (distance, index); the rest is noise.  The
        clusters are selected by size like connected_components' (min_size, max_size, keep_largest).  Returns (filtered,
        kept_index, info): the kept rows in their original order with every column copied bit for bit, their original indices
        (uint32, ascending), and a dict with n, clusters, core, border, noise, kept_clusters, kept, largest, label (N int32: ids in
        ascending order of a cluster's smallest core index, -1 noise), kind (N uint8: 0 noise, 1 border, 2 core), size (clusters
        uint32) and keep (N bools)."""
        a, n, stride = _xyz_view(points)
        prm = _dbscan_params(radius, min_points, min_size, max_size, keep_largest)
        label = np.empty(n, np.int32)
        kind = np.empty(n, np.uint8)
        size = np.empty(n, np.uint32)
        keep = np.zeros(n, np.uint8)
        kept = np.empty(n, np.uint32)
        rows = np.empty((n, stride), np.float32)
        summ = DbscanSummary()
        self._check(self.L.plade_cluster_dbscan(self.h, _ptr(a), n, stride, C.byref(prm), _ptr(label), _ptr(kind), _ptr(size), _ptr(keep),
                                                _ptr(kept), _ptr(rows), C.byref(summ)))
        return rows[:summ.kept].copy(), kept[:summ.kept].copy(), _dbscan_info(summ, label, kind, size, keep)

    def dbscan_dev(self, cloud, radius, min_points=4, min_size=1, max_size=0, keep_largest=0, info=False):
        """plade_cloud_cluster_dbscan_dev: dbscan on a resident cloud (upload, upload_xyz) into a new resident Cloud of the kept
        points; the point data makes no host round trip.  With info also (kept_index, info dict): the same bits as dbscan gives
        (label and kind, no size and keep arrays).  Raises PladeError (PLADE_EFAIL) when nothing is kept."""
        prm = _dbscan_params(radius, min_points, min_size, max_size, keep_largest)
        label = np.empty(cloud.n, np.int32) if info else None
        kind = np.empty(cloud.n, np.uint8) if info else None
        kept = np.empty(cloud.n, np.uint32) if info else None
        summ = DbscanSummary()
        h = C.c_void_p()
        self._check(self.L.plade_cloud_cluster_dbscan_dev(self.h, cloud.h, C.byref(prm), C.byref(h), _ptr(label), _ptr(kind), _ptr(kept),
                                                          C.byref(summ)))
        out = Cloud(self, None, handle=(int(summ.kept), h))
        return (out, kept[:summ.kept].copy(), _dbscan_info(summ, label, kind, None, None)) if info else out

    # ---- subsampling to a minimum spacing ---------------------------------------------------------
    def subsample(self, points, spacing, seed=0, per_point=True):
        """plade_subsample_spacing: the subset of an (N, >= 3) float32 array (first three columns x y z) in which no two kept points
        are closer than spacing (fp32 squared distance, strict <) and every dropped point has a kept point closer than spacing:
        the greedy walk in the order of the hashed keys (mix64(mix64(seed) ^ i), i), an exact set that depends on the points,
        spacing and seed only.  Returns (subset, kept_index, info): the kept rows in their original order with every column copied
        bit for bit, their original indices (uint32, ascending), and a dict with n, kept, rounds and -- with per_point -- keep (N
        bools) and round (N uint32: the synchronous round that decided each point)."""
        a, n, stride = _xyz_view(points)
        prm = _subsample_params(spacing, seed)
        keep = np.zeros(n, np.uint8) if per_point else None
        rnd = np.empty(n, np.uint32) if per_point else None
        kept = np.empty(n, np.uint32)
        rows = np.empty((n, stride), np.float32)
        summ = SubsampleSummary()
        self._check(self.L.plade_subsample_spacing(self.h, _ptr(a), n, stride, C.byref(prm), _ptr(keep), _ptr(kept), _ptr(rows),
                                                   _ptr(rnd), C.byref(summ)))
        return rows[:summ.kept].copy(), kept[:summ.kept].copy(), _subsample_info(summ, keep, rnd)

    def subsample_dev(self, cloud, spacing, seed=0, info=False):
        """plade_cloud_subsample_dev: subsample on a resident cloud (upload, upload_xyz) into a new resident Cloud of the kept
        points; the point data makes no host round trip.  With info also (kept_index, info dict) as subsample gives them (keep,
        no round array): the same bits.  At least one point is always kept."""
        prm = _subsample_params(spacing, seed)
        keep = np.zeros(cloud.n, np.uint8) if info else None
        kept = np.empty(cloud.n, np.uint32) if info else None
        summ = SubsampleSummary()
        h = C.c_void_p()
        self._check(self.L.plade_cloud_subsample_dev(self.h, cloud.h, C.byref(prm), C.byref(h), _ptr(keep), _ptr(kept), C.byref(summ)))
        out = Cloud(self, None, handle=(int(summ.kept), h))
        return (out, kept[:summ.kept].copy(), _subsample_info(summ, keep, None)) if info else out

    # ---- consistent normal orientation ------------------------------------------------------------
    def orient_consistent(self, pos_nrm, radius, mode=ORIENT_VOTE, inward=0, viewpoint=(0.0, 0.0, 0.0), direction=(0.0, 0.0, 1.0),
                          per_point=True):
        """plade_orient_normals: the rows of an (N, 6) float32 array x y z nx ny nz with their normals on one side of the surface
        per component of the graph "closer than radius" (fp32 squared distance, strict <): the flips follow the minimum spanning
        forest of the edge keys 0x7F800000 - bits(|n_i . n_j|) ordered by (key, min index, max index); the side is the majority
        of the viewpoint test (mode ORIENT_VOTE) or the normal of the extreme point along `direction` having a component along it
        (ORIENT_EXTREME); inward=1 inverts it.  Points whose normal is not finite (or above 1e18) are left as they are.  Returns
        (rows, info): the rows with the flipped normals' sign bits toggled and every other float copied bit for bit, and a dict with
        n, unoriented, components, flipped, tree_edges, rounds, tree_key_sum and -- with per_point -- flip (N bools) and label (N
        int32, the component, -1 where the normal is invalid)."""
        a = _f32(pos_nrm)
        if a.ndim != 2 or a.shape[1] != 6:
            raise ValueError(f"an (N, 6) array x y z nx ny nz is required, got shape {a.shape}")
        n = len(a)
        prm = _orient_params(radius, mode, inward, viewpoint, direction)
        rows = np.empty((n, 6), np.float32)
        flip = np.zeros(n, np.uint8) if per_point else None
        label = np.empty(n, np.int32) if per_point else None
        summ = OrientSummary()
        self._check(self.L.plade_orient_normals(self.h, _ptr(a), n, C.byref(prm), _ptr(rows), _ptr(flip), _ptr(label), C.byref(summ)))
        return rows, _orient_info(summ, flip, label)

    def orient_consistent_dev(self, cloud, radius, mode=ORIENT_VOTE, inward=0, viewpoint=(0.0, 0.0, 0.0), direction=(0.0, 0.0, 1.0),
                              info=False):
        """plade_cloud_orient_normals_dev: orient_consistent on a resident cloud (upload, upload_xyz) into a new resident Cloud of
        the same points; the point data makes no host round trip.  With info also the info dict as orient_consistent gives it: the
        same bits."""
        prm = _orient_params(radius, mode, inward, viewpoint, direction)
        flip = np.zeros(cloud.n, np.uint8) if info else None
        label = np.empty(cloud.n, np.int32) if info else None
        summ = OrientSummary()
        h = C.c_void_p()
        self._check(self.L.plade_cloud_orient_normals_dev(self.h, cloud.h, C.byref(prm), C.byref(h), _ptr(flip), _ptr(label), C.byref(summ)))
        out = Cloud(self, None, handle=(int(summ.n), h))
        return (out, _orient_info(summ, flip, label)) if info else out

    # ---- smoothing ---------------------------------------------------------------------------------
    def smooth_cloud(self, points, radius, min_neighbours=None, viewpoint=(0.0, 0.0, 0.0), normals=True, per_point=True, moments=False):
        """plade_smooth_cloud: the moving-least-squares plane projection of an (N, >= 3) float32 array whose first three columns
        are x y z -- every point with at least min_neighbours (default 6, itself included) points closer than radius goes to the
        weighted plane fit of that neighbourhood (weights (1 - d^2 / r^2)^2).  Returns (rows, info): rows (N, 6) float32, the
        smoothed x y z and -- with normals -- the fit's normals toward `viewpoint` (NaN where unfitted; NaN everywhere without
        normals); info: a dict with n, fitted, rms and max (of |displacement| over the fitted points), max_count and -- with
        per_point -- curvature (N float32, NaN where unfitted), displacement (N float64), count (N uint32: the neighbourhood, the
        point itself included), fitted_mask (N bools), and with moments the (N, 10) float64 sums W, S, M of the fit."""
        a, n, stride = _xyz_view(points)
        prm = _smooth_params(radius, min_neighbours, viewpoint)
        xyz = np.empty((n, 3), np.float32)
        nrm = np.empty((n, 3), np.float32) if normals else None
        curv = np.empty(n, np.float32) if per_point else None
        disp = np.empty(n, np.float64) if per_point else None
        count = np.empty(n, np.uint32) if per_point else None
        fitted = np.zeros(n, np.uint8) if per_point else None
        mom = np.empty((n, 10), np.float64) if moments else None
        summ = SmoothSummary()
        self._check(self.L.plade_smooth_cloud(self.h, _ptr(a), n, stride, C.byref(prm), _ptr(xyz), _ptr(nrm), _ptr(curv), _ptr(disp),
                                              _ptr(count), _ptr(fitted), _ptr(mom), C.byref(summ)))
        rows = np.full((n, 6), np.nan, np.float32)
        rows[:, :3] = xyz
        if normals:
            rows[:, 3:] = nrm
        info = _smooth_info(summ)
        if per_point:
            info.update(curvature=curv, displacement=disp, count=count, fitted_mask=fitted.view(np.bool_))
        if moments:
            info["moments"] = mom
        return rows, info

    def smooth_cloud_dev(self, cloud, radius, min_neighbours=None, viewpoint=(0.0, 0.0, 0.0), fit_normals=True, info=False):
        """plade_cloud_smooth_dev: smooth_cloud on a resident cloud (upload, upload_xyz) into a new resident Cloud of the same
        points; the point data makes no host round trip, the positions are the bits of smooth_cloud.  fit_normals: the normal
        columns are the fit's (NaN where unfitted); without, the input cloud's bit for bit.  With info also the summary dict."""
        prm = _smooth_params(radius, min_neighbours, viewpoint)
        summ = SmoothSummary()
        h = C.c_void_p()
        self._check(self.L.plade_cloud_smooth_dev(self.h, cloud.h, C.byref(prm), 1 if fit_normals else 0, C.byref(h), C.byref(summ)))
        out = Cloud(self, None, handle=(int(summ.n), h))
        return (out, _smooth_info(summ)) if info else out

    # ---- multi-scale normals and dimensionality features ------------------------------------------------
    def scale_features(self, points, radii, mode=0, min_neighbours=None, viewpoint=(0.0, 0.0, 0.0), orient=0, query_index=None,
                       per_scale=True, moments=False):
        """plade_cloud_scale_features: normals and dimensionality features of an (N, >= 3) float32 array (x y z first) at the S =
        len(radii) <= 8 ascending `radii` in one walk, and per query the scale that is most planar (mode 0, M3C2's rule) or has the
        smallest surface variation (mode 1).  The queries are all points, or `query_index` (strictly ascending indices; K = their
        number).  orient 0: normals toward `viewpoint`; 1: along columns 3..5 of `points`, the viewpoint where those do not
        decide.  Returns (normals, info): normals (K, 3) float32, the chosen scale's (NaN where no scale is fitted); info: a dict
        with queries, fitted, chosen_hist (S numbers), max_count, chosen (K int32, -1: none), features (K, 4 float32: linearity,
        planarity, sphericity, variation of the chosen scale) and -- with per_scale -- count (K, S uint32), fitted_mask (K, S
        bools), eigenvalues (K, S, 3 float64: l1 >= l2 >= l3) and normals (K, S, 3 float32), with moments the (K, S, 9) float64
        sums of q and q q^T."""
        a, n, stride = _xyz_view(points)
        prm = _scale_params(radii, mode, min_neighbours, viewpoint, orient)
        q, k = _scale_queries(query_index)
        K, S = (n if q is None else k), max(0, min(int(prm.scales), 8))
        chosen = np.empty(K, np.int32)
        nrm = np.empty((K, 3), np.float32)
        feat = np.empty((K, 4), np.float32)
        count = np.empty((K, S), np.uint32) if per_scale else None
        fitted = np.zeros((K, S), np.uint8) if per_scale else None
        eig = np.empty((K, S, 3), np.float64) if per_scale else None
        nrms = np.empty((K, S, 3), np.float32) if per_scale else None
        mom = np.empty((K, S, 9), np.float64) if moments else None
        summ = ScaleSummary()
        self._check(self.L.plade_cloud_scale_features(self.h, _ptr(a), n, stride, _ptr(q), k, C.byref(prm), _ptr(chosen), _ptr(nrm),
                                                      _ptr(feat), _ptr(count), _ptr(fitted), _ptr(eig), _ptr(nrms), _ptr(mom),
                                                      C.byref(summ)))
        info = _scale_info(summ, S)
        info.update(chosen=chosen, features=feat)
        if per_scale:
            info.update(count=count, fitted_mask=fitted.view(np.bool_), eigenvalues=eig, normals=nrms)
        if moments:
            info["moments"] = mom
        return nrm, info

    def scale_normals_dev(self, cloud, radii, mode=0, min_neighbours=None, viewpoint=(0.0, 0.0, 0.0), orient=0, query_index=None,
                          info=False):
        """plade_cloud_scale_normals_dev: scale_features on a resident cloud (upload, upload_xyz; orient 1 reads its normals) into
        a new resident Cloud of the queries: x y z bit for bit and the chosen normal (NaN where no scale is fitted) -- the core
        points m3c2_dev takes.  The rows are the bits of scale_features.  With info also the summary dict."""
        prm = _scale_params(radii, mode, min_neighbours, viewpoint, orient)
        q, k = _scale_queries(query_index)
        summ = ScaleSummary()
        h = C.c_void_p()
        self._check(self.L.plade_cloud_scale_normals_dev(self.h, cloud.h, _ptr(q), k, C.byref(prm), C.byref(h), C.byref(summ)))
        out = Cloud(self, None, handle=(int(summ.queries), h))
        return (out, _scale_info(summ, int(prm.scales))) if info else out

    # ---- change detection: M3C2 distances -------------------------------------------------------------
    def _m3c2(self, call, m, radius, depth, T, min_points, reg_error, per_point, moments):
        T_in = None if T is None else _f32(T).reshape(4, 4).copy()
        prm = _m3c2_params(radius, depth, min_points, reg_error)
        dist = np.empty(m, np.float64)
        lod = np.empty(m, np.float64) if per_point else None
        sig = np.zeros(m, np.uint8) if per_point else None
        count = np.empty((m, 2), np.uint32) if per_point else None
        sigma = np.empty((m, 2), np.float64) if per_point else None
        mom = np.empty((m, 4), np.float64) if moments else None
        summ = M3c2Summary()
        self._check(call(_ptr(T_in), C.byref(prm), _ptr(dist), _ptr(lod), _ptr(sig), _ptr(count), _ptr(sigma), _ptr(mom), C.byref(summ)))
        info = {k: getattr(summ, k) for k, _ in M3c2Summary._fields_ if k != "reserved"}
        if per_point:
            info.update(lod=lod, significant_mask=sig.view(np.bool_), count=count, sigma=sigma)
        if moments:
            info["moments"] = mom
        return dist, info

    def m3c2(self, core, ref, cmp, radius, depth, T=None, min_points=None, reg_error=0.0, per_point=True, moments=False):
        """plade_cloud_m3c2: M3C2 distances of the compared cloud `cmp` against the reference cloud `ref` (both (N, >= 3) float32,
        x y z first) at the (M, 6) core points x y z nx ny nz: per core point a cylinder of `radius` and half-length `depth` along
        its normal, the mean position of each cloud inside it along the normal, distance = mean_cmp - mean_ref and the 95 % level
        of detection.  T: 4 x 4, cmp -> the frame of ref and core (None: the identity).  Returns (distance, info): distance (M,)
        float64 (NaN where a cloud has fewer than min_points (default 4) points in the cylinder or the normal is zero / not
        finite); info: a dict with m, valid, significant, mean, rms, max, max_count and -- with per_point -- lod (M float64),
        significant_mask (M bools), count (M, 2 uint32: ref, cmp), sigma (M, 2 float64), and with moments the (M, 4) float64
        sums S1_ref S2_ref S1_cmp S2_cmp."""
        c = _f32(core)
        self._check_cloud(c, "m3c2")
        a, n_a, stride_a = _xyz_view(ref)
        b, n_b, stride_b = _xyz_view(cmp)
        return self._m3c2(lambda T_in, prm, *out: self.L.plade_cloud_m3c2(
            self.h, _ptr(c), len(c), _ptr(a), n_a, stride_a, _ptr(b), n_b, stride_b, T_in, prm, *out), len(c), radius, depth, T,
            min_points, reg_error, per_point, moments)

    def m3c2_dev(self, core_cloud, ref_cloud, cmp_cloud, radius, depth, T=None, min_points=None, reg_error=0.0, per_point=True,
                 moments=False):
        """plade_cloud_m3c2_dev: m3c2 on resident clouds (upload, upload_xyz; core_cloud may be ref_cloud); bit-identical results."""
        return self._m3c2(lambda T_in, prm, *out: self.L.plade_cloud_m3c2_dev(
            self.h, core_cloud.h, ref_cloud.h, cmp_cloud.h, T_in, prm, *out), core_cloud.n, radius, depth, T, min_points, reg_error,
            per_point, moments)

    # ---- point descriptors: FPFH, and their match ------------------------------------------------------
    def _fpfh(self, call, n, radius, min_pairs, per_point, seams):
        prm = _fpfh_params(radius, min_pairs)
        desc = np.empty((n, FPFH_DIM), np.float32)
        described = np.zeros(n, np.uint8) if per_point else None
        pairs = np.empty(n, np.uint32) if per_point else None
        spfh = np.empty((n, FPFH_DIM), np.uint32) if seams else None
        raw = np.empty((n, FPFH_DIM + 1), np.float64) if seams else None
        summ = FpfhSummary()
        self._check(call(C.byref(prm), _ptr(desc), _ptr(described), _ptr(pairs), _ptr(spfh), _ptr(raw), C.byref(summ)))
        info = {k: getattr(summ, k) for k, _ in FpfhSummary._fields_ if k != "reserved"}
        if per_point:
            info.update(described_mask=described.view(np.bool_), pairs=pairs)
        if seams:
            info.update(spfh=spfh, raw=raw)
        return desc, info

    def fpfh(self, pos_nrm, radius, min_pairs=None, per_point=True, seams=False):
        """plade_cloud_fpfh: the FPFH descriptors of an (N, 6) float32 cloud x y z nx ny nz over the neighbours closer than
        `radius`.  Returns (desc, info): desc (N, 33) float32, three blocks of 11 bins that sum to 100 each, NaN rows where a
        point has no usable normal or fewer than min_pairs (default 5) counted pairs; info: a dict with n, described,
        mean_pairs, max_pairs and -- with per_point -- described_mask (N bools) and pairs (N uint32), with seams the (N, 33)
        uint32 histograms spfh and the (N, 34) float64 weighted sums raw (W, then R)."""
        a = _f32(pos_nrm)
        self._check_cloud(a, "fpfh")
        return self._fpfh(lambda prm, *out: self.L.plade_cloud_fpfh(self.h, _ptr(a), len(a), prm, *out), len(a), radius, min_pairs,
                          per_point, seams)

    def fpfh_dev(self, cloud, radius, min_pairs=None, per_point=True, seams=False, resident=False):
        """plade_cloud_fpfh_dev: fpfh on a resident cloud (upload); bit-identical results.  With resident the return value is
        (desc, info, features): a Features handle for match_features_dev (free() it)."""
        fh = C.c_void_p()
        out = self._fpfh(lambda prm, desc, described, pairs, spfh, raw, summ: self.L.plade_cloud_fpfh_dev(
            self.h, cloud.h, prm, desc, described, pairs, spfh, raw, C.byref(fh) if resident else None, summ), cloud.n, radius,
            min_pairs, per_point, seams)
        return out + (Features(self, cloud.n, fh),) if resident else out

    def _match_features(self, call, ns, nt, mutual, max_ratio, cap):
        prm = _feature_match_params(mutual, max_ratio)
        nn = np.empty(ns, np.int32)
        d2 = np.empty((ns, 2), np.float32)
        back = np.empty(nt, np.int32)
        cap = ns if cap is None else int(cap)
        corr = np.empty((max(cap, 1), 2), np.int32)
        total = C.c_uint64()
        rc = self._check(call(C.byref(prm), _ptr(nn), _ptr(d2), _ptr(back), _ptr(corr), cap, C.byref(total)), allow=(PLADE_ECAP,))
        return corr[:min(cap, total.value)], {"n_corr": total.value, "nn": nn, "d2": d2, "back": back, "complete": rc == 0}

    def match_features(self, src, tgt, mutual=True, max_ratio=0.0, cap=None):
        """plade_match_features: nearest neighbours in feature space between two (N, 33) float32 descriptor tables (rows whose
        first value is NaN take no part).  Returns (corr, info): corr (M, 2) int32, the kept (source, target) pairs ascending
        in the source index -- with mutual only the pairs that are each other's nearest neighbour, with max_ratio > 0 only those
        whose nearest distance is below max_ratio times the second nearest; info: n_corr (exact, also when cap -- the capacity
        of corr, default len(src) -- was smaller: then complete is False), nn (Ns int32, -1: none), d2 (Ns, 2 float32 squared
        distances of the two nearest, NaN: none), back (Nt int32, the targets' nearest sources)."""
        s, t = _feature_table(src, "match_features"), _feature_table(tgt, "match_features")
        return self._match_features(lambda prm, *out: self.L.plade_match_features(self.h, _ptr(s), len(s), _ptr(t), len(t), prm, *out),
                                    len(s), len(t), mutual, max_ratio, cap)

    def match_features_dev(self, src_features, tgt_features, mutual=True, max_ratio=0.0, cap=None):
        """plade_match_features_dev: match_features on two resident tables (fpfh_dev(..., resident=True)); bit-identical results."""
        return self._match_features(lambda prm, *out: self.L.plade_match_features_dev(self.h, src_features.h, tgt_features.h, prm, *out),
                                    src_features.n, tgt_features.n, mutual, max_ratio, cap)

    # ---- a pose from correspondences (RANSAC), and FPFH -> match -> pose in one call -------------------------------
    def _estimate_pose(self, call, m, inlier_dist, seams, pose_params):
        prm = _corr_pose_params(inlier_dist, pose_params)
        H = max(int(prm.hypotheses), 1)
        T = np.empty((4, 4), np.float32)
        inlier = np.zeros(m, np.uint8)
        triple = np.empty((H, 3), np.int32) if seams else None
        status = np.empty(H, np.uint8) if seams else None
        count = np.empty(H, np.uint32) if seams else None
        Th = np.empty((H, 3, 4), np.float64) if seams else None
        res = CorrPoseResult()
        rc = self._check(call(C.byref(prm), _ptr(T), _ptr(inlier), _ptr(triple), _ptr(status), _ptr(count), _ptr(Th), C.byref(res)),
                         allow=(PLADE_EFAIL,))
        info = _corr_pose_info(res)
        info.update(ok=rc == 0, reason=CORR_POSE_FAILURES.get(res.failure), inlier=inlier.view(np.bool_))
        if seams and not (rc != 0 and res.failure == PLADE_CORR_POSE_TOO_FEW):
            info.update(triple=triple, status=status, count=count, hyp_T=Th)
        return T, info

    def estimate_pose(self, src_xyz, tgt_xyz, corr, inlier_dist, seams=False, **pose_params):
        """plade_estimate_pose_corr: the rigid source -> target pose from M correspondences (an (M, 2) int32 array of (source,
        target) rows into the two (N, >= 3) float32 arrays) by RANSAC over triples with an edge-length prerejection, an exhaustive
        inlier count (d < inlier_dist) and a least-squares refit.  pose_params: hypotheses, edge_similarity, min_inliers,
        refine_iterations, seed.  Returns (T, info): T (4, 4) float32 (the identity when it failed), info = the
        plade_corr_pose_result fields plus ok, reason (None, "fewer than 3 correspondences", "nothing scored", "too few inliers"),
        inlier (M bools) and -- with seams -- per hypothesis triple (H, 3), status (H), count (H) and hyp_T (H, 3, 4) float64; T64: the (3, 4) float64 iterate T is rounded from."""
        s, ns, ss = _xyz_view(src_xyz)
        t, nt, ts = _xyz_view(tgt_xyz)
        c = _corr_list(corr, "estimate_pose")
        return self._estimate_pose(lambda prm, *out: self.L.plade_estimate_pose_corr(self.h, _ptr(s), ns, ss, _ptr(t), nt, ts, _ptr(c),
                                                                                     len(c), prm, *out), len(c), inlier_dist, seams,
                                   pose_params)

    def estimate_pose_dev(self, src_cloud, tgt_cloud, corr, inlier_dist, seams=False, **pose_params):
        """plade_estimate_pose_corr_dev: estimate_pose on two resident clouds; bit-identical results."""
        c = _corr_list(corr, "estimate_pose_dev")
        return self._estimate_pose(lambda prm, *out: self.L.plade_estimate_pose_corr_dev(self.h, src_cloud.h, tgt_cloud.h, _ptr(c), len(c),
                                                                                         prm, *out), len(c), inlier_dist, seams, pose_params)

    def corr_pose_moments(self, src_xyz, tgt_xyz, corr, T, inlier_dist):
        """plade_corr_pose_moments (test seam): one refinement pass without the solve under the fp64 T (3 x 4 or 4 x 4).  Returns
        (flags, moments): flags (M bools), moments (17,) float64 = n, mean S, mean Q, C row-major, sum d2 over the flagged."""
        s, ns, ss = _xyz_view(src_xyz)
        t, nt, ts = _xyz_view(tgt_xyz)
        c = _corr_list(corr, "corr_pose_moments")
        T12 = np.ascontiguousarray(np.asarray(T, dtype=np.float64)[:3, :4])
        flags = np.zeros(len(c), np.uint8)
        mom = np.empty(CORR_MOMENTS, np.float64)
        self._check(self.L.plade_corr_pose_moments(self.h, _ptr(s), ns, ss, _ptr(t), nt, ts, _ptr(c), len(c), _ptr(T12),
                                                   float(inlier_dist), _ptr(flags), _ptr(mom)))
        return flags.view(np.bool_), mom

    def _register_features(self, call, ns, radius, inlier_dist, min_pairs, mutual, max_ratio, pose_params):
        fp, mp, pp = _fpfh_params(radius, min_pairs), _feature_match_params(mutual, max_ratio), _corr_pose_params(inlier_dist, pose_params)
        T = np.empty((4, 4), np.float32)
        s_src, s_tgt, res = FpfhSummary(), FpfhSummary(), CorrPoseResult()
        corr = np.empty((max(ns, 1), 2), np.int32)
        total = C.c_uint64()
        rc = self._check(call(C.byref(fp), C.byref(mp), C.byref(pp), _ptr(T), C.byref(s_src), C.byref(s_tgt), C.byref(res), _ptr(corr), ns,
                              C.byref(total)), allow=(PLADE_EFAIL,))
        info = _corr_pose_info(res)
        info.update(ok=rc == 0, reason=CORR_POSE_FAILURES.get(res.failure), n_corr=total.value, corr=corr[:total.value].copy(),
                    fpfh_src={k: getattr(s_src, k) for k, _ in FpfhSummary._fields_ if k != "reserved"},
                    fpfh_tgt={k: getattr(s_tgt, k) for k, _ in FpfhSummary._fields_ if k != "reserved"})
        return T, info

    def register_features(self, tgt, src, radius, inlier_dist, min_pairs=None, mutual=True, max_ratio=0.0, **pose_params):
        """plade_register_features: FPFH of both (N, 6) clouds at `radius`, their match and the pose from the correspondences in one
        call, with nothing leaving the device in between; the bits of fpfh, match_features and estimate_pose chained.  Returns
        (T, info): T the 4 x 4 source -> target pose (the identity when it failed), info = the pose result's fields plus ok, reason,
        n_corr, corr ((n_corr, 2) int32) and the two FPFH summaries fpfh_src, fpfh_tgt."""
        tgt, src = _f32(tgt), _f32(src)
        self._check_cloud(tgt, "register_features"); self._check_cloud(src, "register_features")
        return self._register_features(lambda *a: self.L.plade_register_features(self.h, _ptr(tgt), len(tgt), _ptr(src), len(src), *a),
                                       len(src), radius, inlier_dist, min_pairs, mutual, max_ratio, pose_params)

    def register_features_dev(self, tgt_cloud, src_cloud, radius, inlier_dist, min_pairs=None, mutual=True, max_ratio=0.0, **pose_params):
        """plade_register_features_dev: register_features on two resident clouds; bit-identical results."""
        return self._register_features(lambda *a: self.L.plade_register_features_dev(self.h, tgt_cloud.h, src_cloud.h, *a), src_cloud.n,
                                       radius, inlier_dist, min_pairs, mutual, max_ratio, pose_params)

    # ---- keypoints (ISS), and ISS -> FPFH -> match of the keypoints -> pose in one call ---------------------------
    def _iss(self, call, n, prm, per_point, seams, cap):
        key = np.zeros(n, np.uint8) if per_point else None
        sal = np.empty(n, np.float64) if per_point else None
        eig = np.empty((n, 3), np.float64) if per_point else None
        count = np.empty(n, np.uint32) if per_point else None
        nms = np.empty(n, np.uint32) if per_point else None
        scatter = np.empty((n, 6), np.float64) if seams else None
        cap = n if cap is None else int(cap)
        index = np.empty(max(cap, 1), np.uint32)
        total, summ = C.c_uint64(), IssSummary()
        rc = self._check(call(C.byref(prm), _ptr(key), _ptr(index), cap, C.byref(total), _ptr(sal), _ptr(eig), _ptr(count), _ptr(nms),
                              _ptr(scatter), C.byref(summ)), allow=(PLADE_ECAP,))
        info = {k: getattr(summ, k) for k, _ in IssSummary._fields_ if k != "reserved"}
        info.update(n_keypoints=total.value, complete=rc == 0)
        if per_point:
            info.update(keypoint=key.view(np.bool_), saliency=sal, eigenvalues=eig, count=count, nms_count=nms)
        if seams:
            info.update(scatter=scatter)
        return index[:min(cap, total.value)].copy(), info

    def iss_keypoints(self, points, salient_radius, non_max_radius=0.0, gamma21=None, gamma32=None, min_neighbours=None, per_point=True,
                      seams=False, cap=None):
        """plade_cloud_keypoints_iss: the ISS keypoints of an (N, >= 3) float32 array whose first columns are x y z.  A point is
        salient when the eigenvalues l1 >= l2 >= l3 of the scatter of its neighbours within salient_radius (about the point itself)
        satisfy l2 < gamma21 l1 and l3 < gamma32 l2 (defaults 0.975) and l3 > 1e-9 l1; it is a keypoint when it also has at least
        min_neighbours (default 5) other points within non_max_radius (0: salient_radius) and none of them has a larger l3.  Returns
        (index, info): index, the keypoints' rows ascending (uint32; at most cap of them, default N -- then complete is False);
        info: n, salient, keypoints, max_count, n_keypoints (exact) and -- with per_point -- keypoint (N bools), saliency (N float64:
        l3 or 0), eigenvalues (N, 3 float64, descending), count and nms_count (N uint32: the points within the two radii, the point
        itself included), with seams the (N, 6) float64 sums scatter (xx xy xz yy yz zz)."""
        a, n, stride = _xyz_view(points)
        prm = _iss_params(salient_radius, non_max_radius, gamma21, gamma32, min_neighbours)
        return self._iss(lambda *o: self.L.plade_cloud_keypoints_iss(self.h, _ptr(a), n, stride, *o), n, prm, per_point, seams, cap)

    def iss_keypoints_dev(self, cloud, salient_radius, non_max_radius=0.0, gamma21=None, gamma32=None, min_neighbours=None, per_point=True,
                          seams=False, cap=None):
        """plade_cloud_keypoints_iss_dev: iss_keypoints on a resident cloud (upload); bit-identical results."""
        prm = _iss_params(salient_radius, non_max_radius, gamma21, gamma32, min_neighbours)
        return self._iss(lambda *o: self.L.plade_cloud_keypoints_iss_dev(self.h, cloud.h, *o), cloud.n, prm, per_point, seams, cap)

    def select_features(self, features, index):
        """plade_features_select: rows `index` of a resident descriptor table (fpfh_dev(..., resident=True)) as a new Features handle
        (free() it) -- the table of a cloud's keypoints for match_features_dev."""
        idx = np.ascontiguousarray(np.asarray(index).reshape(-1))
        if idx.size and (idx.min() < 0 or idx.max() > 0xffffffff):
            raise ValueError("select_features: an index is negative or does not fit 32 bits")
        idx = idx.astype(np.uint32)
        fh = C.c_void_p()
        self._check(self.L.plade_features_select(self.h, features.h, _ptr(idx), len(idx), C.byref(fh)))
        return Features(self, len(idx), fh)

    def _register_keypoints(self, call, ns, ip, radius, inlier_dist, min_pairs, mutual, max_ratio, pose_params):
        fp, mp, pp = _fpfh_params(radius, min_pairs), _feature_match_params(mutual, max_ratio), _corr_pose_params(inlier_dist, pose_params)
        T = np.empty((4, 4), np.float32)
        s_iss, s_src, s_tgt, res = IssSummary(), FpfhSummary(), FpfhSummary(), CorrPoseResult()
        corr = np.empty((max(ns, 1), 2), np.int32)
        total = C.c_uint64()
        rc = self._check(call(C.byref(ip), C.byref(fp), C.byref(mp), C.byref(pp), _ptr(T), C.byref(s_iss), C.byref(s_src), C.byref(s_tgt),
                              C.byref(res), _ptr(corr), ns, C.byref(total)), allow=(PLADE_EFAIL,))
        info = _corr_pose_info(res)
        info.update(ok=rc == 0, reason=CORR_POSE_FAILURES.get(res.failure), n_corr=total.value, corr=corr[:total.value].copy(),
                    iss={k: getattr(s_iss, k) for k, _ in IssSummary._fields_ if k != "reserved"},
                    fpfh_src={k: getattr(s_src, k) for k, _ in FpfhSummary._fields_ if k != "reserved"},
                    fpfh_tgt={k: getattr(s_tgt, k) for k, _ in FpfhSummary._fields_ if k != "reserved"})
        return T, info

    def register_keypoints(self, tgt, src, radius, inlier_dist, salient_radius, non_max_radius=0.0, gamma21=None, gamma32=None,
                           min_neighbours=None, min_pairs=None, mutual=True, max_ratio=0.0, **pose_params):
        """plade_register_keypoints: register_features with the ISS detector in front of the match -- the keypoints of the source
        (iss_keypoints at salient_radius / non_max_radius), FPFH of both (N, 6) clouds at `radius`, the source's keypoint rows
        matched against every described target point, the pose from the correspondences; the bits of those calls chained by hand.
        Returns (T, info) as register_features, corr holding original source indices, plus the detector's summary info["iss"]."""
        tgt, src = _f32(tgt), _f32(src)
        self._check_cloud(tgt, "register_keypoints"); self._check_cloud(src, "register_keypoints")
        ip = _iss_params(salient_radius, non_max_radius, gamma21, gamma32, min_neighbours)
        return self._register_keypoints(lambda *a: self.L.plade_register_keypoints(self.h, _ptr(tgt), len(tgt), _ptr(src), len(src), *a),
                                        len(src), ip, radius, inlier_dist, min_pairs, mutual, max_ratio, pose_params)

    def register_keypoints_dev(self, tgt_cloud, src_cloud, radius, inlier_dist, salient_radius, non_max_radius=0.0, gamma21=None,
                               gamma32=None, min_neighbours=None, min_pairs=None, mutual=True, max_ratio=0.0, **pose_params):
        """plade_register_keypoints_dev: register_keypoints on two resident clouds; bit-identical results."""
        ip = _iss_params(salient_radius, non_max_radius, gamma21, gamma32, min_neighbours)
        return self._register_keypoints(lambda *a: self.L.plade_register_keypoints_dev(self.h, tgt_cloud.h, src_cloud.h, *a), src_cloud.n,
                                        ip, radius, inlier_dist, min_pairs, mutual, max_ratio, pose_params)

    # ---- merging registered clouds ---------------------------------------------------------------
    @staticmethod
    def _merge_transforms(transforms, k):
        if transforms is None:
            return None
        if len(transforms) != k:
            raise ValueError("merge_clouds: one transform per cloud (None entries: the identity)")
        T = np.empty((k, 4, 4), np.float32)
        for c, t in enumerate(transforms):
            T[c] = np.eye(4, dtype=np.float32) if t is None else _f32(t).reshape(4, 4)
        return T

    @staticmethod
    def _merge_info(summ, count, mask):
        info = {k: getattr(summ, k) for k, _ in MergeSummary._fields_ if k != "reserved"}
        if count is not None:
            info["count"], info["mask"] = count[:summ.n_out].copy(), mask[:summ.n_out].copy()
        return info

    def merge_clouds(self, clouds, transforms=None, leaf=0.0, per_voxel=True):
        """plade_merge_clouds: 1..16 (N_c, 6) float32 clouds x y z nx ny nz, each taken into the output frame by its 4 x 4
        transform (None: the identity), fused per voxel of edge `leaf` -- fp64 mean position, normalised fp64 sum of the finite
        normals (opposite normals cancel: NaN) -- or, with leaf = 0, concatenated.  Returns (rows, info): the (M, 6) float32 rows in
        voxel order and a dict with n_in, n_out, n_shared, max_count and -- with per_voxel -- count and mask (M uint32: the
        voxel's points, bit c set when cloud c contributed)."""
        arrs = [_f32(a) for a in clouds]
        k = len(arrs)
        for a in arrs:
            if a.ndim != 2 or a.shape[1] != 6:
                raise ValueError(f"merge_clouds: (N, 6) arrays x y z nx ny nz are required, got shape {a.shape}")
        T = self._merge_transforms(transforms, k)
        ptrs, ns = self._cloud_table(arrs)
        total = sum(len(a) for a in arrs)
        rows = np.empty((total, 6), np.float32)
        count = np.empty(total, np.uint32) if per_voxel else None
        mask = np.empty(total, np.uint32) if per_voxel else None
        summ = MergeSummary()
        self._check(self.L.plade_merge_clouds(self.h, k, ptrs, ns, _ptr(T), float(leaf), _ptr(rows), _ptr(count), _ptr(mask),
                                              C.byref(summ)))
        return rows[:summ.n_out].copy(), self._merge_info(summ, count, mask)

    def merge_clouds_dev(self, clouds, transforms=None, leaf=0.0, info=False, per_voxel=True):
        """plade_merge_clouds_dev: merge_clouds on resident clouds into a new resident Cloud (the point data makes no host round
        trip); the same bits.  With info also the info dict of merge_clouds."""
        k = len(clouds)
        T = self._merge_transforms(transforms, k)
        hs = (C.c_void_p * k)(*[c.h.value for c in clouds])
        total = sum(c.n for c in clouds)
        count = np.empty(total, np.uint32) if info and per_voxel else None
        mask = np.empty(total, np.uint32) if info and per_voxel else None
        summ = MergeSummary()
        h = C.c_void_p()
        self._check(self.L.plade_merge_clouds_dev(self.h, k, hs, _ptr(T), float(leaf), C.byref(h), _ptr(count), _ptr(mask), C.byref(summ)))
        out = Cloud(self, None, handle=(int(summ.n_out), h))
        return (out, self._merge_info(summ, count, mask)) if info else out

    def pin(self, arr):
        """Page-lock a C-contiguous float32 array the caller keeps alive (plade_host_pin); registration() calls that are
        handed this very array then upload it by asynchronous DMA."""
        assert arr.dtype == np.float32 and arr.flags["C_CONTIGUOUS"]
        self._check(self.L.plade_host_pin(self.h, _ptr(arr), arr.nbytes))
        return arr

    def unpin(self, arr):
        self._check(self.L.plade_host_unpin(self.h, _ptr(arr)))

    def registration_dev(self, tgt_cloud, src_cloud):
        T = np.zeros((4, 4), np.float32)
        rc = self._check(self.L.plade_registration_dev(self.h, tgt_cloud.h, src_cloud.h, _ptr(T)), allow=(PLADE_EFAIL,))
        return rc == 0, T

    # ---- instrumentation ---------------------------------------------------------------------
    def dump(self, pair=0):
        out = {}
        h = self._pair_handle(pair) if pair else self.h
        for name, dt in DUMP_FIELDS.items():
            ptr = C.c_void_p()
            nb = C.c_int64()
            if self.L.plade_dump_get(h, name.encode(), C.byref(ptr), C.byref(nb)) != 0:
                continue
            if nb.value == 0 or not ptr.value:
                out[name] = np.zeros(0, dt)
                continue
            buf = (C.c_char * nb.value).from_address(ptr.value)
            out[name] = np.frombuffer(bytes(buf), dtype=dt).copy()
        return out

    def stats(self, pair=0):
        names = C.c_char_p()
        vals = C.POINTER(C.c_double)()
        cnt = C.c_int32()
        self._check(self.L.plade_stats_get(self._pair_handle(pair) if pair else self.h, C.byref(names), C.byref(vals), C.byref(cnt)))
        ns = names.value.decode().strip(";").split(";") if cnt.value else []
        return {ns[i]: vals[i] for i in range(cnt.value)}

    def kernel_time(self, which, iters=20):
        t = C.c_double()
        b = C.c_double()
        self._check(self.L.plade_kernel_time(self.h, which.encode(), iters, C.byref(t), C.byref(b)))
        return t.value, b.value
