// plade_amd/csrc/plade.h -- the C++ host API of PLADE, kept source compatible with the reference's
// code/PLADE/plade.h:44-96 (same four registration() overloads, same argument order and meaning,
// same bool/identity-on-failure behaviour, messages on std::cout/std::cerr), implemented on top of
// the C ABI of libplade_hip.so (include/plade_hip.h).
//
// The reference's signatures mention Eigen::Matrix<float,4,4>, pcl::PointCloud<pcl::PointNormal>::Ptr
// and PLANE (code/PLADE/plane_extraction.h:44-50).  This image has neither Eigen nor PCL/Boost, so
// "plade_compat.h" provides minimal stand-ins with the same names, layouts and members the
// signatures and the CLI use; define PLADE_USE_REAL_EIGEN_PCL before including this header in a
// tree that has the real libraries (INTEGRATION.md shows the reference-side change).
#ifndef PLADE_H
#define PLADE_H

#include <iosfwd>
#include <string>
#include <utility>
#include <vector>

#ifdef PLADE_USE_REAL_EIGEN_PCL
#include <Eigen/Core>
#include <Eigen/LU>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include "plane_extraction.h"
#else
#include "plade_compat.h"
#endif

/** plade.h:44-47 -- file names of two PLY point clouds. */
bool registration(Eigen::Matrix<float, 4, 4> &transformation,
                  const std::string &target_cloud_file,
                  const std::string &source_cloud_file);

/** plade.h:58-61 -- auto-tunes the RANSAC min support so that 10..40 planes are used. */
bool registration(Eigen::Matrix<float, 4, 4> &transformation,
                  pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                  pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud);

/** plade.h:74-79 -- the user provides the extracted planes. */
bool registration(Eigen::Matrix<float, 4, 4> &transformation,
                  pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                  pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud,
                  const std::vector<PLANE> &target_planes,
                  const std::vector<PLANE> &source_planes);

/** plade.h:91-96 -- explicit RANSAC min support per cloud. */
bool registration(Eigen::Matrix<float, 4, 4> &transformation,
                  pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                  pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud,
                  int ransac_min_support_target,
                  int ransac_min_support_source);

/** Fine alignment (no counterpart in the reference): refines `transformation` (source -> target, e.g. the result of one of the
 *  registration() overloads above) by point-to-plane ICP on the GPU (plade_refine_icp, default parameters; the target needs
 *  normals, the source's are ignored).  Prints one line on success.  false: the refinement failed (too few correspondences, a
 *  degenerate geometry, no GPU) and `transformation` is unchanged; a warning is printed.  The CLI and the file / cloud overloads
 *  of registration(T, target, source) call it for every registered pair when PLADE_REFINE_ICP=1. */
bool refine_registration(Eigen::Matrix<float, 4, 4> &transformation,
                         pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                         pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud);

/** Fine alignment by plane-to-plane (generalized) ICP on the GPU (plade_refine_gicp, default parameters and the given epsilon --
 *  0: 1e-3; 1: point-to-point ICP): like refine_registration, but BOTH clouds' normals are read and every correspondence is
 *  weighted by how well the two normals agree, so the roles of the two clouds are symmetric and clutter in front of a wall counts
 *  little.  Prints one line on success.  false: the refinement failed (too few correspondences, a degenerate geometry, an invalid
 *  epsilon, no GPU) and `transformation` is unchanged; a warning is printed.  The CLI and the file / cloud overloads of
 *  registration(T, target, source) call it for every registered pair when PLADE_REFINE_GICP=1[,<epsilon>] is set (it then takes
 *  the place of PLADE_REFINE_ICP's refinement). */
bool refine_registration_gicp(Eigen::Matrix<float, 4, 4> &transformation,
                              pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                              pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud, double epsilon = 0.0);

/** Registration quality (no counterpart in the reference): the fields of plade_distance_summary (include/plade_hip.h). */
struct RegistrationQuality {
    uint64_t n = 0, count = 0, plane_count = 0;   // source points, those within max_dist, those of them with a finite target normal
    double fitness = 0, rmse = 0, mean = 0, max = 0, plane_rmse = 0;
};
/** Evaluates `transformation` (source -> target) on the GPU (plade_cloud_distances, no per-point outputs): fitness = the share of
 *  source points whose nearest target point is closer than max_dist (absolute, in the clouds' units), the rmse / mean / max of
 *  those distances and the point-to-plane rmse.  false: invalid input or no GPU; a warning is printed and `out` is unchanged.
 *  The CLI prints one such evaluation per registered pair when PLADE_EVALUATE=<max_dist> is set. */
bool evaluate_registration(const Eigen::Matrix4f &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                           pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud, float max_dist, RegistrationQuality &out);

/** Outlier removal (no counterpart in the reference): the fields of plade_outlier_summary (include/plade_hip.h). */
struct OutlierRemoval {
    uint64_t n = 0, kept = 0;                  // points in, points kept
    double mu = 0, sigma = 0, threshold = 0;   // of the mean neighbour distances; threshold = mu + alpha sigma
};
/** Statistical outlier filter on the GPU (plade_filter_outliers): a point is kept when the mean distance to its k (1..64) nearest
 *  neighbours is at most mu + alpha sigma of those means over the cloud.  `filtered` receives the kept points in their original
 *  order, coordinates and normals copied bit for bit (it may be *cloud).  false: invalid input or no GPU; a message is printed and
 *  `filtered` is unchanged.  The CLI and the file overload of registration() filter both clouds of a pair after reading them, and
 *  before PLADE_ESTIMATE_NORMALS, when PLADE_REMOVE_OUTLIERS=<k>[,<alpha>] is set, and print one line per cloud. */
bool remove_outliers(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, pcl::PointCloud<pcl::PointNormal> &filtered, int k = 16,
                     double alpha = 1.0, OutlierRemoval *info = nullptr);

/** Connected components (no counterpart in the reference): the fields of plade_component_summary (include/plade_hip.h). */
struct ComponentFilter {
    uint64_t n = 0, components = 0, kept_components = 0, kept = 0;   // points in, components found, components and points kept
    uint32_t largest = 0;                                            // the size of the largest component
};
/** Keeps the connected components of the graph "closer than radius" (absolute, in the cloud's units; fp32 squared distance, strict
 *  <) that hold at least min_size and, when max_size > 0, at most max_size points -- with keep_largest = m > 0 only the m largest of
 *  them -- on the GPU (plade_label_components): dense blobs that do not belong to the structure, which no neighbour-count filter
 *  removes.  `filtered` receives the kept points in their original order, coordinates and normals copied bit for bit (it may be
 *  *cloud).  false: invalid input or no GPU; a message is printed and `filtered` is unchanged.  The CLI and the file overload of
 *  registration() filter both clouds of a pair after PLADE_REMOVE_OUTLIERS and before PLADE_ESTIMATE_NORMALS when
 *  PLADE_KEEP_COMPONENTS=<radius>[,<min_size>[,<keep_largest>]] is set, and print one line per cloud. */
bool keep_components(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, pcl::PointCloud<pcl::PointNormal> &filtered, double radius,
                     int min_size = 1, int max_size = 0, int keep_largest = 0, ComponentFilter *info = nullptr);

/** DBSCAN (no counterpart in the reference): the fields of plade_dbscan_summary (include/plade_hip.h). */
struct CloudClusters {
    uint64_t n = 0, clusters = 0, core = 0, border = 0, noise = 0;   // points in, clusters found, points of each kind
    uint64_t kept_clusters = 0, kept = 0;                            // clusters and points kept
    uint32_t largest = 0;                                            // the size of the largest cluster
};
/** Clusters a cloud by density on the GPU (plade_cluster_dbscan; radius absolute, in the cloud's units; fp32 squared distance, strict
 *  <): a point with at least min_points points closer than radius, itself included, is a core point; the clusters are the connected
 *  components of the core points; a non-core point with a core point closer than radius joins the cluster of the nearest one (ties:
 *  the smaller index); the rest is noise.  Unlike keep_components, one thin thread of stray points joins no two objects.  `labels`
 *  receives one id per point of *cloud (ascending in the order of a cluster's smallest core index, -1 = noise); `filtered` the points
 *  of the clusters that hold at least min_size points -- with keep_largest = m > 0 only of the m largest -- in their original order,
 *  coordinates and normals copied bit for bit (it may be *cloud).  false: invalid input or no GPU; a message is printed and
 *  `filtered` and `labels` are unchanged.  The CLI and the file overload of registration() filter both clouds of a pair after
 *  PLADE_KEEP_COMPONENTS and before PLADE_SMOOTH when PLADE_DBSCAN=<radius>,<min_points>[,<min_size>[,<keep_largest>]] is set, and
 *  print one line per cloud; PLADE_M3C2_CLUSTERS=<radius>[,<min_points>[,<min_size>]] groups the significant core points of
 *  PLADE_M3C2 into objects of change. */
bool cluster_cloud(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, pcl::PointCloud<pcl::PointNormal> &filtered, std::vector<int32_t> &labels,
                   double radius, int min_points = 4, int min_size = 1, int keep_largest = 0, CloudClusters *info = nullptr);

/** Subsampling (no counterpart in the reference): the fields of plade_subsample_summary (include/plade_hip.h). */
struct CloudSubsample {
    uint32_t n = 0, kept = 0, rounds = 0;   // points in, points kept, synchronous rounds until every point was decided
};
/** Thins a cloud to a subset of its own points at a minimum spacing (absolute, in the cloud's units; fp32 squared distance, strict
 *  <) on the GPU (plade_subsample_spacing): no two kept points are closer than spacing, every dropped point has a kept point closer
 *  than spacing.  The set is the greedy walk in the order of the hashed keys of (seed, index): it depends on the points, spacing and
 *  seed only.  `subset` receives the kept points in their original order, coordinates and normals copied bit for bit (it may be
 *  *cloud).  false: invalid input or no GPU; a message is printed and `subset` is unchanged.  The CLI and the file overload of
 *  registration() thin both clouds of a pair as the last preparation step, after PLADE_ESTIMATE_NORMALS, when
 *  PLADE_SUBSAMPLE=<spacing>[,<seed>] is set, and print one line per cloud; PLADE_M3C2_CORE=<spacing>[,<seed>] makes the subsample
 *  of the target the core points of PLADE_M3C2. */
bool subsample_cloud(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, pcl::PointCloud<pcl::PointNormal> &subset, double spacing,
                     uint64_t seed = 0, CloudSubsample *info = nullptr);

/** Consistent normal orientation (no counterpart in the reference): the fields of plade_orient_summary (include/plade_hip.h). */
struct NormalOrientation {
    uint32_t n = 0, unoriented = 0, components = 0, flipped = 0, tree_edges = 0, rounds = 0;
    uint64_t tree_key_sum = 0;
};
/** Puts the normals of a cloud on one side of the surface on the GPU (plade_orient_normals), per connected component of the graph
 *  "closer than radius" (absolute, in the cloud's units; fp32 squared distance, strict <): the flips follow the minimum spanning forest
 *  of the flattest neighbour pairs (Hoppe et al. 1992), so no viewpoint per point is needed -- merged clouds, moved scans and files with
 *  unoriented normals.  mode 0: every component takes the side on which more of its normals face `reference`, a viewpoint of three
 *  floats (nullptr: the origin); mode 1: the normal of the component's extreme point along `reference`, a direction of three floats
 *  that must not be zero (nullptr: +z), gets a component along it.  inward inverts either decision.  Normals that
 *  are not finite stay as they are.  `oriented` receives the same points in the same order, flipped normals with their sign bits
 *  toggled (it may be *cloud).  Two parallel sheets closer than radius get the same side: keep radius below the thinnest wall.
 *  false: invalid input or no GPU; a message is printed and `oriented` is unchanged.  The CLI and the file overload of registration()
 *  orient both clouds of a pair after PLADE_ESTIMATE_NORMALS when PLADE_CONSISTENT_NORMALS=<radius>[,<mode>[,<inward>]] is set
 *  (reference: the origin / +z), and print one line per cloud.  This is not the `orient_normals` parameter of the registration,
 *  which only makes the planes' normals agree with their points' (DESIGN.md section 2). */
bool orient_cloud_normals(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, pcl::PointCloud<pcl::PointNormal> &oriented, double radius,
                          int mode = 0, bool inward = false, const float *reference = nullptr, NormalOrientation *info = nullptr);

/** Smoothing (no counterpart in the reference): the fields of plade_smooth_summary (include/plade_hip.h). */
struct CloudSmoothing {
    uint64_t n = 0, fitted = 0;   // points in, points that were fitted and projected
    double rms = 0, max = 0;      // of the displacements of the fitted points
    uint32_t max_count = 0;       // the largest neighbourhood
};
/** Moving-least-squares plane projection on the GPU (plade_smooth_cloud): every point with at least min_neighbours points (itself
 *  included) closer than radius (absolute, in the cloud's units) is projected onto the plane fitted to that neighbourhood with the
 *  weights (1 - d^2 / radius^2)^2; the others stay where they are.  `smoothed` receives the points in their original order (it may
 *  be *cloud) with their own normals bit for bit or, with use_fit_normals, the fits' normals oriented toward the origin (NaN where
 *  unfitted).  false: invalid input or no GPU; a message is printed and `smoothed` is unchanged.  The CLI and the file overload of
 *  registration() smooth both clouds of a pair after PLADE_REMOVE_OUTLIERS and PLADE_KEEP_COMPONENTS and before
 *  PLADE_ESTIMATE_NORMALS when PLADE_SMOOTH=<radius>[,<min_neighbours>] is set, and print one line per cloud. */
bool smooth_cloud(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, pcl::PointCloud<pcl::PointNormal> &smoothed, double radius,
                  int min_neighbours = 6, bool use_fit_normals = false, CloudSmoothing *info = nullptr);

/** Multi-scale normals (no counterpart in the reference): the fields of plade_scale_summary (include/plade_hip.h). */
struct CloudScales {
    uint64_t queries = 0, fitted = 0;   // points in, points with a chosen scale
    uint32_t chosen_hist[8] = {};       // points per chosen scale
    uint32_t max_count = 0;             // the largest neighbourhood
};
/** Normals at the most planar of several scales on the GPU (plade_cloud_scale_features, the normal-scale step of M3C2): every
 *  point's neighbourhood is fitted at each of the 1 .. 8 ascending `radii` (absolute, in the cloud's units) in one walk, and the
 *  point takes the normal of the scale with the largest planarity (mode 0) or the smallest surface variation (mode 1) among those
 *  with at least min_neighbours points (itself included).  `with_normals` receives the points in their original order (it may be
 *  *cloud) with these normals, NaN where no scale is fitted; they point toward the origin or, with orient_by_cloud_normals, to the
 *  side of the cloud's own normals (toward the origin where those are zero, orthogonal or not finite).  false: invalid input or no
 *  GPU; a message is printed and `with_normals` is unchanged.  The CLI gives the core points of PLADE_M3C2 such normals when
 *  PLADE_M3C2_NORMALS=<r_min>,<r_max>[,<scales>[,<mode>]] is set, and prints one line. */
bool multiscale_normals(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, pcl::PointCloud<pcl::PointNormal> &with_normals,
                        const std::vector<double> &radii, int mode = 0, int min_neighbours = 6, bool orient_by_cloud_normals = false,
                        CloudScales *info = nullptr);

/** Change detection (no counterpart in the reference): the fields of plade_m3c2_summary (include/plade_hip.h). */
struct CloudComparison {
    uint64_t m = 0, valid = 0, significant = 0;   // core points, those with enough points of both clouds, those beyond the level of detection
    double mean = 0, rms = 0, max = 0;            // of the distances (max: of their absolute values) over the valid core points
    uint32_t max_count = 0;                       // the largest number of points of one cloud in a cylinder
};
/** M3C2 distances on the GPU (plade_cloud_m3c2): the core points are the points of reference_cloud with their normals; per core
 *  point a cylinder of `radius` and half-length `depth` (absolute, in the clouds' units) along the normal, the mean position of
 *  each cloud inside it along the normal -- compared_cloud under `transformation` (compared -> reference) -- and the difference of
 *  the two means.  `distances` receives one value per point of reference_cloud (NaN where a cloud has fewer than min_points points
 *  in the cylinder or the normal is zero or not finite); info->significant counts the core points with |distance| above the 95 %
 *  level of detection, to which reg_error (e.g. RegistrationQuality::rmse) is added.  false: invalid input or no GPU; a message is
 *  printed, `distances` and `info` are unchanged.  The CLI prints one summary line per registered pair (reference = the target)
 *  when PLADE_M3C2=<radius>,<depth>[,<min_points>[,<reg_error>]] is set. */
bool compare_clouds(const Eigen::Matrix4f &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr reference_cloud,
                    pcl::PointCloud<pcl::PointNormal>::Ptr compared_cloud, double radius, double depth, std::vector<double> &distances,
                    CloudComparison *info = nullptr, int min_points = 4, double reg_error = 0.0);

/** Point descriptors (no counterpart in the reference): the fields of plade_fpfh_summary (include/plade_hip.h). */
struct CloudDescription {
    uint64_t n = 0, described = 0;   // points, those with a descriptor
    double mean_pairs = 0;           // the mean number of counted neighbour pairs of a described point
    uint32_t max_pairs = 0;          // the largest number of counted pairs of any point
};
/** FPFH descriptors on the GPU (plade_cloud_fpfh): `features` receives 33 floats per point of `cloud` -- three histograms of 11 bins
 *  over the neighbours closer than `radius` (absolute, in the cloud's units), each summing to 100; 33 NaNs where the point's normal
 *  is zero or not finite or it has fewer than min_pairs counted neighbour pairs.  false: invalid input or no GPU; a message is
 *  printed, `features` and `info` are unchanged. */
bool describe_cloud(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, double radius, std::vector<float> &features,
                    CloudDescription *info = nullptr, int min_pairs = 5);
/** The match of two tables of describe_cloud in feature space on the GPU (plade_match_features): `correspondences` receives the
 *  pairs (source point, target point), ascending in the source point, of the source points whose nearest target descriptor is
 *  kept: with `mutual` only when that target's nearest source is the point itself, with max_ratio > 0 only when the nearest
 *  distance is below max_ratio times the second nearest.  Points without a descriptor take no part.  false: invalid input or no
 *  GPU; a message is printed, `correspondences` is unchanged.  The CLI prints one summary line per pair when
 *  PLADE_FPFH_MATCH=<radius>[,<min_pairs>[,<max_ratio>]] is set. */
bool match_features(const std::vector<float> &source_features, const std::vector<float> &target_features,
                    std::vector<std::pair<int, int>> &correspondences, bool mutual = true, float max_ratio = 0.f);

/** A pose from correspondences (no counterpart in the reference): the fields of plade_corr_pose_result (include/plade_hip.h). */
struct PoseEstimate {
    uint64_t correspondences = 0;                                   // the list's length
    uint32_t hypotheses = 0, scored = 0;                            // drawn; those that passed the prerejection
    uint32_t best_hypothesis = 0, best_count = 0, inliers = 0;      // the winner, its count, the inliers of the refitted pose
    int refinements = 0;                                            // accepted least-squares refits
    double rmse = 0, fitness = 0;                                   // over the inliers; inliers / correspondences
};
/** The rigid source -> target pose from (source point, target point) correspondences on the GPU (plade_estimate_pose_corr): RANSAC
 *  over triples with an edge-length prerejection, an exhaustive count of the correspondences closer than inlier_dist (absolute) per
 *  surviving hypothesis, and a least-squares refit of the best one.  false: invalid input, no GPU, or no pose with min_inliers
 *  inliers; a message is printed, `transformation` and `info` are unchanged. */
bool estimate_pose_from_correspondences(Eigen::Matrix4f &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                                        pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud,
                                        const std::vector<std::pair<int, int>> &correspondences, double inlier_dist,
                                        PoseEstimate *info = nullptr, int min_inliers = 3, int hypotheses = 65536, uint64_t seed = 0);
/** Registers a pair that has no planes from its features, in one call on the GPU (plade_register_features): describe_cloud of both
 *  clouds at `radius`, their mutual match and estimate_pose_from_correspondences at inlier_dist, with the same bits as the three
 *  calls chained.  `correspondences` (optional) receives the matched pairs.  false as above, with every output unchanged.  The CLI
 *  does this for the pairs whose plane registration failed when PLADE_FEATURE_REGISTER=<radius>,<inlier_dist>[,<min_inliers>
 *  [,<hypotheses>]] is set. */
bool register_by_features(Eigen::Matrix4f &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                          pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud, double radius, double inlier_dist,
                          PoseEstimate *info = nullptr, std::vector<std::pair<int, int>> *correspondences = nullptr, int min_inliers = 3,
                          int hypotheses = 65536, int min_pairs = 5, uint64_t seed = 0);

/** Keypoints (no counterpart in the reference): the fields of plade_iss_summary (include/plade_hip.h). */
struct KeypointDetection {
    uint64_t n = 0, salient = 0, keypoints = 0;   // points, those that pass the eigenvalue tests, those that survive the suppression
    uint32_t max_count = 0;                       // the largest number of points within salient_radius of a point
};
/** ISS keypoints on the GPU (plade_cloud_keypoints_iss): `keypoints` receives, ascending, the points of `cloud` whose neighbourhood
 *  within salient_radius (absolute) varies in all three directions -- the eigenvalues l1 >= l2 >= l3 of its scatter about the point
 *  satisfy l2 < gamma21 l1, l3 < gamma32 l2 and l3 > 1e-9 l1 -- that have at least min_neighbours other points within
 *  non_max_radius (0: salient_radius) and the largest l3 among them.  Normals are not used.  false: invalid input or no GPU; a
 *  message is printed, `keypoints` and `info` are unchanged. */
bool detect_keypoints(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, double salient_radius, std::vector<int> &keypoints,
                      KeypointDetection *info = nullptr, double non_max_radius = 0.0, int min_neighbours = 5, double gamma21 = 0.975,
                      double gamma32 = 0.975);
/** register_by_features with the detector in front of the match, in one call on the GPU (plade_register_keypoints): only the
 *  source's keypoints are matched, against every described target point, so the match costs a few per cent of the full one.
 *  `correspondences` (optional) receives the matched pairs in the clouds' own indices, `detection` the detector's summary.  false as
 *  there, with every output unchanged.  The CLI does this in place of register_by_features when
 *  PLADE_FEATURE_KEYPOINTS=<salient_radius>[,<non_max_radius>[,<min_neighbours>]] is set next to PLADE_FEATURE_REGISTER. */
bool register_by_keypoints(Eigen::Matrix4f &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                           pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud, double radius, double inlier_dist, double salient_radius,
                           PoseEstimate *info = nullptr, KeypointDetection *detection = nullptr,
                           std::vector<std::pair<int, int>> *correspondences = nullptr, double non_max_radius = 0.0, int min_neighbours = 5,
                           int min_inliers = 3, int hypotheses = 65536, int min_pairs = 5, uint64_t seed = 0);

/** Merging registered clouds (no counterpart in the reference): the fields of plade_merge_summary (include/plade_hip.h). */
struct CloudMerge {
    uint64_t n_in = 0, n_out = 0, n_shared = 0;   // points in, rows out, rows to which two or more clouds contributed
    uint32_t max_count = 0;                       // the largest number of points fused into one row
};
/** Merges 1..16 clouds on the GPU (plade_merge_clouds): cloud c is taken into the common frame by transformations[c] (an empty
 *  vector: identities), and the points of every voxel of edge `leaf` are fused into one -- the mean position and the normalised
 *  sum of the finite normals (opposite normals cancel: NaN), both summed in fp64 in a fixed order; leaf = 0 concatenates.  false:
 *  invalid input or no GPU; a message is printed and `merged` is unchanged.  The CLI writes the merged target and source of every
 *  registered pair, in the target file's frame, when PLADE_MERGE=<leaf> is set, and prints one line per pair. */
bool merge_clouds(const std::vector<pcl::PointCloud<pcl::PointNormal>::Ptr> &clouds, const std::vector<Eigen::Matrix4f> &transformations,
                  float leaf, pcl::PointCloud<pcl::PointNormal> &merged, CloudMerge *info = nullptr);

/** Batch extension (no counterpart in the reference, whose batch mode is a plain loop of the file overload above,
 *  code/PLADE/main.cpp:122-148): `count` (1..registration_group_max = PLADE_GROUP_MAX) consecutive pairs of the list as ONE group.  Every pair gets the result,
 *  the messages and the identity-on-failure of the file overload -- its transformation is bit for bit the one the file overload
 *  returns -- but the plane extraction of all clouds of the group is one GPU launch sequence (plade_registration_pairs,
 *  include/plade_hip.h).  out[i] / err[i]: where pair i's console messages go (nullptr: std::cout / std::cerr). */
constexpr size_t registration_group_max = 8;
void registration_group(size_t count, Eigen::Matrix<float, 4, 4> *transformations, const std::string *target_cloud_files,
                        const std::string *source_cloud_files, bool *ok, std::ostream *const *out, std::ostream *const *err);

/** load_ply_cloud (code/PLADE/util.cpp:1505-1546): ascii / binary PLY with x y z nx ny nz. */
bool load_ply_cloud(const std::string &file_name, pcl::PointCloud<pcl::PointNormal> &cloud);

/** Select the GPU used by the calling thread's registrations (default 0). */
void plade_select_device(int device);
/** PLADE_TRACE_CLI=1: a time-stamped line on std::cerr (seconds since the first such call). */
void plade_cli_trace(const char *what);
/** GPUs this process sees (0 without one): the CLI's batch mode spreads the list over all of them by default. */
int plade_gpu_count();

/** Console of the calling thread's registrations: the messages the reference prints on std::cout / std::cerr go to
 *  these streams instead (nullptr = std::cout / std::cerr again).  Used by the CLI's batch workers. */
void plade_set_thread_console(std::ostream *out, std::ostream *err);

/** PLADE_MERGE: the result file whose name the merged clouds of the calling thread's registrations take -- <result_file>.merged.ply
 *  with first_pair < 0, <result_file>.<first_pair + i>.merged.ply for pair i of a registration_group call (an empty name: no
 *  merged cloud is written).  Used by the CLI. */
void plade_set_thread_merge_output(const std::string &result_file, long first_pair);

/** Destroy the calling thread's GPU context (it is created on first use and otherwise lives as long as the thread). */
void plade_release_thread_context();

#endif  // PLADE_H
