/* include/plade_hip.h -- C ABI of libplade_hip.so, the MI355X (gfx950) implementation of
 * PLADE's registration hot path.  Plain pointers and sizes only; every entry point
 * returns 0 on success and a negative PLADE_E* code on failure (never throws).
 *
 * The reference (chsl/PLADE) has no FFI layer; these symbols are cut at the internal
 * seams listed in SURVEY.md section 8b.  Each declaration cites the reference
 * interface it replaces (paths relative to the reference tree).
 *
 * Host pointers unless a parameter is documented as a plade_cloud handle.
 * One plade_ctx per host thread / device stream; a ctx is not re-entrant.
 */
#ifndef PLADE_HIP_H
#define PLADE_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PLADE_OK 0
#define PLADE_EINVAL (-1)   /* bad argument */
#define PLADE_EDEVICE (-2)  /* HIP runtime error / no gfx950 device */
#define PLADE_ECAP (-3)     /* caller-provided capacity too small */
#define PLADE_EFAIL (-4)    /* registration failed (reference returns false) */
#define PLADE_ELIMIT (-5)   /* internal limit exceeded */

#define PLADE_GROUP_MAX 8   /* pairs per group of plade_registration_pairs */

typedef struct plade_ctx plade_ctx;
typedef struct plade_cloud plade_cloud; /* device-resident oriented point cloud */
typedef struct plade_comm plade_comm;   /* RCCL communicator of this rank (multi-GPU), see below */

/* Context: owns the HIP stream, scratch pools and the debug dump. */
int plade_ctx_create(int device, plade_ctx **out);
void plade_ctx_destroy(plade_ctx *ctx);
const char *plade_last_error(const plade_ctx *ctx);
const char *plade_version(void);
/* hipDeviceSynchronize on `device`: everything this process has queued there has finished (benchmark brackets). */
int plade_device_synchronize(int device);
/* GPUs this process sees (hipGetDeviceCount; 0 without a GPU or a HIP runtime): the CLI's batch mode spreads the pairs of the
 * list (the loop code/PLADE/main.cpp:122-148) over all of them by default. */
int plade_device_count(void);

/* Tunables that are hard-coded literals in the reference (defaults = reference values):
 *   max_planes      40     code/PLADE/plade.cpp:604   (extract(): top-40 cap)
 *   min_planes      10     code/PLADE/plade.cpp:603
 *   max_candidates  200    code/PLADE/plade.cpp:54    (maxCandidateResultNum)
 *   init_min_support 10000 code/PLADE/plade.cpp:602
 *   orient_normals  0      0 = reference behaviour (plane_extraction.cpp:43-58: correct_normal divides by a
 *                          counter that stays 0, so its average normal is NaN and the test never flips:
 *                          the plane normal keeps the sign of the LS-fit eigenvector); 1 = the evident
 *                          intent: flip (n, d) so that n agrees with the mean normal of the plane's inliers.
 *                          The C ABI never looks at the environment for anything that selects a result or an algorithm
 *                          (only PLADE_TRACE_* / PLADE_DEBUG_* printing and A/B timing hooks); the C++
 *                          API / CLI (plade_host.cpp) turn it on with env PLADE_ORIENT_NORMALS=1.
 *   unoriented_normals 0   1 = the "unoriented normals" mode README.md:109-110 describes: every plane takes part
 *                          with both orientations (2x planes, ~4x line pairs / descriptors), so a pair registers
 *                          whatever the signs of the extracted plane normals are.  C++ API / CLI: env PLADE_UNORIENTED_NORMALS=1.
 *   ransac_seed     fixed  the reference seeds from time(NULL) (RansacShapeDetector.cpp:463-464)
 *   dump            0      bit 0: keep named intermediates for plade_dump_get (tests); bit 1 (2): time the scan kernels
 *                          (HIP events on the launch stream + the kernel's own clock; the extraction loop is then
 *                          launched kernel by kernel); bits 1 + 2 (6): the kernel's own clock only, inside the captured
 *                          graph of the iteration as the unprofiled path launches it (bench.py's roofline leg)
 *   ransac_topup    1      schedule of the plane extraction's hypothesis rounds.  1 = every iteration draws a round and
 *                          what the previous batch left of the candidate pool competes with the new draws (the
 *                          reference's loop generates candidates in every pass, RansacShapeDetector.cpp:548-617);
 *                          0 = a round is drawn only when the pool is empty: strict best-first acceptance, two more
 *                          launches per iteration and more iterations.  Same acceptance semantics; which of two touching
 *                          faces takes contested points can differ (tests/test_gpu_golden.py).
 *   match_window    0      enumeration of the descriptor match (seam S2): 0 = brute force up to 2e10 descriptor pairs,
 *                          length-windowed above; 1 = always windowed; -1 = never.  The lists are identical either way.
 *   match_cell_budget 0    (query, chunk) cells per slab of the windowed enumeration; 0 = 2^26.  Test hook.
 *   prepare_sides   0      what the two clouds of a pair go through between plane extraction and descriptor match (downsampling,
 *                          boxes, grids, line pairs): 1 = side by side (source on an auxiliary stream + host thread: the shortest
 *                          single registration), 2 = one after the other on the context's stream (fewer streams and threads: the
 *                          higher batch throughput), 0 = 2 inside a group of several pairs or with host_wait != 0, else 1.
 *                          Results do not depend on it.
 *   group_max_points 48e6  points of all clouds that go through ONE extraction sequence of plade_registration_pairs*: a group
 *                          that holds more is registered in consecutive parts within this budget (the extraction's work area
 *                          takes ~0.9 KB of HBM per point it serves at once); results do not depend on it.  0 = default. */
typedef struct plade_params {
    int32_t max_planes;
    int32_t min_planes;
    int32_t max_candidates;
    int32_t init_min_support;
    int32_t orient_normals;
    int32_t dump;
    uint64_t ransac_seed;
    int32_t host_wait;   /* how the calling thread waits for the GPU: 0 = spin (lowest latency; the HIP runtime keeps
                          * one CPU busy per waiting thread), 1 = poll + 50-100 us sleeps (throughput mode: many
                          * contexts in flight per CPU), 2 = as 1 and the next plane-extraction iteration is
                          * queued before the current one has reported (a few contexts per GPU whose stream would
                          * otherwise idle while the host sleeps; with >= 8 in flight the empty speculative
                          * iteration costs more than it hides).  C++ API / CLI: env PLADE_HOST_WAIT=spin|sleep. */
    int32_t unoriented_normals;
    int32_t ransac_topup;
    int32_t match_window;
    uint32_t match_cell_budget;
    uint32_t group_max_points;
    int32_t prepare_sides;
    int32_t closest_point_mode;   /* arithmetic of ComputeNearstTwoPointsOfTwo3DLine (code/PLADE/util.cpp:1167-1229) and
                          * ComputeIntersectionPointOf23DLine (util.cpp:1461-1500): 1 = "svd_fp32" (DEFAULT = the reference's own
                          * arithmetic): cv::solve(A, B, X, DECOMP_SVD) on the 9 x 9 / 6 x 5 float systems, rounding for rounding
                          * (opencv/modules/core/src/lapack.cpp:533-710, 751-812, 1335-1460; one system per lane,
                          * plade_amd/csrc/k_svd.h); 0 = exact closed form in fp64: the better-conditioned evaluation of the
                          * same inputs, an OPT-IN deviation (like orient_normals = 1) -- on axis-aligned scenes the
                          * reference's solves are ill-conditioned and the two modes part.
                          * C++ API / CLI: env PLADE_CLOSEST_POINT_MODE=closed_form. */
} plade_params;
void plade_default_params(plade_params *p);
int plade_set_params(plade_ctx *ctx, const plade_params *p);

/* ---- seam S1a: plane scoring ------------------------------------------------------------
 * Replaces m_shape->Visit(&scoreVisitor) (code/3rd_party/ransac/Candidate.h:174,290) =
 * ScorePrimitiveShapeVisitorImpl::operator() (ransac/ScorePrimitiveShapeVisitor.h:39-46) with
 * FlatNormalThreshPointCompatibilityFunc (ransac/FlatNormalThreshPointCompatibilityFunc.h:14-23):
 * inlier <=> shape_index[i] == -1 && |dist - n.p_i| < eps && |n.n_i| >= cos_thresh.
 * pos_nrm: N x 6 (x y z nx ny nz); shape_index may be NULL (all unassigned);
 * planes: H x 4 = (n, dist = n.p0); counts: H; idx_out (optional): H x cap, ascending point
 * index per hypothesis (rows are truncated at cap; counts stay exact). */
int plade_score_planes(plade_ctx *ctx, const float *pos_nrm, const int32_t *shape_index, uint32_t n,
                       const float *planes, uint32_t h, float eps, float cos_thresh,
                       uint32_t *counts, uint32_t *idx_out, uint32_t cap);
/* The same visitor over a SUBSET of the cloud -- the call shape of candidate generation and bound refinement:
 * Candidate::ImproveBounds(..., maxSubset = 1) scores H new hypotheses on subset 0 only
 * (ransac/RansacShapeDetector.cpp:163 -> Candidate.h:154-179, one nested random subset per call); the GPU loop
 * scores a sampling round on a stratified subset in one launch.  sub_index: m point indices (< n, any order,
 * repeats allowed); counts[j] = #{ s < m : shape_index[sub_index[s]] == -1 and point sub_index[s] is compatible
 * with hypothesis j }; *n_unassigned (optional) = #{ s : shape_index[sub_index[s]] == -1 } (the loop's estimate of
 * the support on the whole cloud scales the counts by remaining / this). */
int plade_score_planes_subset(plade_ctx *ctx, const float *pos_nrm, const int32_t *shape_index, uint32_t n,
                              const uint32_t *sub_index, uint32_t m, const float *planes, uint32_t h, float eps,
                              float cos_thresh, uint32_t *counts, uint32_t *n_unassigned);

/* ---- seam S1c: connected component + LS refit of one plane candidate ---------------------
 * Replaces PlanePrimitiveShape/BitmapPrimitiveShape::ConnectedComponent
 * (ransac/BitmapPrimitiveShape.cpp:97-265, PlanePrimitiveShape.cpp:164-207), followed by
 * PlanePrimitiveShape::LSFit (PlanePrimitiveShape.cpp:98-111 -> Plane::LeastSquaresFit, Plane.cpp:169-176)
 * and Candidate::WeightedScore (Candidate.cpp:77-87) on the kept points -- the per-slot body of the
 * acceptance loop RansacShapeDetector.cpp:618-656.
 * plane = Plane(point, normal); idx: m distinct point indices (the score list, any order); kept_out (cap m):
 * the indices of the largest 8-connected bitmap component in list order, n_kept their number;
 * fit_out[7] = LS plane of the kept points (unit normal, mean, dist = mean.normal);
 * wscore_out = sum over kept points of exp(-d^2 / (2/9 w_eps^2)) against the INPUT plane. */
int plade_plane_component(plade_ctx *ctx, const float *pos_nrm, uint32_t n, const float normal[3],
                          const float point[3], const int32_t *idx, uint32_t m, float bitmap_eps,
                          int closing_filter, float w_eps, int32_t *kept_out, uint32_t *n_kept,
                          float *fit_out, double *wscore_out);

/* ---- seam S1b: whole plane-extraction stage --------------------------------------------
 * Replaces PlaneExtraction::detect (code/PLADE/plane_extraction.cpp:173-200 -> :61-168 ->
 * RansacShapeDetector::Detect, ransac/RansacShapeDetector.cpp:455-907).
 * dist_rel/bitmap_rel are relative to max(dx,dy) of the bbox (the reference's Z-ignoring scale,
 * plane_extraction.cpp:71-80).  Output: planes_out P x 4 = (unit n, d = -n.p); offsets_out P+1;
 * idx_out = original point indices of each plane's support (capacity n). */
int plade_extract_planes(plade_ctx *ctx, const float *pos_nrm, uint32_t n, uint32_t min_support,
                         float dist_rel, float bitmap_rel, float cos_thresh, float overlook_p,
                         float *planes_out, int32_t *offsets_out, int32_t *idx_out,
                         uint32_t max_planes, uint32_t *n_planes_out);

/* ---- seam S2: descriptor match ------------------------------------------------------------
 * Replaces the kdtree22.find_neighbors loop (code/PLADE/util.cpp:133-293, call at :163) =
 * KdTreeSearchNDim<VectorXf,8>::find_neighbors(p, 0, radius, ...) (ann_1.1.2/include/ANN/ANN.h:
 * 978-1029): all target descriptors with sum_d (double(q_d)-double(t_d))^2 <= double(float(r*r)).
 * Output sorted by (query, dist2, target index); offsets: Dq+1; t_idx/dist2 capacity `cap`
 * (may be NULL with cap 0 to size the result); *n_pairs receives the exact total. */
int plade_match_descriptors(plade_ctx *ctx, const float *src, uint32_t ds, const float *tgt,
                            uint32_t dt, float radius, int64_t *offsets, uint32_t *t_idx,
                            double *dist2, uint64_t cap, uint64_t *n_pairs);

/* ---- seam S3: candidate verification ------------------------------------------------------
 * Replaces the loop code/PLADE/plade.cpp:547-564: per candidate k,
 *   count_k = #{ p in src_ds : exists t in tgt_ds with |t - c_k|^2 < float(R^2) and
 *                              |t - T_k p|^2 < float(leaf^2) }
 * (ComputeOverlap, code/PLADE/util.h:611-647; pcl transformPointCloud, FLANN strict <).
 * T: K x 16 row-major; centers: K x 3 (= R c_s + T, formed by the caller as plade.cpp:555);
 * counts[k] = -1 when the coarse sphere holds no target point (overlap ratio 0). */
int plade_overlap_counts(plade_ctx *ctx, const float *src_ds, uint32_t n_s, const float *tgt_ds,
                         uint32_t n_t, const float *T, uint32_t k, const float *centers,
                         float src_radius, float inlier_dist, int32_t *counts);

/* ---- seam of the clustering stage (A9) ------------------------------------------------------
 * Replaces ClusterTransformation (code/PLADE/util.cpp:1245-1277) = pcl::ConditionalEuclideanClustering::segment
 * (pcl-1.8.1/segmentation/include/pcl/segmentation/impl/conditional_euclidean_clustering.hpp:42-138) with the condition
 * EnforceSimilarity (util.cpp:1232-1243): candidates a, b are joined when |t_a - t_b|^2 < float(dist_threshold^2) and
 * |euler_a - euler_b|^2 < angle_gate; clusters = connected components.  t_xyz, euler: m x 3 (translation; roll, pitch,
 * yaw as pcl::getEulerAngles gives them); cluster_of[i] = index of i's cluster, clusters numbered by their smallest
 * member (the order PCL creates them in). */
int plade_cluster_transforms(plade_ctx *ctx, const float *t_xyz, const float *euler, uint32_t m, float dist_threshold,
                             float angle_gate, int32_t *cluster_of, uint32_t *n_clusters);

/* ---- seam of the penetration filter (A11) -------------------------------------------------------
 * Replaces the loop code/PLADE/util.cpp:450-519 around AreTwoPlanesPenetrable (util.cpp:1279-1458) on the filter's own
 * tables: cand = K x 12 (R row-major, then T); per side (s_ = source, t_ = target) coef P x 4, center P x 3, four P x 12
 * (the plane's projected rectangle), pts = the per-plane downsampled clouds end to end (x, y, z), off = P + 1 offsets into
 * them (points).  flags[k] = 1 when candidate k has a penetrating plane pair.  PLADE_ELIMIT when a common segment is
 * longer than 1024 search steps.
 * items != NULL asks for the AUDIT: one plade_pen_item per (candidate, source plane, target plane) that reached the walks
 * (in no particular order; *n_items of them, PLADE_ECAP when items_cap is smaller; K * ps * pt always suffices), and every
 * such item is then evaluated in full -- no early exit once its candidate is flagged, the second walk also behind a failed
 * first one.  plane1 = the transformed source plane, start / direc / length = the common segment, nsteps = the search
 * steps with dist < length; pass 0 classifies the transformed source points against the target plane behind the target
 * cloud's gate, pass 1 the other way round: pos / neg = points on either side, gated = the steps whose gate found two
 * points; verdict = 1 when the pair penetrates. */
typedef struct plade_pen_item {
    uint32_t k, i1, j1;
    float plane1[4], start[3], direc[3], length;
    int32_t nsteps, pos[2], neg[2], gated[2], verdict;
} plade_pen_item;
int plade_penetration_filter(plade_ctx *ctx, const float *cand, uint32_t K, const float *s_coef, const float *s_center,
                             const float *s_four, const float *s_pts, const uint32_t *s_off, uint32_t ps,
                             const float *t_coef, const float *t_center, const float *t_four, const float *t_pts,
                             const uint32_t *t_off, uint32_t pt, float length_threshold, float angle_threshold,
                             int32_t *flags, plade_pen_item *items, uint64_t items_cap, uint64_t *n_items);

/* ---- seams of the line geometry (A6 / A11) ------------------------------------------------------
 * plade_closest_points replaces ComputeNearstTwoPointsOfTwo3DLine (code/PLADE/util.cpp:1167-1229) for n line pairs:
 * u1, u2 (n x 3, directions: normalised first, as the reference does in place), p1, p2 (n x 3, a point of each line) ->
 * q1, q2 (n x 3, the closest points), len (n doubles: (q1 - q2).norm() in float, widened), ok (n: 0 where the two
 * normalised directions are bitwise equal -- the reference returns -1 there -- else 1).
 * plade_lines_meet replaces ComputeIntersectionPointOf23DLine (util.cpp:1461-1500): v1, v2 are used as given;
 * ok = 0 where |v1 . v2| > 0.9999.
 * mode: 0 = closed form (fp64), 1 = the reference's cv::solve(DECOMP_SVD) in float (plade_params.closest_point_mode). */
int plade_closest_points(plade_ctx *ctx, int32_t mode, const float *u1, const float *p1, const float *u2, const float *p2,
                         uint32_t n, float *q1, float *q2, double *len, int32_t *ok);
int plade_lines_meet(plade_ctx *ctx, int32_t mode, const float *v1, const float *p1, const float *v2, const float *p2,
                     uint32_t n, float *out, int32_t *ok);

/* ---- supporting stage entry points (A13) ------------------------------------------------- */
/* average_spacing(cloud, k) (code/PLADE/util.cpp:1619-1648); xyz read with `stride` floats. */
int plade_average_spacing(plade_ctx *ctx, const float *xyz, uint32_t n, uint32_t stride,
                          uint32_t k, uint32_t samples, float *spacing_out);
/* DownSamplePointCloud -> pcl::VoxelGrid (code/PLADE/util.h:161-184); out capacity n. */
int plade_voxel_downsample(plade_ctx *ctx, const float *xyz, uint32_t n, uint32_t stride, float leaf,
                           float *out_xyz, uint32_t *n_out);

/* ---- registration() overloads (code/PLADE/plade.h) ---------------------------------------- */
/* plade.h:74-79  registration(T, target, source, target_planes, source_planes) -- the
 * deterministic parity boundary.  planes: P x 4 (n, d), offsets P+1, idx. T16: row-major 4x4. */
int plade_registration_planes(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t,
                              const float *src_pos_nrm, uint32_t n_s, const float *tgt_planes,
                              const int32_t *tgt_offsets, const int32_t *tgt_idx, uint32_t p_t,
                              const float *src_planes, const int32_t *src_offsets,
                              const int32_t *src_idx, uint32_t p_s, float *T16);
/* plade.h:58-61  registration(T, target, source): auto-tuned plane extraction (plade.cpp:602-662) */
int plade_registration(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t,
                       const float *src_pos_nrm, uint32_t n_s, float *T16);
/* The same call in BATCH mode (code/PLADE/main.cpp:97-158: a plain loop of registration() over the pairs of
 * file_pairs.txt).  Registers (tgt, src) exactly like plade_registration and, before it starts computing, queues the
 * upload of the pair the NEXT call on this ctx will be handed (next_*; NULL / 0 = none) on a stream of its own, so that
 * the PCIe transfer of pair i+1 runs under the kernels of pair i.  The next call recognises its clouds by pointer and size
 * and skips its upload; any other pair is uploaded as usual.  The caller must leave the next_* buffers untouched until
 * that call (page-lock them with plade_host_pin for a truly asynchronous copy).  Results are identical to
 * plade_registration's. */
int plade_registration_next(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t,
                            const float *src_pos_nrm, uint32_t n_s, const float *next_tgt_pos_nrm,
                            uint32_t next_n_t, const float *next_src_pos_nrm, uint32_t next_n_s, float *T16);
/* Batch mode, `count` (1..PLADE_GROUP_MAX) consecutive pairs of the list per call (the loop of code/PLADE/main.cpp:122-148
 * taken up to PLADE_GROUP_MAX pairs at a time).  Every pair is registered exactly like plade_registration -- results are bit-identical to
 * registering it alone -- but the plane extraction of all clouds of the group (PlaneExtraction::detect x 2 count) is ONE launch
 * sequence: its ~150 kernels per cloud pair are short and mostly latency-bound, and carrying the clouds of up to 8 pairs per
 * launch divides the commands, host waits and much of the GPU time per registration (~0.9 GB of HBM per cloud of the group); behind the extraction the pairs proceed
 * concurrently, pairs 1.. on internal peer contexts (plade_pair_ctx).  tgt_pos_nrm / src_pos_nrm: count pointers to N x 6 arrays, n_t / n_s their point
 * counts; next_*: the clouds the NEXT call on this ctx will be handed (next_count = 0: none), prefetched as
 * plade_registration_next does.  T16: count x 16 (identity where a pair fails); status[i]: PLADE_OK, PLADE_EFAIL (the
 * reference returns false) or another PLADE_E* code for pair i.  The return value reports errors that concern the whole
 * call (bad arguments, upload, plane extraction); plade_last_error(plade_pair_ctx(ctx, i)) has pair i's message. */
int plade_registration_pairs(plade_ctx *ctx, uint32_t count, const float *const *tgt_pos_nrm, const uint32_t *n_t,
                             const float *const *src_pos_nrm, const uint32_t *n_s, uint32_t next_count,
                             const float *const *next_tgt_pos_nrm, const uint32_t *next_n_t,
                             const float *const *next_src_pos_nrm, const uint32_t *next_n_s, float *T16, int32_t *status);
/* The context that carried pair `index` of the last plade_registration_pairs* call on ctx (0: ctx itself; 1..: its peers, NULL
 * before the first call with that many pairs): stats, dump and last error of that pair are read from it with the entry points below.
 * Borrowed -- it is destroyed with ctx; do not register on it. */
plade_ctx *plade_pair_ctx(plade_ctx *ctx, uint32_t index);
/* plade.h:91-96  registration(T, target, source, min_support_target, min_support_source) */
int plade_registration_minsupport(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t,
                                  const float *src_pos_nrm, uint32_t n_s, int32_t min_support_t,
                                  int32_t min_support_s, float *T16);

/* ---- second sharding axis: the candidates of ONE pair over several GPUs -------------------------------------
 * The K candidate transforms of the verification loop (code/PLADE/plade.cpp:547-564) are independent.  With a shard set, a
 * registration whose verification holds at least `min_candidates` candidates scores only candidates k with k % world == rank
 * on this context's GPU (every rank runs the same registration on its own copy of the pair, so all ranks hold the same
 * candidate list) and then calls `exchange`: values holds `count` int32 words of which this rank has filled those at indices
 * i with (i % (count / 2)) % world == rank (first half: counts, second half: sphere flags); on return ALL words must be
 * valid on every rank (an all-gather: RCCL / MPI / torch.distributed, the caller's choice -- the library itself links no
 * communication library).  exchange returns 0 on success.  world <= 1 or exchange == NULL switches the axis off. */
typedef int (*plade_exchange_fn)(void *user, int32_t *values, uint32_t count, uint32_t rank, uint32_t world);
int plade_set_candidate_shard(plade_ctx *ctx, uint32_t rank, uint32_t world, uint32_t min_candidates, plade_exchange_fn exchange,
                              void *user);
/* The shard applies to calls that register ONE pair (plade_registration, _next, _dev, _planes, _minsupport and groups of
 * one); inside a group of several pairs (plade_registration_pairs* with count > 1) it is switched off for the call: the pairs'
 * tails run on concurrent threads, and collectives entered from several threads in an order that may differ between the
 * ranks would mismatch -- a batch shards whole pairs over the ranks instead. */

/* ---- RCCL communicator (multi-GPU): one process per GPU, ranks of one node over xGMI ---------------------------
 * The two exchange steps of the path -- the 68 bytes of result per pair that batch mode gathers once per batch (the loop
 * code/PLADE/main.cpp:122-148 sharded pair i -> rank i % world) and the 8 bytes per candidate of the candidate shard above --
 * are each ONE ncclAllGather.  librccl is opened with dlopen() on first use: a single-GPU host never loads it and the library
 * keeps no link dependency on it.
 *   plade_comm_unique_id   rank 0: 128 bytes (ncclGetUniqueId) that the host hands to every rank of the job by its own means
 *                          (bench.py / plade_amd.rccl_comm: the ranks' rendezvous file; MPI_Bcast; a pipe)
 *   plade_comm_create      every rank, collectively: ncclCommInitRank on `device`
 *   plade_comm_all_gather  send: `bytes` bytes of this rank (host memory), recv: world x bytes in rank order (host memory);
 *                          staged through device memory, one ncclAllGather, blocking.  A barrier is an all-gather of one word.
 *   plade_set_candidate_shard_comm   the candidate shard with the library doing the exchange itself: the counts the
 *                          verification kernel wrote stay in device memory, one ncclAllGather on the context's stream behind that
 *                          kernel, one read-back of all ranks' counts -- no host callback.  comm == NULL switches the axis off (a
 *                          communicator of one rank still runs the exchange: that is how a one-GPU box tests it).  The communicator must outlive its use by the context and serve one call at a time.
 * Errors: PLADE_EDEVICE (no librccl, RCCL error; plade_comm_last_error(comm or NULL) has the text). */
#define PLADE_COMM_ID_BYTES 128
int plade_comm_unique_id(void *id128);
int plade_comm_create(int device, uint32_t rank, uint32_t world, const void *id128, plade_comm **out);
int plade_comm_all_gather(plade_comm *comm, const void *send, void *recv, uint64_t bytes);
void plade_comm_destroy(plade_comm *comm);
const char *plade_comm_last_error(const plade_comm *comm);
int plade_set_candidate_shard_comm(plade_ctx *ctx, plade_comm *comm, uint32_t min_candidates);

/* Optional page-locking of caller-owned cloud buffers (hipHostRegister / hipHostUnregister): the host-pointer overloads
 * above then upload by asynchronous DMA instead of through the runtime's bounce buffer.  The reference has no counterpart
 * (its clouds never leave host memory); a host that keeps its PLY staging buffers alive pins them once. */
int plade_host_pin(plade_ctx *ctx, const void *ptr, size_t bytes);
int plade_host_unpin(plade_ctx *ctx, const void *ptr);

/* Device-resident clouds: upload once, register many times (bench: inputs resident in HBM). */
int plade_cloud_upload(plade_ctx *ctx, const float *pos_nrm, uint32_t n, plade_cloud **out);
void plade_cloud_free(plade_ctx *ctx, plade_cloud *c);
int plade_registration_dev(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, float *T16);
/* plade_registration_pairs on resident clouds */
int plade_registration_pairs_dev(plade_ctx *ctx, uint32_t count, plade_cloud *const *tgt, plade_cloud *const *src, float *T16,
                                 int32_t *status);

/* ---- normal estimation: clouds without normals (no reference counterpart: the reference requires oriented normals in its
 * input, README "should provide oriented point normals", and rejects a PLY without them, code/PLADE/util.cpp:1533-1536) -----
 * Semantics, exact where a CPU restatement can check them bit for bit (plade_amd/csrc/normals.h):
 *   neighbours   the k_eff = min(k, n) points j -- i itself included -- with the smallest d(i, j) = fp32 FLANN L2 of (p_i, p_j)
 *                ((dx*dx + dy*dy) + dz*dz), ties broken by the smaller original index j; listed in ascending (d, j) order
 *   PCA          fp64 on the neighbours' coordinates relative to p_i, accumulated in the listed order (centroid, then the
 *                covariance about it); normal = unit eigenvector of the smallest eigenvalue l0, written as fp32; curvature =
 *                l0 / (l0 + l1 + l2).  Independent of launch shape, grid cell size and what else is in flight.
 *   orientation  n is flipped when (v - p_i) . n < 0 (PCL's flipNormalTowardsViewpoint); viewpoint NULL = (0, 0, 0), the
 *                sensor origin of a scan in its own frame
 *   degenerate   k_eff < 3 or a covariance that is exactly zero (all neighbours coincide): normal and curvature NaN -- such points
 *                never pass the plane tests of the registration (a NaN comparison is false)
 * Errors: PLADE_EINVAL for n = 0, k outside [3, 64], stride < 3, a non-finite coordinate or viewpoint; the context stays usable.
 * plade_estimate_normals   xyz: n points of `stride` floats (host).  pos_nrm_out: n x 6 (x y z copied, nx ny nz); curvature_out
 *                          (n floats) and nbr_out (n x k int32: the neighbour list, -1 behind the k_eff entries when n < k) may be
 *                          NULL.  plade_stats_get then reports normals_grid_s / normals_search_s (HIP events on the context's
 *                          stream: grid build including its host waits below, search + PCA), normals_grid_builds and
 *                          normals_ring_queries (points the 27-cell search could not finish).
 * plade_cloud_upload_xyz   the same estimate straight into a resident cloud (plade_cloud_upload's layout): the coordinates are
 *                          uploaded once and the normals never leave the device.  The call still waits on the host several times
 *                          for small results: the bounding box, the occupied-cell count of each grid build (up to four builds
 *                          while the cell is adapted), the end of the estimate and the cloud's own bounding box.  Register the
 *                          cloud with plade_registration_dev / plade_registration_pairs_dev, free it with plade_cloud_free. */
int plade_estimate_normals(plade_ctx *ctx, const float *xyz, uint32_t n, uint32_t stride, int32_t k, const float *viewpoint,
                           float *pos_nrm_out, float *curvature_out, int32_t *nbr_out);
int plade_cloud_upload_xyz(plade_ctx *ctx, const float *xyz, uint32_t n, uint32_t stride, int32_t k, const float *viewpoint,
                           plade_cloud **out);

/* ---- fine alignment: point-to-plane ICP after the coarse registration (no reference counterpart: the reference returns the
 * Umeyama fit of its matched descriptors and refines nothing) -------------------------------------------------------------
 * Semantics (plade_amd/csrc/icp.h).  Target: n_t points x y z nx ny nz; source: its x y z (normals ignored);
 * T_in: source -> target, row-major 4 x 4 like plade_registration's T16.  D = the diagonal of the target's bounding box; a
 * parameter that is 0 takes the automatic value in brackets.
 *   sample       S = plade_voxel_downsample of the source's x y z with leaf source_leaf [0.005 D]
 *   iterate      T_k in fp64, T_0 = T_in; the stage distance d starts at max_dist [0.025 D]
 *   centre       s-bar = the fp64 mean of S (summed once in a fixed order), c_k = T_k s-bar in fp64
 *   match        p' = fp32(R) s + fp32(t), each row ((r0 x + r1 y) + r2 z) + t in fp32; j = the argmin over ALL target points
 *                of (fp32 FLANN L2 (p', q_j), j); s has a correspondence when that distance < (float)d * (float)d and n_j is
 *                finite.  An exact set: independent of grid cell sizes and launch shapes.
 *   linearise    fp64 over the correspondences, p = T_k double(s): r = n . (p - q), J = [(p - c_k) x n, n]; the 21 values of J^T J, the 6 of
 *                J^T r, sum r^2 and the count, summed in a fixed order (bit-identical from run to run)
 *   solve        J^T J x = -J^T r by fp64 Cholesky; pivot j <= 1e-12 A[j][j] (its own diagonal entry, so an exactly zero column
 *                counts) is a degenerate geometry; the test does not depend on the units or the distance from the origin
 *   update       T_{k+1} = [R | (c_k - R c_k) + x3..5] T_k, R = Rodrigues(x0..2): a rotation about c_k; x3..5 moves the centre
 *   tolerances   with A = the target's max |coordinate|, the effective tolerances are eps_t = max(eps_translation, 4 2^-23 A) and
 *                eps_r = max(eps_rotation, 4 2^-23 A / D), given values included: no step can shrink below the fp32 resolution of
 *                the coordinates, so a tighter tolerance would only run the loop to max_iterations
 *   schedule     a stage converges when |x0..2| < eps_r [1e-6 rad] and |x3..5| < eps_t [1e-6 D]; then
 *                d = max(min_dist, d / 2) while d > min_dist [0.0025 D], else stop with converged = 1; at most max_iterations
 *                [60] updates in all (then converged = 0, still PLADE_OK, T_out = the last iterate)
 *   failure      PLADE_EFAIL and T_out = T_in when an iteration has fewer than min_correspondences [100] correspondences
 *                (failure = PLADE_ICP_TOO_FEW) or a degenerate system (PLADE_ICP_DEGENERATE, e.g. a single plane)
 *   output       T_out: fp32 of the fp64 iterate; the result's correspondences, rmse = sqrt(sum r^2 / count) and fitness =
 *                count / |S| are those of the last linearisation
 * Errors: PLADE_EINVAL for NULL pointers, n = 0, non-finite coordinates or T_in, negative or non-finite parameters, min_dist >
 * max_dist, more than 16 stages (max_dist / min_dist > 2^15); the context stays usable.  plade_stats_get then reports
 * icp_sample_s, icp_grid_s (one target grid per stage), icp_loop_s and icp_iterations (HIP events on the context's stream).  The
 * loop queues max_iterations pairs of kernels without a host wait between them and reads T and the result back once. */
#define PLADE_ICP_TOO_FEW 1
#define PLADE_ICP_DEGENERATE 2
typedef struct plade_icp_params {
    double source_leaf;          /* 0: 0.005 D */
    double max_dist;             /* 0: 0.025 D */
    double min_dist;             /* 0: 0.0025 D (capped at max_dist when max_dist is given and min_dist is not) */
    double eps_rotation;         /* radians, 0: 1e-6 */
    double eps_translation;      /* 0: 1e-6 D */
    int32_t max_iterations;      /* 0: 60 */
    int32_t min_correspondences; /* 0: 100 */
} plade_icp_params;
typedef struct plade_icp_result {
    int32_t iterations;          /* updates applied */
    int32_t stages;              /* stage distances used (1 + the index of the last) */
    int32_t converged;           /* 1: the stage at min_dist converged */
    int32_t failure;             /* 0, PLADE_ICP_TOO_FEW or PLADE_ICP_DEGENERATE */
    uint32_t correspondences;    /* of the last linearisation */
    uint32_t samples;            /* |S| */
    double rmse, fitness;        /* of the last linearisation */
    double final_dist;           /* the stage distance d of the last linearisation */
} plade_icp_result;
/* The defaults: 0 for the scale-dependent values (automatic), eps_rotation = 1e-6, max_iterations = 60, min_correspondences = 100. */
void plade_icp_default_params(plade_icp_params *p);
/* params NULL: the defaults.  T_out16 may be T_in16. */
int plade_refine_icp(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm, uint32_t n_s,
                     const float *T_in16, const plade_icp_params *params, float *T_out16, plade_icp_result *result);
/* The same on resident clouds (plade_cloud_upload, plade_cloud_upload_xyz): bit-identical results. */
int plade_refine_icp_dev(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, const float *T_in16, const plade_icp_params *params,
                         float *T_out16, plade_icp_result *result);
/* Test seam: one match + linearise pass at stage distance `dist` on the given points (no sample), with J taken about the fp64
 * point center[3] (the refinement uses c_k = T_k s-bar): corr_out[i] = j or -1 (n_s int32, may be NULL); moments_out = J^T J
 * (21 values, row-major upper triangle), J^T r (6), sum r^2, count. */
int plade_icp_linearize(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_xyz, uint32_t n_s, uint32_t stride,
                        const double *T16, const double *center, float dist, int32_t *corr_out, double *moments_out);

/* ---- fine alignment: plane-to-plane (generalized) ICP (no reference counterpart) ------------------------------------------------
 * Semantics (plade_amd/csrc/gicp.h).  Segal's Generalized ICP with the covariances built from the normals,
 * C = I - (1 - epsilon) n n^T: every correspondence is weighted by M = (C_t + R C_s R^T)^-1.  Where the two normals agree the term
 * is point-to-plane with weight ~ 1 / (2 epsilon); where they disagree (a wall against the clutter in front of it, corners, the
 * other side of a thin wall) the weight falls to order 1; the two clouds play symmetric roles.  epsilon = 1 makes M = I / 2
 * exactly: point-to-point ICP.  Target: n_t points x y z nx ny nz; source: n_s points x y z nx ny nz (BOTH normals are read);
 * T_in, D, A, the automatic values, the stage distances, the tolerances with their fp32 floors and the limit of 16 stages are those
 * of plade_refine_icp above, word for word.
 *   sample       S = the source alone, voxel-fused under plade_merge_clouds' rules at leaf source_leaf [0.005 D]
 *                (plade_merge_clouds_dev of one cloud under the identity): fp64 mean position, normalised fp64 sum of the finite
 *                normals, ascending voxel order; every sample point carries a normal m or three NaNs.  Not the xyz-only sample
 *                of plade_refine_icp: the two are not expected to have the same bits
 *   centre       s-bar = the fp64 mean of S (summed once in a fixed order), c_k = T_k s-bar in fp64
 *   match        p' and j as plade_refine_icp.  s has a correspondence when the distance < (float)d * (float)d, n_j is finite
 *                with (n0 n0 + n1 n1) + n2 n2 > 0 in fp64, and m is finite with non-zero length in the same way.  No second choice
 *                is looked for when the nearest point fails the normal test
 *   linearise    fp64 per correspondence, p = T_k double(s): e = p - q_j, u = p - c_k, nh = n_j / |n_j|, ah = R m / |R m|,
 *                k = 1 - epsilon, Sigma = 2 I - k nh nh^T - k ah ah^T, M = adj(Sigma) / det Sigma in closed form,
 *                J = [-[u]x | I]; the 21 values of J^T M J (row-major upper triangle), the 6 of J^T M e, sum e^T M e, sum e . e and
 *                the count: 30 moments, every term in the written operation order of gicp.h, summed in the fixed order of
 *                plade_refine_icp (bit-identical from run to run).  The eigenvalues of Sigma lie in [2 epsilon, 2]
 *   solve, update, tolerances, schedule   those of plade_refine_icp on the 21 + 6 moments
 *   failure      PLADE_EFAIL and T_out = T_in with failure = PLADE_ICP_TOO_FEW or PLADE_ICP_DEGENERATE.  The isotropic part of M
 *                makes a single plane or a crease NON-degenerate here (an in-plane pull at relative weight epsilon is inherent
 *                to GICP); degenerate remains for the truly singular cases, e.g. a sample on one straight line through c_k
 *   output       T_out: fp32 of the fp64 iterate; rmse = sqrt(sum e . e / count) (point-to-point), cost = sum e^T M e / count,
 *                fitness = count / |S|, all of the last linearisation
 * Errors: PLADE_EINVAL with a message for every case of plade_refine_icp and for epsilon < 0, epsilon > 1 or not finite (and what
 * plade_merge_clouds refuses for the sample: PLADE_ELIMIT for more than 2^18 leaves along an axis); the context stays usable.
 * plade_stats_get then reports gicp_sample_s, gicp_grid_s, gicp_loop_s, gicp_iterations and gicp_stages. */
typedef struct plade_gicp_params {
    double source_leaf;          /* 0: 0.005 D */
    double max_dist;             /* 0: 0.025 D */
    double min_dist;             /* 0: 0.0025 D (capped at max_dist when max_dist is given and min_dist is not) */
    double eps_rotation;         /* radians, 0: 1e-6 */
    double eps_translation;      /* 0: 1e-6 D */
    int32_t max_iterations;      /* 0: 60 */
    int32_t min_correspondences; /* 0: 100 */
    double epsilon;              /* variance along the normal relative to 1 in the tangent plane; 0: 1e-3; valid: 0 < epsilon <= 1 */
} plade_gicp_params;
typedef struct plade_gicp_result {
    int32_t iterations;          /* updates applied */
    int32_t stages;              /* stage distances used (1 + the index of the last) */
    int32_t converged;           /* 1: the stage at min_dist converged */
    int32_t failure;             /* 0, PLADE_ICP_TOO_FEW or PLADE_ICP_DEGENERATE */
    uint32_t correspondences;    /* of the last linearisation */
    uint32_t samples;            /* |S| */
    double rmse, fitness;        /* of the last linearisation; rmse is point-to-point */
    double final_dist;           /* the stage distance d of the last linearisation */
    double cost;                 /* sum e^T M e / count of the last linearisation */
} plade_gicp_result;
/* The defaults of plade_icp_default_params and epsilon = 1e-3.  Pure: needs no GPU. */
void plade_gicp_default_params(plade_gicp_params *p);
/* params NULL: the defaults.  T_out16 may be T_in16. */
int plade_refine_gicp(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm, uint32_t n_s,
                      const float *T_in16, const plade_gicp_params *params, float *T_out16, plade_gicp_result *result);
/* The same on resident clouds (plade_cloud_upload, plade_cloud_upload_xyz): bit-identical results. */
int plade_refine_gicp_dev(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, const float *T_in16, const plade_gicp_params *params,
                          float *T_out16, plade_gicp_result *result);
/* Test seam: one match + linearise pass at stage distance `dist` on the given source rows (x y z nx ny nz, no sample), about the
 * fp64 point center[3]; epsilon as in the parameters (0: 1e-3).  corr_out[i] = j or -1 (n_s int32, may be NULL); moments_out =
 * J^T M J (21 values, row-major upper triangle), J^T M e (6), sum e^T M e, sum e . e, count. */
int plade_gicp_linearize(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm, uint32_t n_s,
                         const double *T16, const double *center, float dist, double epsilon, int32_t *corr_out, double *moments_out);

/* ---- cloud-to-cloud distances and registration quality (no reference counterpart) ------------------------------------------
 * Semantics (plade_amd/csrc/distances.h).  Target: n_t points x y z nx ny nz (the normals may be NaN, as
 * plade_ply_read_points gives for xyz-only files); source: n_s points x y z, `stride` floats apart; T16: the row-major 4 x 4
 * source -> target transform in fp32 (NULL: the identity); d = max_dist (fp32, finite, > 0).
 *   transform    p'_i = fp32(R) s_i + fp32(t), each row ((r0 x + r1 y) + r2 z) + t in fp32 (the ICP's match rule)
 *   nearest      j_i = the argmin over ALL target points of (fp32 FLANN L2 (p'_i, q_j), j): ties go to the smaller index
 *   corresp.     i has one when that distance < (float)d * (float)d; an exact set, independent of cell sizes, source order and
 *                launch shapes
 *   per point    each array may be NULL.  idx_out[i] = j_i or -1; d2_out[i] = the fp32 distance or +inf without a
 *                correspondence; plane_out[i] = fp32 of r_i = (n0 (p0 - q0) + n1 (p1 - q1)) + n2 (p2 - q2), p = double(T) double(s_i)
 *                in fp64 with the same row order, NaN without a correspondence or when n_j is not finite
 *   summary      n = n_s, count, fitness = count / n, rmse = sqrt(sum d2 / count), mean = sum sqrt(d2) / count, max = max sqrt(d2),
 *                plane_count = the correspondences with a finite n_j, plane_rmse = sqrt(sum r^2 / plane_count).  The sums are fp64
 *                over double(d2) and r, in a fixed order of the original index (no fp64 atomics): bit-identical from run to run,
 *                with or without per-point outputs, for host or resident clouds.  count = 0 (still PLADE_OK): rmse, mean and max
 *                are NaN and fitness is 0; plane_count = 0: plane_rmse is NaN.
 * Errors: PLADE_EINVAL for NULL clouds or summary, n = 0, non-finite coordinates or T, d <= 0 or not finite, stride < 3; the
 * context stays usable.  plade_stats_get then reports distances_grid_s, distances_sort_s, distances_search_s (lane and ring
 * passes), distances_lane_s, distances_ring_s, distances_summary_s (HIP events on the context's stream) and distances_ring_queries
 * (probes the first pass could not finish). */
typedef struct plade_distance_summary {
    uint64_t n, count, plane_count;
    double fitness, rmse, mean, max, plane_rmse;
} plade_distance_summary;
int plade_cloud_distances(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_xyz, uint32_t n_s,
                          uint32_t stride, const float *T16, float max_dist, int32_t *idx_out, float *d2_out,
                          float *plane_out, plade_distance_summary *summary);
/* The same on resident clouds (plade_cloud_upload / plade_cloud_upload_xyz; the source's x y z): bit-identical results. */
int plade_cloud_distances_dev(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, const float *T16, float max_dist,
                              int32_t *idx_out, float *d2_out, float *plane_out, plade_distance_summary *summary);

/* ---- outlier removal: the step a chain on a raw scan starts with (no reference counterpart; PCL, Open3D and CloudCompare ship
 * both filters) ---------------------------------------------------------------------------------------------------------------
 * Semantics (plade_amd/csrc/outliers.h).  Input: n points, rows of `stride` >= 3 floats, x y z first, all
 * coordinates finite.  d(i, j) = the fp32 FLANN L2 of (p_i, p_j), ((dx*dx + dy*dy) + dz*dz).
 *   statistical  k in [1, 64], alpha >= 0.  Neighbours of i: the k_eff = min(k, n - 1) points j != i with the smallest keys
 *                (d(i, j), j); i is left out by its index, so a duplicate of i is a neighbour at distance 0.  m_i = (the sum of
 *                sqrt(double(d(i, j))) in ascending key order) / k_eff in fp64 (n = 1: 0).  mu = sum m_i / n, sigma =
 *                sqrt(sum (m_i - mu)^2 / (n - 1)) in a second pass (n = 1: 0), both fp64 in a fixed order of the original index:
 *                the same bits on every run.  Point i is kept when m_i <= mu + alpha * sigma (fp64).
 *   radius       radius > 0, min_neighbours >= 1.  c_i = the number of j != i with d(i, j) < (float)radius * (float)radius;
 *                point i is kept when c_i >= min_neighbours.
 *   output       each array may be NULL.  keep_out: n bytes 0 / 1; kept_index_out: the kept original indices, ascending (room
 *                for n); rows_out: the kept rows in that order, every float copied bit for bit (room for n rows; may be `rows`
 *                itself); mean_dist_out: m_i (n doubles, statistical mode only); count_out: c_i (n uint32, radius mode only --
 *                without it a point's count may stop at min_neighbours); summary: n, kept, mu, sigma, threshold (NaN in radius
 *                mode).  The result depends on the point set and the parameters only.
 * Errors: PLADE_EINVAL for n = 0, stride < 3, a non-finite coordinate, k outside [1, 64], alpha negative or not finite, radius
 * <= 0 or not finite, min_neighbours < 1; the context stays usable.  A filter that keeps nothing is PLADE_OK with kept = 0.
 * plade_stats_get then reports outliers_grid_s, outliers_search_s, outliers_reduce_s (mu, sigma, flags), outliers_compact_s
 * (scan, kept list and row gather; HIP events on the context's stream), outliers_grid_builds, outliers_ring_queries (points the
 * 27-cell search could not finish) and outliers_kept. */
#define PLADE_OUTLIER_STATISTICAL 0
#define PLADE_OUTLIER_RADIUS 1
typedef struct plade_outlier_params {
    int32_t mode;                /* PLADE_OUTLIER_STATISTICAL or PLADE_OUTLIER_RADIUS */
    int32_t k;                   /* statistical: neighbours, 1..64 */
    double alpha;                /* statistical: the threshold is mu + alpha sigma */
    double radius;               /* radius mode: must be set (> 0) */
    int32_t min_neighbours;      /* radius mode: >= 1 */
    int32_t reserved;            /* 0 */
} plade_outlier_params;
typedef struct plade_outlier_summary {
    uint64_t n, kept;
    double mu, sigma, threshold; /* NaN in radius mode */
} plade_outlier_summary;
/* The defaults: statistical mode, k = 16, alpha = 1.0, radius = 0 (unset), min_neighbours = 1.  Needs no GPU. */
void plade_outlier_default_params(plade_outlier_params *p);
/* params NULL: the defaults. */
int plade_filter_outliers(plade_ctx *ctx, const float *rows, uint32_t n, uint32_t stride, const plade_outlier_params *params,
                          uint8_t *keep_out, uint32_t *kept_index_out, float *rows_out, double *mean_dist_out, uint32_t *count_out,
                          plade_outlier_summary *summary);
/* The same on a resident cloud (plade_cloud_upload / plade_cloud_upload_xyz; rows x y z nx ny nz) into a NEW resident cloud: the
 * point data makes no host round trip.  The same keep, kept_index and summary bits as plade_filter_outliers on the cloud's rows.
 * PLADE_EFAIL (summary filled, *out NULL) when nothing is kept: a resident cloud has no empty form.  Free both clouds with
 * plade_cloud_free. */
int plade_cloud_filter_outliers_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_outlier_params *params, plade_cloud **out,
                                    uint8_t *keep_out, uint32_t *kept_index_out, plade_outlier_summary *summary);

/* ---- connected components: dropping dense blobs that do not belong to the structure (no reference counterpart; PCL ships it as
 * EuclideanClusterExtraction, Open3D as cluster_dbscan) ----------------------------------------------------------------------------
 * Semantics (plade_amd/csrc/components.h).  Input: n >= 1 points, rows of `stride` >= 3 floats, x y z first,
 * all coordinates finite.  d(i, j) = the fp32 FLANN L2 of (p_i, p_j), ((dx*dx + dy*dy) + dz*dz).
 *   edge         i ~ j when i != j and d(i, j) < (float)radius * (float)radius (the strict `<` of the radius filter): duplicates are
 *                connected, a pair at exactly radius^2 is not.
 *   components   the connected components of that graph, an exact set; ids 0 .. C - 1 in ascending order of the component's smallest
 *                original index.
 *   selection    component c passes when min_size <= size[c] and (max_size = 0 or size[c] <= max_size).  keep_largest = m > 0: only
 *                the m passing components that come first in the order (size descending, id ascending) are kept; 0: all passing
 *                ones.  A point is kept when its component is.
 *   output       each array may be NULL.  label_out: n int32, the id of each point's component; size_out: the C sizes (room for
 *                n); keep_out: n bytes 0 / 1; kept_index_out: the kept original indices, ascending (room for n); rows_out: the kept
 *                rows in that order, every float copied bit for bit (room for n rows; may be `rows` itself); summary: n,
 *                components = C, kept_components, kept, largest = the largest size.  The result depends on the point set and the
 *                parameters only, and is the same bits on every run.
 * Errors: PLADE_EINVAL for n = 0, stride < 3, a NULL cloud, a non-finite coordinate, radius <= 0 or not finite (or its fp32 square
 * not finite), min_size < 1, max_size in (0, min_size), keep_largest < 0; the context stays usable.  A
 * selection that keeps nothing is PLADE_OK with kept = 0.  A radius that is tiny against the cloud's extent (one far point is
 * enough) is not refused: the grid's cell grows until 48e6 cells hold the cloud, and every call then fills a row table of up to
 * 192 MB -- crop such a cloud first.  plade_stats_get then reports components_grid_s,
 * components_link_s (the union-find over the edges), components_label_s (roots, ids, sizes, selection), components_compact_s (scan,
 * kept list and row gather; HIP events on the context's stream), components_count and components_kept. */
typedef struct plade_component_params {
    double radius;               /* must be set (> 0): there is no automatic value */
    int32_t min_size;            /* >= 1 */
    int32_t max_size;            /* 0: no upper bound, else >= min_size */
    int32_t keep_largest;        /* 0: every passing component, m > 0: the m largest passing ones */
    int32_t reserved;            /* 0 */
} plade_component_params;
typedef struct plade_component_summary {
    uint64_t n, components, kept_components, kept;
    uint32_t largest;
    uint32_t reserved;           /* 0 */
} plade_component_summary;
/* The defaults: radius = 0 (unset), min_size = 1, max_size = 0, keep_largest = 0.  Needs no GPU. */
void plade_component_default_params(plade_component_params *p);
int plade_label_components(plade_ctx *ctx, const float *rows, uint32_t n, uint32_t stride, const plade_component_params *params,
                           int32_t *label_out, uint32_t *size_out, uint8_t *keep_out, uint32_t *kept_index_out, float *rows_out,
                           plade_component_summary *summary);
/* The same on a resident cloud (plade_cloud_upload / plade_cloud_upload_xyz; rows x y z nx ny nz) into a NEW resident cloud of the
 * kept points, a resident cloud like any other: the point data makes no host round trip.  The same label, kept_index and summary
 * bits as plade_label_components on the cloud's rows.  PLADE_EFAIL (summary filled, *out NULL) when nothing is kept: a resident
 * cloud has no empty form.  Free both clouds with plade_cloud_free. */
int plade_cloud_filter_components_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_component_params *params, plade_cloud **out,
                                      int32_t *label_out, uint32_t *kept_index_out, plade_component_summary *summary);

/* ---- DBSCAN: clustering by density, where one thin thread of stray points must not join two objects and isolated points must stay
 * noise (no reference counterpart; Open3D ships it as cluster_dbscan, scikit-learn as DBSCAN) ---------------------------------------
 * Semantics (plade_amd/csrc/dbscan.h).  Input: n >= 1 points, rows of `stride` >= 3 floats, x y z first, all
 * coordinates finite.  d(i, j) = the fp32 FLANN L2 of (p_i, p_j), ((dx*dx + dy*dy) + dz*dz); r2 = (float)radius * (float)radius.
 *   count        count(i) = |{ j : d(i, j) < r2 }| (strict `<`), the point itself included (Open3D's and scikit-learn's convention);
 *                i is a core point iff count(i) >= min_points.
 *   clusters     the connected components of the graph on the core points alone (i ~ j iff both are core and d(i, j) < r2), an
 *                exact set; ids 0 .. C - 1 in ascending order of the cluster's smallest core index.
 *   border       a non-core point with at least one core point closer than radius; it takes the label of the core neighbour j with
 *                the smallest pair (d(i, j), j).  (Textbook DBSCAN leaves that to the visiting order.)  A border point never
 *                connects two clusters.
 *   noise        everything else: label -1.
 *   selection    on the sizes (core and border members) exactly as plade_label_components selects: min_size, max_size,
 *                keep_largest; noise is never kept.
 *   output       each array may be NULL.  label_out: n int32; kind_out: n bytes, 0 noise / 1 border / 2 core; size_out: the C sizes
 *                (room for n); keep_out: n bytes 0 / 1; kept_index_out: the kept original indices, ascending (room for n);
 *                rows_out: the kept rows in that order, every float copied bit for bit (room for n rows; may be `rows` itself);
 *                summary: n, clusters = C, core, border, noise, kept_clusters, kept, largest = the largest size.  The result
 *                depends on the point set and the parameters only, and is the same bits on every run.  With min_points = 1 every
 *                point is core, and label, size, keep, kept_index and the rows are those of plade_label_components bit for bit.
 * Errors: PLADE_EINVAL for n = 0, stride < 3, a NULL cloud, a non-finite coordinate, radius <= 0 or not finite (or its fp32 square
 * not finite or below FLT_MIN: a point must be its own neighbour), min_points < 1, min_size < 1, max_size in (0, min_size),
 * keep_largest < 0; the outputs are untouched and the context stays usable.  All noise, or a selection that keeps nothing, is
 * PLADE_OK with kept = 0.  The grid is the components': a radius that is tiny against the cloud's extent is not refused (see there).
 * plade_stats_get then reports dbscan_grid_s, dbscan_core_s (the counting walk), dbscan_link_s (the union-find over the core-core
 * edges and the border rule), dbscan_label_s (roots, ids, sizes, selection), dbscan_compact_s (scan, kept list and row gather; HIP
 * events on the context's stream), dbscan_clusters and dbscan_kept. */
typedef struct plade_dbscan_params {
    double radius;               /* must be set (> 0): there is no automatic value */
    int32_t min_points;          /* >= 1: the neighbours (itself included) that make a point a core point; 4 */
    int32_t min_size;            /* >= 1 */
    int32_t max_size;            /* 0: no upper bound, else >= min_size */
    int32_t keep_largest;        /* 0: every passing cluster, m > 0: the m largest passing ones */
} plade_dbscan_params;
typedef struct plade_dbscan_summary {
    uint64_t n, clusters, core, border, noise, kept_clusters, kept;
    uint32_t largest;
    uint32_t reserved;           /* 0 */
} plade_dbscan_summary;
/* The defaults: radius = 0 (unset), min_points = 4, min_size = 1, max_size = 0, keep_largest = 0.  Needs no GPU. */
void plade_dbscan_default_params(plade_dbscan_params *p);
int plade_cluster_dbscan(plade_ctx *ctx, const float *rows, uint32_t n, uint32_t stride, const plade_dbscan_params *params,
                         int32_t *label_out, uint8_t *kind_out, uint32_t *size_out, uint8_t *keep_out, uint32_t *kept_index_out,
                         float *rows_out, plade_dbscan_summary *summary);
/* The same on a resident cloud (rows x y z nx ny nz) into a NEW resident cloud of the kept points: the point data makes no host round
 * trip.  The same label, kind, kept_index and summary bits as plade_cluster_dbscan on the cloud's rows.  PLADE_EFAIL (summary
 * filled, *out NULL) when nothing is kept: a resident cloud has no empty form.  Free both clouds with plade_cloud_free. */
int plade_cloud_cluster_dbscan_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_dbscan_params *params, plade_cloud **out,
                                   int32_t *label_out, uint8_t *kind_out, uint32_t *kept_index_out, plade_dbscan_summary *summary);

/* ---- subsampling to a minimum point spacing: a subset of the cloud's OWN points (no reference counterpart; CloudCompare ships it
 * as "Subsample -> Space" and takes M3C2's core points from it) ------------------------------------------------------------------
 * Semantics (plade_amd/csrc/subsample.h).  Input: n >= 1 points, rows of `stride` >= 3 floats, x y z first,
 * all coordinates finite.  d(i, j) = the fp32 FLANN L2 of (p_i, p_j), ((dx*dx + dy*dy) + dz*dz); r2 = (float)spacing * (float)spacing.
 *   priority     point i has the key (mix64(mix64(seed) ^ i), i), mix64 = the splitmix64 finaliser (z += 0x9E3779B97F4A7C15;
 *                z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31); keys compare
 *                lexicographically, no two are equal.
 *   kept set     walk the points in ascending key order: a point is kept if and only if no already-kept point j has d(i, j) < r2
 *                (the strict `<` of the radius filter: of duplicates exactly one is kept, a pair at exactly d = r2 keeps both).  No
 *                two kept points are closer than spacing, every dropped point has a kept point closer than spacing, and the set --
 *                the lexicographically first maximal independent set of the graph "closer than spacing" -- is unique.
 *   rounds       the same set as the fixed point of synchronous rounds: in round t every undecided point looks at its neighbours
 *                with d < r2 and a smaller key as they stood at the end of round t - 1; one of them kept: dropped; otherwise none
 *                of them undecided: kept; otherwise it waits.  round[i] = the round that decided i, rounds = the largest.
 *   output       each array may be NULL.  keep_out: n bytes 0 / 1; kept_index_out: the kept original indices, ascending (room for
 *                n); rows_out: the kept rows in that order, every float copied bit for bit (room for n rows; may be `rows` itself);
 *                round_out: n uint32; summary: n, kept, rounds.  The result depends on the points, spacing and seed only, and is
 *                the same bits on every run.
 * Errors: PLADE_EINVAL for n = 0 (or n >= 2^31), stride < 3, a NULL cloud, a non-finite coordinate, a spacing that is not finite and > 0 or whose
 * fp32 square is not finite or below FLT_MIN; the context stays usable.  At least one point is always kept.  A spacing that is tiny
 * against the cloud's extent is not refused: the grid's cell grows until 48e6 cells hold the cloud (the result is the same).
 * plade_stats_get then reports subsample_grid_s, subsample_rounds_s, subsample_compact_s (scatter to the original order, scan, kept
 * list and row gather; HIP events on the context's stream), subsample_rounds, subsample_kept and subsample_grid_dx / _dy / _dz /
 * _cell. */
typedef struct plade_subsample_params {
    double spacing;              /* must be set (> 0): there is no automatic value */
    uint64_t seed;               /* of the priority keys */
} plade_subsample_params;
typedef struct plade_subsample_summary {
    uint32_t n, kept, rounds;
} plade_subsample_summary;
/* The defaults: spacing = 0 (unset), seed = 0.  Needs no GPU. */
void plade_subsample_default_params(plade_subsample_params *p);
int plade_subsample_spacing(plade_ctx *ctx, const float *rows, uint32_t n, uint32_t stride, const plade_subsample_params *params,
                            uint8_t *keep_out, uint32_t *kept_index_out, float *rows_out, uint32_t *round_out,
                            plade_subsample_summary *summary);
/* The same on a resident cloud (plade_cloud_upload / plade_cloud_upload_xyz; rows x y z nx ny nz) into a NEW resident cloud of the
 * kept points, a resident cloud like any other: the point data makes no host round trip.  The same keep, kept_index and summary
 * bits as plade_subsample_spacing on the cloud's rows.  Free both clouds with plade_cloud_free. */
int plade_cloud_subsample_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_subsample_params *params, plade_cloud **out,
                              uint8_t *keep_out, uint32_t *kept_index_out, plade_subsample_summary *summary);

/* ---- consistent normal orientation: one side of the surface everywhere, without a viewpoint per point (no reference counterpart;
 * Open3D ships it as orient_normals_consistent_tangent_plane, CloudCompare as its MST orientation; Hoppe et al. 1992) ---------------
 * Semantics (plade_amd/csrc/orient.h).  Input: n >= 1 rows x y z nx ny nz, n < 2^31, all coordinates finite.
 * d(i, j) = the fp32 FLANN L2 of (p_i, p_j), ((dx*dx + dy*dy) + dz*dz); r2 = (float)radius * (float)radius.
 *   valid point  its three normal components are finite and each |component| <= 1e18f.  Every other point is left bit for bit as it
 *                is, gets flip = 0 and label = -1 and is counted in `unoriented`.
 *   graph        the vertices are the valid points; i ~ j when i != j and d(i, j) < r2 (the strict `<` of the radius filter).
 *   edge weight  dot32 = (nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j in fp32 without contraction; key32 = 0x7F800000u - bits(fabsf(dot32)):
 *                the smaller key is the flatter pair.  Edges are ordered by (key32, min(i,j), max(i,j)); no two are equal.
 *   tree, flips  the minimum spanning forest under that order (unique).  s_ij = 1 when dot32 < 0.0f, else 0; along every forest edge
 *                flip_i ^ flip_j = s_ij.  That fixes a component's flips up to one bit, which its anchor fixes:
 *   mode PLADE_ORIENT_VOTE     anchored provisionally at flip = 0 on the component's valid point of smallest index, the flip test of
 *                plade_estimate_normals, t_i = ((vx - px) * nx + (vy - py) * ny) + (vz - pz) * nz in fp64 (v = viewpoint), is taken
 *                on every provisionally flipped normal; when strictly more points have t_i < 0 than t_i > 0 the whole component is
 *                toggled.  A tie toggles nothing.
 *   mode PLADE_ORIENT_EXTREME  e_i = ((double)x*dx + (double)y*dy) + (double)z*dz (d = direction); the anchor is the component's valid
 *                point with the largest (e_i, then the smaller index); it is flipped when the same form g on its normal is < 0.
 *   inward = 1   inverts the decision of either mode (a room scanned from the inside: EXTREME with inward = 1).
 *   output       each array may be NULL.  rows_out: the n rows, a flipped point's three normal floats with their sign bit toggled,
 *                every other float copied bit for bit (may be pos_nrm itself); flip_out: n bytes 0 / 1; label_out: n int32, the
 *                component of the graph, ids ascending in the order of each component's smallest index, -1 for invalid points;
 *                summary: n, unoriented, components, flipped, tree_edges (= valid points - components), rounds (of the GPU's
 *                Boruvka iteration, at most ceil(log2 n) + 1; the only field that is not part of the definition) and tree_key_sum
 *                (the sum of key32 over the forest's edges).  The result depends on the rows and the parameters only, and is the
 *                same bits on every run.
 * Two parallel sheets of opposite orientation that are closer than `radius` get the same side: inherent to the method; keep
 * `radius` below the thinnest wall.
 * Errors: PLADE_EINVAL for n = 0 (or n >= 2^31), a NULL cloud, a non-finite coordinate, a radius that is not finite and > 0 or whose
 * fp32 square is not finite or below FLT_MIN, a non-finite viewpoint or direction, direction = 0, a mode other than 0 or 1, inward
 * not 0 or 1; the context stays usable.  A cloud without any valid point is PLADE_OK with everything copied.  A radius that is tiny
 * against the cloud's extent is not refused: the grid's cell grows until 48e6 cells hold the cloud (the result is the same).
 * plade_stats_get then reports orient_grid_s, orient_rounds_s (every launch of the rounds with the read-backs between them),
 * orient_finish_s (anchors, ids, scatter to the original order; HIP events on the context's stream), orient_rounds,
 * orient_components, orient_flipped and orient_grid_dx / _dy / _dz / _cell. */
#define PLADE_ORIENT_VOTE 0
#define PLADE_ORIENT_EXTREME 1
typedef struct plade_orient_params {
    double radius;               /* must be set (> 0), absolute, in the cloud's units: there is no automatic value */
    int32_t mode;                /* PLADE_ORIENT_VOTE (default) or PLADE_ORIENT_EXTREME */
    int32_t inward;              /* 0 (default) or 1 */
    float viewpoint[3];          /* of PLADE_ORIENT_VOTE; default the origin */
    float direction[3];          /* of PLADE_ORIENT_EXTREME; default (0, 0, 1); not zero */
} plade_orient_params;
typedef struct plade_orient_summary {
    uint32_t n, unoriented, components, flipped, tree_edges, rounds;
    uint64_t tree_key_sum;
} plade_orient_summary;
/* The defaults: radius = 0 (unset), mode = PLADE_ORIENT_VOTE, inward = 0, viewpoint (0, 0, 0), direction (0, 0, 1).  Needs no GPU. */
void plade_orient_default_params(plade_orient_params *p);
int plade_orient_normals(plade_ctx *ctx, const float *pos_nrm, uint32_t n, const plade_orient_params *params, float *rows_out,
                         uint8_t *flip_out, int32_t *label_out, plade_orient_summary *summary);
/* The same on a resident cloud (plade_cloud_upload / plade_cloud_upload_xyz) into a NEW resident cloud of the same n points, a
 * resident cloud like any other: the point data makes no host round trip.  The same rows, flip, label and summary bits as
 * plade_orient_normals on the cloud's rows.  Free both clouds with plade_cloud_free. */
int plade_cloud_orient_normals_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_orient_params *params, plade_cloud **out,
                                   uint8_t *flip_out, int32_t *label_out, plade_orient_summary *summary);

/* ---- smoothing: moving-least-squares plane projection, the step between outlier removal and normals (no reference counterpart;
 * PCL ships it as MovingLeastSquares, Open3D users expect it) -----------------------------------------------------------------------
 * Semantics (plade_amd/csrc/smooth.h).  Input: n >= 1 points, rows of `stride` >= 3 floats, x y z first, all
 * coordinates finite.  r2 = (float)radius * (float)radius; d(i, j) = the fp32 FLANN L2 of (p_i, p_j), ((dx*dx + dy*dy) + dz*dz).
 *   neighbours   N_i = the j with d(i, j) < r2 (strict, as the radius filter); the point itself is one of them.  c_i = |N_i|.
 *   moments      u = (double)d / (double)r2, w = (1 - u) * (1 - u); q_j = double(p_j) - double(p_i); W = sum w, S = sum w q,
 *                M = sum (w q_a) q_b (xx xy xz yy yz zz), fp64, added in the order of the grid walk (no atomics).
 *                mu = S / W, C = M / W - mu mu^T.
 *   fit          n = the unit eigenvector of C's smallest eigenvalue l0 (the closed-form fp64 solve of plade_estimate_normals),
 *                flipped when (viewpoint - p_i) . n < 0; curvature = max(l0, 0) / trace.
 *   projection   delta_i = n . mu (fp64), the signed distance from p_i to the fitted plane along n;
 *                p_i' = fp32(double(p_i) + delta_i * n) per coordinate.
 *   unfitted     c_i < min_neighbours or C exactly zero: the position is copied bit for bit, normal and curvature are NaN,
 *                delta = 0, fitted = 0.
 *   output       by original index; every array after out_xyz may be NULL.  out_xyz: n x 3 floats; out_normal: n x 3 floats;
 *                curvature_out: n floats; displacement_out: n doubles (delta); count_out: n uint32 (c_i); fitted_out: n bytes
 *                0 / 1; moments_out: n x 10 doubles W, S (3), M (6) -- a test seam; summary: n, fitted, the rms and the max of
 *                |delta| over the fitted points (0 when there is none; a fixed-order fp64 reduction) and the largest c_i.
 * The same input gives the same bits on every run, on every context and from plade_cloud_smooth_dev.  c_i and fitted depend on the
 * point set and the radius only; the fp64 sums follow the grid's order: under a permutation of the input their last bits may
 * differ.
 * Errors: PLADE_EINVAL for n = 0, stride < 3, a NULL cloud or out_xyz, a non-finite coordinate or viewpoint, radius <= 0 or not
 * finite (or its fp32 square r2 not finite or below FLT_MIN: the point itself must satisfy 0 < r2), min_neighbours < 3; the context stays usable.  plade_stats_get then reports
 * smooth_grid_s, smooth_fit_s, smooth_reduce_s (HIP events on the context's stream) and smooth_fitted. */
typedef struct plade_smooth_params {
    double radius;               /* must be set (> 0), absolute, in the cloud's units: there is no automatic value */
    int32_t min_neighbours;      /* >= 3; a point with fewer neighbours (itself included) is left where it is */
    float viewpoint[3];          /* the fit's normals point toward it */
    int32_t reserved;            /* 0 */
} plade_smooth_params;
typedef struct plade_smooth_summary {
    uint64_t n, fitted;
    double rms, max;             /* of |delta| over the fitted points */
    uint32_t max_count;          /* the largest c_i */
    uint32_t reserved;           /* 0 */
} plade_smooth_summary;
/* The defaults: radius = 0 (unset), min_neighbours = 6, viewpoint = 0 0 0.  Needs no GPU. */
void plade_smooth_default_params(plade_smooth_params *p);
int plade_smooth_cloud(plade_ctx *ctx, const float *rows, uint32_t n, uint32_t stride, const plade_smooth_params *params,
                       float *out_xyz, float *out_normal, float *curvature_out, double *displacement_out, uint32_t *count_out,
                       uint8_t *fitted_out, double *moments_out, plade_smooth_summary *summary);
/* The same on a resident cloud (plade_cloud_upload / plade_cloud_upload_xyz; rows x y z nx ny nz) into a NEW resident cloud of the
 * same n points with the smoothed positions: the point data makes no host round trip, the positions and the summary are the bits
 * of plade_smooth_cloud on the cloud's rows.  use_fit_normals = 1: columns 3..5 are the fit's normals (NaN where unfitted, which the
 * registration skips like the NaN normals of plade_estimate_normals); 0: the input cloud's normal columns bit for bit.  Free both
 * clouds with plade_cloud_free. */
int plade_cloud_smooth_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_smooth_params *params, int32_t use_fit_normals,
                           plade_cloud **out, plade_smooth_summary *summary);

/* ---- multi-scale normals and dimensionality features: the normal-scale step of M3C2 (Lague, Brodu, Leroux 2013; no reference
 * counterpart) ------------------------------------------------------------------------------------------------------------------------
 * Semantics (plade_amd/csrc/scales.h).  Input: n >= 1 points, rows of `stride` >= 3 floats, x y z first, all
 * coordinates finite.  The queries are all n points (query_index NULL; k is ignored) or query_index: k >= 1 strictly ascending indices
 * < n, e.g. the kept_index of plade_subsample_spacing; every output is by query, in the order of that list.  params->scales = S radii,
 * 1 <= S <= 8, whose fp32 squares r2_s = (float)r_s * (float)r_s are strictly ascending.  One grid and one walk serve all scales.
 *   neighbours   N(i, s) = the j with d(i, j) < r2_s (the fp32 squared distance and the strict `<` of plade_smooth_cloud); the point
 *                itself is one of them.  c(i, s) = |N(i, s)|.
 *   moments      unweighted, fp64, q_j = double(p_j) - double(p_i): per scale the sums of q (3) and of q_a q_b (xx xy xz yy yz zz).
 *                Each scale adds the terms of the neighbours that pass its own test, in the order of the walk over the grid of the
 *                largest radius (no atomics): a scale's moments do not depend on which smaller scales were asked for.
 *   fit          mu = sum q / c, C = M / c - mu mu^T; l1 >= l2 >= l3 = the eigenvalues of C by the closed form, each clamped to
 *                >= 0; n = the unit eigenvector of the smallest one (the solve of plade_estimate_normals).  A scale is fitted iff
 *                c >= min_neighbours, C is not exactly zero and l1 > 0; the normal of an unfitted scale is NaN.
 *   features     fp64: linearity (l1 - l2) / l1, planarity (l2 - l3) / l1, sphericity l3 / l1, variation l3 / ((l1 + l2) + l3).
 *   choice       over the fitted scales in ascending s: mode 0 keeps the largest planarity (M3C2's rule), mode 1 the smallest
 *                variation; only a strict improvement replaces a scale (ties keep the smaller radius); -1: no scale is fitted.
 *   orientation  of every scale's normal.  orient = 0: flipped when (viewpoint - p_i) . n < 0.  orient = 1 (stride >= 6): words
 *                3..5 of the row are a normal g; t = (g_x n_x + g_y n_y) + g_z n_z in fp64; flipped when t < 0; when t is 0 or not
 *                finite the viewpoint test decides.
 *   output       every array may be NULL.  chosen_out: k int32; normal_out: k x 3 floats, the chosen scale's (NaN when -1);
 *                features_out: k x 4 floats in the order above, the chosen scale's (NaN when -1); per scale count_out: k x S uint32;
 *                fitted_out: k x S bytes 0 / 1; eigenvalues_out: k x S x 3 doubles l1 l2 l3; normals_out: k x S x 3 floats;
 *                moments_out: k x S x 9 doubles -- a test seam; summary: queries, fitted (chosen >= 0), the histogram of the chosen
 *                scale and the largest count (integers, a fixed-order reduction).
 * The same input gives the same bits on every run, on every context and from plade_cloud_scale_normals_dev.  Counts, fitted flags
 * and -- away from ties -- chosen depend on the point set and the radii only; the fp64 sums follow the grid's order.
 * Errors: PLADE_EINVAL for n = 0, stride < 3 (< 6 with orient = 1), a NULL cloud, a non-finite coordinate or viewpoint, scales outside
 * 1..8, a radius <= 0 or not finite (or its fp32 square not finite or below FLT_MIN), squares not strictly ascending, min_neighbours
 * < 3, mode or orient not 0 / 1, k = 0 with a list, a query index >= n or a list not strictly ascending; the context stays usable.
 * plade_stats_get then reports scales_grid_s, scales_walk_s (the walk and the fits), scales_reduce_s (HIP events on the context's
 * stream) and scales_fitted. */
typedef struct plade_scale_params {
    double radii[8];             /* the first `scales` must be set (> 0), absolute, in the cloud's units */
    int32_t scales;              /* S, 1 .. 8: there is no automatic value */
    int32_t min_neighbours;      /* >= 3; a scale with fewer neighbours (the point itself included) is not fitted */
    int32_t mode;                /* 0: the largest planarity; 1: the smallest surface variation */
    int32_t orient;              /* 0: toward the viewpoint; 1: along the rows' own normals, the viewpoint where they do not decide */
    float viewpoint[3];
    int32_t reserved;            /* 0 */
} plade_scale_params;
typedef struct plade_scale_summary {
    uint64_t queries, fitted;    /* fitted: queries with chosen >= 0 */
    uint32_t chosen_hist[8];     /* queries per chosen scale */
    uint32_t max_count;          /* the largest c(i, s) */
    uint32_t reserved;           /* 0 */
} plade_scale_summary;
/* The defaults: radii 0 and scales = 0 (unset), min_neighbours = 6, mode = 0, orient = 0, viewpoint = 0 0 0.  Needs no GPU. */
void plade_scale_default_params(plade_scale_params *p);
int plade_cloud_scale_features(plade_ctx *ctx, const float *rows, uint32_t n, uint32_t stride, const uint32_t *query_index, uint32_t k,
                               const plade_scale_params *params, int32_t *chosen_out, float *normal_out, float *features_out,
                               uint32_t *count_out, uint8_t *fitted_out, double *eigenvalues_out, float *normals_out,
                               double *moments_out, plade_scale_summary *summary);
/* The same on a resident cloud (plade_cloud_upload / plade_cloud_upload_xyz; rows x y z nx ny nz, so orient = 1 reads the cloud's
 * normals) into a NEW resident cloud of the k queries: x y z bit for bit, columns 3..5 the chosen normal (NaN where no scale is
 * fitted, which plade_cloud_m3c2_dev reports as "no axis").  The rows and the summary are the bits of plade_cloud_scale_features on
 * the cloud's rows.  *out is NULL after every refusal.  Free both clouds with plade_cloud_free. */
int plade_cloud_scale_normals_dev(plade_ctx *ctx, plade_cloud *cloud, const uint32_t *query_index, uint32_t k,
                                  const plade_scale_params *params, plade_cloud **out, plade_scale_summary *summary);

/* ---- change detection between two registered clouds: M3C2 distances (Lague, Brodu, Leroux 2013; no reference counterpart) -------
 * Semantics (plade_amd/csrc/m3c2.h).  Per core point a cylinder of radius R and half-length L along the core
 * point's normal; the mean position of each cloud inside it, measured along the normal; the difference of the two means and its
 * 95 % level of detection.  Input: m >= 1 core points, rows x y z nx ny nz with finite coordinates (the normals need not be unit
 * and may be non-finite); the reference cloud A and the compared cloud B: n >= 1 points each, rows of `stride` >= 3 floats, x y z
 * first, finite; T16: row-major fp32 4 x 4, B -> the frame of A and the core points (NULL: the identity, which goes through the
 * same arithmetic).
 *   transform    B' = ((r0 x + r1 y) + r2 z) + t per row in fp32 (the rule of plade_cloud_distances).
 *   axis         len2 = (nx nx + ny ny) + nz nz in fp64, n^ = double(n) / sqrt(len2).  A core point whose len2 is not finite or is 0
 *                has no axis: both counts 0, the moments 0, distance, lod and sigma NaN, significant 0.  Not an error.
 *   membership   in fp64 from the fp32 inputs, without contraction: q = double(p) - double(c); t = (q_x n^_x + q_y n^_y) + q_z n^_z;
 *                e = q - t n^ per coordinate; rho2 = (e_x e_x + e_y e_y) + e_z e_z.  p is in the cylinder iff
 *                fabs(t) <= L && rho2 < R * R: the radius test is strict, the ends are closed.
 *   moments      per core point and cloud X in {A, B}: the exact count c_X, S1_X = sum t, S2_X = sum t t: fp64 sums in the fixed
 *                order of the grid walk.  No atomics.
 *   result       a core point is valid iff it has an axis and c_A, c_B >= min_points.  Then mean_X = S1_X / c_X,
 *                var_X = max(S2_X - S1_X mean_X, 0) / (c_X - 1), sigma_X = sqrt(var_X), distance = mean_B - mean_A,
 *                lod = 1.96 (sqrt(var_A / c_A + var_B / c_B) + reg_error), significant = |distance| > lod.  Not valid: distance,
 *                lod and sigma are NaN and significant is 0; the counts and moments are still reported when there is an axis.
 *   output       by core index; each array may be NULL.  distance_out, lod_out: m doubles; significant_out: m bytes 0 / 1;
 *                count_out: m x 2 uint32 (c_A, c_B); sigma_out: m x 2 doubles; moments_out: m x 4 doubles S1_A S2_A S1_B S2_B -- a
 *                test seam.  summary: m, valid, significant, the mean of distance, the rms of distance and the max of |distance|
 *                over the valid core points (NaN when there is none; a fixed-order fp64 reduction over the core index) and the
 *                largest count of either cloud.
 * The same input gives the same bits on every run, on every context and from plade_cloud_m3c2_dev.  The counts depend on the point
 * sets, the axes, R and L only; the last bits of the sums follow the grid (another bounding box, a permutation of the input).
 * Errors: PLADE_EINVAL for a NULL cloud, params or summary, m = 0 or n = 0, stride < 3, a non-finite coordinate or T, radius or
 * depth <= 0 or not finite (or radius * radius not finite), reg_error < 0 or not finite, min_points < 2; the context stays usable.
 * plade_stats_get then reports m3c2_grid_s (transform + both grids), m3c2_walk_s, m3c2_reduce_s (HIP events on the context's
 * stream) and m3c2_valid. */
typedef struct plade_m3c2_params {
    double radius;               /* R: must be set (> 0), absolute, in the clouds' units */
    double depth;                /* L, the cylinder's half-length: must be set (> 0) */
    double reg_error;            /* >= 0: the registration error added to the level of detection (e.g. plade_distance_summary.rmse) */
    int32_t min_points;          /* >= 2: the smallest count per cloud of a valid core point */
    int32_t reserved;            /* 0 */
} plade_m3c2_params;
typedef struct plade_m3c2_summary {
    uint64_t m, valid, significant;
    double mean, rms, max;       /* of distance, of distance, of |distance| over the valid core points */
    uint32_t max_count;          /* the largest c_A or c_B */
    uint32_t reserved;           /* 0 */
} plade_m3c2_summary;
/* The defaults: radius = depth = 0 (unset), reg_error = 0, min_points = 4.  Needs no GPU. */
void plade_m3c2_default_params(plade_m3c2_params *p);
int plade_cloud_m3c2(plade_ctx *ctx, const float *core_pos_nrm, uint32_t m, const float *ref_rows, uint32_t n_a, uint32_t stride_a,
                     const float *cmp_rows, uint32_t n_b, uint32_t stride_b, const float *T16, const plade_m3c2_params *params,
                     double *distance_out, double *lod_out, uint8_t *significant_out, uint32_t *count_out, double *sigma_out,
                     double *moments_out, plade_m3c2_summary *summary);
/* The same on resident clouds (rows x y z nx ny nz; `core` supplies the core points and their normals and may be the same handle
 * as `ref`): the point data makes no host round trip, the outputs (host arrays) are the bits of plade_cloud_m3c2 on the clouds'
 * rows. */
int plade_cloud_m3c2_dev(plade_ctx *ctx, plade_cloud *core, plade_cloud *ref, plade_cloud *cmp, const float *T16,
                         const plade_m3c2_params *params, double *distance_out, double *lod_out, uint8_t *significant_out,
                         uint32_t *count_out, double *sigma_out, double *moments_out, plade_m3c2_summary *summary);

/* ---- point descriptors and their match between two clouds: FPFH (Rusu, Blodow, Beetz 2009; no reference counterpart) -------------
 * Semantics (plade_amd/csrc/fpfh.h).  Input: n >= 1 rows x y z nx ny nz in fp32 with finite coordinates (the
 * normals need not be unit and may be non-finite).
 *   neighbours   d(i, j) = the fp32 squared distance of plade_smooth_cloud; N_i = { j : 0 < d(i, j) < r2 }, r2 = (float)r * (float)r:
 *                strict on both sides, so coincident points -- i itself included -- are no neighbours.
 *   axis         len2 = (nx nx + ny ny) + nz nz in fp64, n^ = double(n) / sqrt(len2).  A point whose len2 is 0 or not finite has no
 *                axis: it has no descriptor and is nobody's neighbour.  Not an error.
 *   pair (i, j)  for j in N_i, both with an axis, in fp64 without contraction, every dot product (a_x b_x + a_y b_y) + a_z b_z:
 *                q = p_j - p_i, l = sqrt(q.q), e = q / l, a_i = n^_i.e, a_j = n^_j.e; when fabs(a_i) < fabs(a_j) the roles swap:
 *                (n1, n2, dp) = (n^_j, n^_i, -e), otherwise (n^_i, n^_j, e).  f3 = n1.dp; v = dp x n1, a pair with |v| = 0 is not
 *                counted, else v /= |v|; w = n1 x v; f2 = v.n2; f1 = atan2(w.n2, n1.n2).  Eleven bins per feature:
 *                b1 = clamp((int)floor(11 ((f1 + pi) / (2 pi))), 0, 10), b2 = clamp((int)floor(11 ((f2 + 1) 0.5)), 0, 10), b3 from
 *                f3 as b2; the pair adds one to H_i[b1], H_i[11 + b2] and H_i[22 + b3].
 *   SPFH         H_i (33 counters) and c_i, the number of counted pairs: exact integers.  i is described iff it has an axis and
 *                c_i >= min_pairs.
 *   FPFH         for a described i, over the described j in N_i: w_ij = (double)r2 / (double)d(i, j), W_i = sum w_ij,
 *                R_i[b] = sum w_ij (double(H_j[b]) / double(c_j)): fp64 sums in the fixed order of the grid walk, no atomics.
 *                W_i > 0: F_i[b] = (float)(50 (double(H_i[b]) / double(c_i) + R_i[b] / W_i)); W_i = 0:
 *                F_i[b] = (float)((100 double(H_i[b])) / double(c_i)).  Each block of 11 bins sums to 100 up to rounding.  A point
 *                that is not described gets 33 NaNs.
 *   output       by original index; each array may be NULL.  desc_out: n x 33 floats; described_out: n bytes 0 / 1; pairs_out: n
 *                uint32 (c_i); spfh_out: n x 33 uint32 (H_i) and raw_out: n x 34 doubles (W_i, then R_i; zeros where the point is
 *                not described) -- test seams.  summary: n, described, the largest c_i and the mean c_i over the described points
 *                (an exact integer sum and one division; 0 when nothing is described).
 * H, c and described depend on the point set and the radius only; the last bits of raw follow the grid (another bounding box, a
 * permutation of the input).  The same input gives the same bits on every run, on every context and from plade_cloud_fpfh_dev.
 * Errors: PLADE_EINVAL for a NULL cloud or summary, n = 0, a non-finite coordinate, radius <= 0 or not finite (or its fp32 square not
 * finite or below FLT_MIN), min_pairs < 1; the context stays usable.  plade_stats_get then reports fpfh_grid_s (grid + axes),
 * fpfh_spfh_s, fpfh_weight_s (HIP events on the context's stream) and fpfh_described. */
typedef struct plade_fpfh_params {
    double radius;               /* must be set (> 0), absolute, in the cloud's units */
    int32_t min_pairs;           /* >= 1: the smallest number of counted pairs of a described point */
    int32_t reserved;            /* 0 */
} plade_fpfh_params;
typedef struct plade_fpfh_summary {
    uint64_t n, described;
    double mean_pairs;           /* of c_i over the described points */
    uint32_t max_pairs;          /* the largest c_i of any point */
    uint32_t reserved;           /* 0 */
} plade_fpfh_summary;
typedef struct plade_features plade_features; /* a device-resident table of n x 33 descriptors */
/* The defaults: radius = 0 (unset), min_pairs = 5.  Needs no GPU. */
void plade_fpfh_default_params(plade_fpfh_params *p);
int plade_cloud_fpfh(plade_ctx *ctx, const float *pos_nrm, uint32_t n, const plade_fpfh_params *params, float *desc_out,
                     uint8_t *described_out, uint32_t *pairs_out, uint32_t *spfh_out, double *raw_out, plade_fpfh_summary *summary);
/* The same on a resident cloud: the point data makes no host round trip, the outputs (host arrays) are the bits of plade_cloud_fpfh
 * on the cloud's rows.  features_out (or NULL): receives a resident copy of the descriptors for plade_match_features_dev, to be
 * released with plade_features_free. */
int plade_cloud_fpfh_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_fpfh_params *params, float *desc_out, uint8_t *described_out,
                         uint32_t *pairs_out, uint32_t *spfh_out, double *raw_out, plade_features **features_out,
                         plade_fpfh_summary *summary);
void plade_features_free(plade_features *f);

/* The match of two descriptor tables in feature space: src ns x 33 floats, tgt nt x 33, ns, nt >= 1.  A row is valid iff its first
 * value is not NaN (the rows plade_cloud_fpfh gives to points that are not described are not).
 *   distance     delta(s, t) = the sum over b = 0 .. 32, in that order, of (S_b - T_b) * (S_b - T_b), in fp32 without contraction
 *                (numpy float32 reproduces it bit for bit).  A target whose delta is NaN is passed over.
 *   neighbours   per valid source row the two smallest keys (delta, t) over the valid targets; ties go to the smaller index.
 *                nn_out: ns int32, -1 where there is none; d2_out: ns x 2 floats, NaN where there is none.
 *   mutual       with it the same search runs target -> source (back_out: nt int32) and s is kept iff back[nn[s]] == s.
 *   max_ratio    0: off; otherwise s is kept iff it has no second neighbour or d2[s][0] < (max_ratio * max_ratio) * d2[s][1] in fp32.
 *   output       nn_out, d2_out, back_out and corr_out may be NULL; back is computed when mutual is set or back_out is given.
 *                corr_out: cap x 2 int32, the kept (s, nn[s]) ascending in s; *n_corr: their exact number.  PLADE_ECAP when
 *                corr_out is given and *n_corr > cap (the first cap pairs are written).
 * Integers and fp32 bit patterns only: the same on every run and for every launch geometry.  Errors: PLADE_EINVAL for a NULL table
 * or n_corr, ns = 0 or nt = 0, max_ratio negative or not finite; the context stays usable.  plade_stats_get then reports
 * feat_match_s (HIP events) and feat_corr. */
typedef struct plade_feature_match_params {
    int32_t mutual;              /* 1: keep s only when its neighbour's neighbour is s */
    float max_ratio;             /* 0: off; else Lowe's ratio test on the distances (not squared) */
} plade_feature_match_params;
/* The defaults: mutual = 1, max_ratio = 0.  Needs no GPU. */
void plade_feature_match_default_params(plade_feature_match_params *p);
int plade_match_features(plade_ctx *ctx, const float *src, uint32_t ns, const float *tgt, uint32_t nt,
                         const plade_feature_match_params *params, int32_t *nn_out, float *d2_out, int32_t *back_out, int32_t *corr_out,
                         uint64_t cap, uint64_t *n_corr);
/* The same on two resident tables (plade_cloud_fpfh_dev): bit-identical results. */
int plade_match_features_dev(plade_ctx *ctx, plade_features *src, plade_features *tgt, const plade_feature_match_params *params,
                             int32_t *nn_out, float *d2_out, int32_t *back_out, int32_t *corr_out, uint64_t cap, uint64_t *n_corr);

/* ---- a rigid pose from feature correspondences: RANSAC with prerejection (no reference counterpart) --------------------------------
 * Semantics (plade_amd/csrc/corr_pose.h).  Source points (ns rows) and target points (nt rows): fp32 x y z,
 * `stride` >= 3 floats apart, finite; m correspondences as int32 pairs (s, t), 0 <= s < ns, 0 <= t < nt.  S_m, Q_m: the two points of
 * correspondence m widened to fp64.  All arithmetic below is fp64 with + - * / sqrt only, no contraction, every dot product
 * (a_x b_x + a_y b_y) + a_z b_z, so numpy reproduces every step up to the least-squares refit bit for bit.
 *   sample       base = mix64(seed) (splitmix64's finaliser); for k = 0, 1, 2: z = mix64(base ^ (4 h + k)),
 *                index = ((z >> 32) * m) >> 32: the triple (a, b, c) of hypothesis h.  status 1 when two of them are equal (no redraw).
 *   prerejection for the edges (a, b), (b, c), (c, a): ls = sqrt(|S_i - S_j|^2), lt = sqrt(|Q_i - Q_j|^2); status 2 when
 *                fmin(ls, lt) < edge_similarity * fmax(ls, lt) on any edge.
 *   transform    per side u = p_b - p_a, v = p_c - p_a, e1 = u / sqrt(u.u), w = u x v, e3 = w / sqrt(w.w), e2 = e3 x e1; status 3
 *                when sqrt(w.w) is 0 or not finite on either side.  R_ij = (e1t_i e1s_j + e2t_i e2s_j) + e3t_i e3s_j;
 *                c_s = ((S_a + S_b) + S_c) / 3.0, c_t likewise; t_i = c_t,i - ((R_i0 c_s0 + R_i1 c_s1) + R_i2 c_s2).  status 0:
 *                the hypothesis is scored.
 *   score        count_h = the number of m with d2 < inlier_dist * inlier_dist, x'_i = ((R_i0 S_0 + R_i1 S_1) + R_i2 S_2) + t_i,
 *                d = x' - Q, d2 = (d_x d_x + d_y d_y) + d_z d_z.  Exact integers.
 *   best         the scored hypothesis with the largest count, ties to the smallest h.  PLADE_EFAIL with T = identity and
 *                result->failure set when m < 3 (PLADE_CORR_POSE_TOO_FEW), nothing is scored (PLADE_CORR_POSE_NONE_SCORED) or the best
 *                count is below min_inliers (PLADE_CORR_POSE_FEW_INLIERS).
 *   refinement   at most refine_iterations times: over the inliers of the current T (in correspondence order, the fixed order of
 *                the cloud tools' summaries, workgroups of 256) n, sum S, sum Q, the means, then the nine sums
 *                C_ij = sum (Q - q)_i (S - s)_j; the least-squares rotation of C by Horn's unit quaternion (the eigenvector of the
 *                largest eigenvalue of the symmetric 4 x 4 matrix N(C), 12 cyclic Jacobi sweeps: a proper rotation by construction),
 *                t = q - R s.  The new T is accepted when its inlier count is >= the old one (refinements counts these); otherwise
 *                the old T stays and the loop stops.  It also stops when the flags did not change.
 *   output       T16: row-major fp32 4 x 4, the fp32 of the fp64 iterate.  result: see the struct; rmse = sqrt(sum d2 / inliers)
 *                under the final T.  inlier_out (m bytes 0 / 1) and the per-hypothesis test seams triple_out (H x 3 int32),
 *                status_out (H bytes), count_out (H uint32, 0 unless scored) and T_out (H x 12 doubles, rows of [R | t]; zeros unless
 *                scored) may each be NULL.
 * The same input gives the same bits on every run, on every context and from plade_estimate_pose_corr_dev.  Errors: PLADE_EINVAL for
 * NULL arguments, ns, nt or m = 0, a stride below 3, an index out of range, a non-finite coordinate, inlier_dist not finite or <= 0,
 * hypotheses outside 1 .. 2^24, edge_similarity outside [0, 1], min_inliers < 3, refine_iterations < 0; the context stays usable.
 * plade_stats_get then reports corr_pose_build_s, corr_pose_score_s, corr_pose_refine_s (HIP events), corr_pose_scored and
 * corr_pose_inliers. */
#define PLADE_CORR_POSE_TOO_FEW 1
#define PLADE_CORR_POSE_NONE_SCORED 2
#define PLADE_CORR_POSE_FEW_INLIERS 3
typedef struct plade_corr_pose_params {
    double inlier_dist;          /* must be set (> 0), absolute */
    double edge_similarity;      /* [0, 1]: the prerejection's bound on the ratio of the triangles' edge lengths */
    uint64_t seed;
    int32_t hypotheses;          /* 1 .. 2^24 */
    int32_t min_inliers;         /* >= 3 */
    int32_t refine_iterations;   /* >= 0 */
    int32_t reserved;            /* 0 */
} plade_corr_pose_params;
typedef struct plade_corr_pose_result {
    uint32_t hypotheses, scored; /* drawn; with status 0 */
    uint32_t best_hypothesis, best_count;
    uint32_t inliers;            /* under the final T */
    int32_t refinements;         /* accepted refits */
    int32_t failure;             /* 0 or PLADE_CORR_POSE_* */
    int32_t reserved;            /* 0 */
    double rmse, fitness;        /* sqrt(sum d2 / inliers); inliers / m */
    double T[12];                /* the fp64 iterate T16 is rounded from: 3 rows of [R | t] (the identity's when it failed) */
} plade_corr_pose_result;
/* The defaults: inlier_dist = 0 (unset), hypotheses = 65536, edge_similarity = 0.9, min_inliers = 3, refine_iterations = 5, seed = 0.
 * Needs no GPU. */
void plade_corr_pose_default_params(plade_corr_pose_params *p);
int plade_estimate_pose_corr(plade_ctx *ctx, const float *src, uint32_t ns, uint32_t src_stride, const float *tgt, uint32_t nt,
                             uint32_t tgt_stride, const int32_t *corr, uint64_t m, const plade_corr_pose_params *params, float *T16,
                             uint8_t *inlier_out, int32_t *triple_out, uint8_t *status_out, uint32_t *count_out, double *T_out,
                             plade_corr_pose_result *result);
/* The same on two resident clouds (the list stays a host array): bit-identical results. */
int plade_estimate_pose_corr_dev(plade_ctx *ctx, plade_cloud *src, plade_cloud *tgt, const int32_t *corr, uint64_t m,
                                 const plade_corr_pose_params *params, float *T16, uint8_t *inlier_out, int32_t *triple_out,
                                 uint8_t *status_out, uint32_t *count_out, double *T_out, plade_corr_pose_result *result);
/* Test seam: one refinement pass without the solve.  T12: 3 rows of [R | t] in fp64; flags_out (m bytes): d2 < inlier_dist^2 under
 * T12; moments_out: 17 doubles -- n, the mean of S (3), the mean of Q (3), C row-major (9), sum d2 -- over the flagged
 * correspondences (n = 0: the means are 0 / 0 = NaN, C and sum d2 are 0). */
int plade_corr_pose_moments(plade_ctx *ctx, const float *src, uint32_t ns, uint32_t src_stride, const float *tgt, uint32_t nt,
                            uint32_t tgt_stride, const int32_t *corr, uint64_t m, const double *T12, double inlier_dist,
                            uint8_t *flags_out, double *moments_out);
/* FPFH of both clouds (rows x y z nx ny nz), their match and the pose from the correspondences in one call, with nothing but the
 * summaries leaving the device in between: the bits of plade_cloud_fpfh on each cloud, plade_match_features (source -> target) and
 * plade_estimate_pose_corr chained.  match may be NULL (the defaults).  T16: source -> target, the identity with PLADE_EFAIL when
 * the pose fails (fewer than 3 correspondences included: PLADE_CORR_POSE_TOO_FEW).  corr_out (or NULL): cap x 2 int32, the first
 * min(cap, *n_corr) pairs (s, t); n_corr may be NULL.  Errors: those of the three calls. */
int plade_register_features(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm, uint32_t n_s,
                            const plade_fpfh_params *fpfh, const plade_feature_match_params *match, const plade_corr_pose_params *pose,
                            float *T16, plade_fpfh_summary *src_summary, plade_fpfh_summary *tgt_summary,
                            plade_corr_pose_result *result, int32_t *corr_out, uint64_t cap, uint64_t *n_corr);
/* The same on two resident clouds: bit-identical results. */
int plade_register_features_dev(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, const plade_fpfh_params *fpfh,
                                const plade_feature_match_params *match, const plade_corr_pose_params *pose, float *T16,
                                plade_fpfh_summary *src_summary, plade_fpfh_summary *tgt_summary, plade_corr_pose_result *result,
                                int32_t *corr_out, uint64_t cap, uint64_t *n_corr);

/* ---- keypoints: Intrinsic Shape Signatures (Zhong 2009, the scatter of PCL's ISSKeypoint3D; no reference counterpart) ---------------
 * Semantics (plade_amd/csrc/keypoints.h).  The few per cent of a cloud's points whose neighbourhood varies in
 * all three directions: what goes into the feature match in place of every point.  Input: n >= 1 rows of `stride` >= 3 floats, x y z
 * first, all finite; normals are not used.
 *   distance     d(i, j) = the fp32 squared distance of plade_smooth_cloud; rs2 = (float)rs * (float)rs, rn2 likewise (rn = 0: rs).
 *   scatter      N_i = { j : d(i, j) < rs2 } (strict; the point itself belongs to it), c_i = |N_i|, an exact integer.
 *                q_j = double(p_j) - double(p_i); M_i = sum q_a q_b: six fp64 sums xx xy xz yy yz zz in the fixed order of the grid
 *                walk, no atomics; C_i = M_i / double(c_i) entry by entry -- the scatter about the query point, not the centroid.
 *   eigenvalues  l1 >= l2 >= l3 of C_i by the trigonometric closed form of the normals' eigen-solve: q = tr / 3, p2 the squared
 *                norm of C - q I, pp = sqrt(p2 / 6), r = det((C - q I) / pp) / 2 clamped to [-1, 1], phi = acos(r) / 3;
 *                l_max = q + 2 pp cos(phi), l_min = q + 2 pp cos(phi + 2 pi / 3), l_mid = tr - l_max - l_min, then ordered with
 *                fmin / fmax; p2 = 0: all three are q.
 *   salient      c_i >= 3 && l1 > 0 && l2 < gamma21 * l1 && l3 < gamma32 * l2 && l3 > 1e-9 * l1, products and comparisons in fp64
 *                (a collinear or coplanar neighbourhood is flat by arithmetic, not by the sign of a rounding error).
 *                saliency_i = l3 when salient, else 0.
 *   suppression  B_i = { j : d(i, j) < rn2 }, i included, m_i = |B_i|.  i is a keypoint iff it is salient, m_i - 1 >= min_neighbours
 *                and no j in B_i, j != i, has saliency_j > saliency_i, or saliency_j == saliency_i with j < i: an exact function of
 *                the points and the saliencies.
 *   output       by original index; each array may be NULL.  keypoint_out: n bytes 0 / 1; index_out: cap uint32, the keypoints'
 *                indices ascending; *n_keypoints: their exact number -- PLADE_ECAP when index_out is given and *n_keypoints > cap
 *                (the first cap entries are written); saliency_out: n doubles; eigenvalues_out: n x 3 doubles, descending;
 *                count_out: n uint32 (c_i); nms_count_out: n uint32 (m_i); scatter_out: n x 6 doubles (M_i) -- a test seam.
 *                summary: n, salient, keypoints, the largest c_i.
 * c, m and, given the saliencies, the flags depend on the point set and the radii only; the last bits of M follow the grid (another
 * bounding box, a permutation of the input).  The same input gives the same bits on every run, on every context and from
 * plade_cloud_keypoints_iss_dev.  Keypoints of two independent samplings of a surface repeat badly at moderate densities: match the
 * keypoints of ONE cloud against every described point of the other (plade_register_keypoints), not keypoints against keypoints.
 * Errors: PLADE_EINVAL for a NULL cloud, params or summary, n = 0, stride < 3, a non-finite coordinate, salient_radius <= 0 or not
 * finite (or its fp32 square not finite or below FLT_MIN), non_max_radius neither 0 nor such a radius, a gamma outside (0, 1],
 * min_neighbours < 1; the context stays usable.  plade_stats_get then reports iss_grid_s, iss_scatter_s, iss_nms_s (HIP events on
 * the context's stream; the last one includes the list and the summary), iss_salient and iss_keypoints. */
typedef struct plade_iss_params {
    double salient_radius;       /* rs: must be set (> 0), absolute, in the cloud's units */
    double non_max_radius;       /* rn; 0: salient_radius */
    double gamma21, gamma32;     /* (0, 1]: the bounds on l2 / l1 and l3 / l2 */
    int32_t min_neighbours;      /* >= 1: the smallest m_i - 1 of a keypoint */
    int32_t reserved;            /* 0 */
} plade_iss_params;
typedef struct plade_iss_summary {
    uint64_t n, salient, keypoints;
    uint32_t max_count;          /* the largest c_i */
    uint32_t reserved;           /* 0 */
} plade_iss_summary;
/* The defaults: salient_radius = 0 (unset), non_max_radius = 0 (= salient_radius), gamma21 = gamma32 = 0.975, min_neighbours = 5.
 * Needs no GPU. */
void plade_iss_default_params(plade_iss_params *p);
int plade_cloud_keypoints_iss(plade_ctx *ctx, const float *rows, uint32_t n, uint32_t stride, const plade_iss_params *params,
                              uint8_t *keypoint_out, uint32_t *index_out, uint64_t cap, uint64_t *n_keypoints, double *saliency_out,
                              double *eigenvalues_out, uint32_t *count_out, uint32_t *nms_count_out, double *scatter_out,
                              plade_iss_summary *summary);
/* The same on a resident cloud: the point data makes no host round trip, the outputs (host arrays) are the bits of
 * plade_cloud_keypoints_iss on the cloud's rows. */
int plade_cloud_keypoints_iss_dev(plade_ctx *ctx, plade_cloud *cloud, const plade_iss_params *params, uint8_t *keypoint_out,
                                  uint32_t *index_out, uint64_t cap, uint64_t *n_keypoints, double *saliency_out,
                                  double *eigenvalues_out, uint32_t *count_out, uint32_t *nms_count_out, double *scatter_out,
                                  plade_iss_summary *summary);
/* Rows index[0 .. k - 1] of a resident descriptor table (plade_cloud_fpfh_dev) as a NEW resident table of k rows, bit for bit, for
 * plade_match_features_dev; release it with plade_features_free.  PLADE_EINVAL for a NULL argument, k = 0 or an index >= the
 * table's rows. */
int plade_features_select(plade_ctx *ctx, plade_features *features, const uint32_t *index, uint32_t k, plade_features **out);
/* plade_register_features with a keypoint detector in front of the match: ISS on the source's x y z, FPFH of both full clouds, the
 * source rows at the keypoints matched against the WHOLE target table (mutual as given), the pose from the correspondences -- with
 * nothing but the summaries and the two list lengths leaving the device in between.  The list (corr_out, *n_corr; original source
 * indices) and the pose carry the bits of plade_cloud_keypoints_iss, plade_cloud_fpfh, plade_features_select,
 * plade_match_features_dev and plade_estimate_pose_corr chained by hand.  Fewer than three correspondences (no keypoint included)
 * fail as there: PLADE_EFAIL, the identity, PLADE_CORR_POSE_TOO_FEW.  Errors: those of the calls it chains. */
int plade_register_keypoints(plade_ctx *ctx, const float *tgt_pos_nrm, uint32_t n_t, const float *src_pos_nrm, uint32_t n_s,
                             const plade_iss_params *iss, const plade_fpfh_params *fpfh, const plade_feature_match_params *match,
                             const plade_corr_pose_params *pose, float *T16, plade_iss_summary *iss_summary,
                             plade_fpfh_summary *src_summary, plade_fpfh_summary *tgt_summary, plade_corr_pose_result *result,
                             int32_t *corr_out, uint64_t cap, uint64_t *n_corr);
/* The same on two resident clouds: bit-identical results. */
int plade_register_keypoints_dev(plade_ctx *ctx, plade_cloud *tgt, plade_cloud *src, const plade_iss_params *iss,
                                 const plade_fpfh_params *fpfh, const plade_feature_match_params *match,
                                 const plade_corr_pose_params *pose, float *T16, plade_iss_summary *iss_summary,
                                 plade_fpfh_summary *src_summary, plade_fpfh_summary *tgt_summary, plade_corr_pose_result *result,
                                 int32_t *corr_out, uint64_t cap, uint64_t *n_corr);

/* ---- merging registered clouds: the step a scan-to-scan chain ends with (no reference counterpart) -----------------------------
 * Semantics (plade_amd/csrc/merge.h).  k clouds, 1 <= k <= 16; cloud c: n_c >= 1 rows x y z nx ny nz with
 * finite coordinates (the normals may be NaN); T: k row-major fp32 4 x 4 matrices, cloud c -> the output frame (NULL: identities,
 * which go through the same arithmetic); leaf >= 0 (fp32).
 *   transform  p' = ((r0 x + r1 y) + r2 z) + t and n' = (r0 nx + r1 ny) + r2 nz, row by row in fp32 (the match rule of ICP and
 *              distances).  n' gets no translation and is not renormalised; a non-finite normal stays non-finite.
 *   leaf = 0   the output is the transformed concatenation in (cloud, index) order: sum n_c rows, count = 1, mask = 1 << c.
 *   leaf > 0   inv = 1.f / leaf; voxel of p' = floor(p' * inv) per axis in fp32 minus floor(min * inv) of the bounding box of all
 *              p' (the key of plade_voxel_downsample); one row per occupied voxel in ascending (k, j, i).  Position: the fp64 sum of
 *              double(p') over the voxel's points, added one after the other in ascending (cloud, index) order, divided by the
 *              count in fp64, rounded to fp32.  Normal: s = the fp64 sum of double(n') in the same order over the points with a
 *              finite n'; q = (sx sx + sy sy) + sz sz; three NaNs when there is no such point or q == 0, else fp32(s / sqrt(q)).
 *              A plain sum, as PCL's normal accumulator: OPPOSITE NORMALS CANCEL (orient the scans consistently first).
 *   per row    count (uint32): the voxel's points; mask (uint32): bit c set when cloud c contributed.
 *   summary    n_in = sum n_c, n_out = rows, n_shared = rows whose mask has two or more bits, max_count = the largest count.
 * The result depends on the inputs only (not on launch shapes), is the same bits for host and resident clouds and on every run;
 * there are no floating-point atomics.  out_rows (6 floats per row), out_count and out_mask hold sum n_c rows; out_count and
 * out_mask may be NULL.
 * Errors: PLADE_EINVAL for k outside [1, 16], a NULL cloud, n_c = 0, a non-finite coordinate or T, leaf negative or not finite;
 * PLADE_ELIMIT for more than 2^18 leaves along an axis or sum n_c >= 2^31; the context stays usable.  plade_stats_get then reports
 * merge_transform_s, merge_sort_s (keys + sort), merge_runs_s, merge_fuse_s (HIP events on the context's stream) and merge_rows. */
typedef struct plade_merge_summary {
    uint64_t n_in, n_out, n_shared;
    uint32_t max_count;
    uint32_t reserved;           /* 0 */
} plade_merge_summary;
int plade_merge_clouds(plade_ctx *ctx, uint32_t k, const float *const *clouds, const uint32_t *n, const float *T /* k x 16 or NULL */,
                       float leaf, float *out_rows, uint32_t *out_count, uint32_t *out_mask, plade_merge_summary *summary);
/* The same on resident clouds into a NEW resident cloud (free it with plade_cloud_free): the point data makes no host round trip;
 * out_count / out_mask are host arrays of sum n_c entries or NULL.  The merged cloud is a resident cloud like any other. */
int plade_merge_clouds_dev(plade_ctx *ctx, uint32_t k, plade_cloud *const *clouds, const float *T /* k x 16 or NULL */, float leaf,
                           plade_cloud **out, uint32_t *out_count, uint32_t *out_mask, plade_merge_summary *summary);
/* Reads a resident cloud back, whichever call made it: *n = its rows; rows (x y z nx ny nz, room for capacity_rows rows) may be
 * NULL to ask for n only.  PLADE_ECAP when capacity_rows < n. */
int plade_cloud_download(plade_ctx *ctx, const plade_cloud *cloud, float *rows, uint32_t capacity_rows, uint32_t *n);

/* ---- instrumentation ---------------------------------------------------------------------- */
/* Named intermediates of the last registration (when params.dump != 0). Returns 0 if found;
 * the pointer stays valid until the next call on this ctx.
 * Among them the acceptance chains of every cloud's last detect call: [tgt_ | src_]extract_trace_{call_u, call_f, entry,
 * cand, slot_f, slot_u, slot_w} (no tag after plade_extract_planes; layout: ExtractTrace in plade_amd/csrc/ransac.h). */
int plade_dump_get(plade_ctx *ctx, const char *name, const void **ptr, int64_t *nbytes);
/* Per-stage GPU/host seconds and byte counts of the last registration:
 * names is a ';'-separated list, values has one double per name.
 * The cloud tools that search a point grid also report the grid of their last call: <tool>_grid_dx, _grid_dy, _grid_dz (cells per
 * axis) and <tool>_grid_cell (the cell size, which is larger than the one the tool asked for when the cap on the grid's size
 * applied), <tool> = normals, outliers, distances, smooth, scales, components, dbscan, fpfh, iss, m3c2_a and m3c2_b (the grids over the reference and
 * the compared cloud), icp and gicp (the first, widest stage; the linearize seams: their one stage). */
int plade_stats_get(plade_ctx *ctx, const char **names, const double **values, int32_t *count);
/* ---- diagnostic: the device-wide stable radix sort every grid of the path is built with ----------------
 * (radix_sort.hip; no reference counterpart -- it stands where PCL sorts voxel indices with std::sort,
 * voxel_grid.hpp:325, and where the kd-trees are built.)  keys: n keys of key_bytes (4 or 8) each, of which the low
 * `bits` bits are significant; vals: n u32 payloads.  Outputs are host arrays of the same shapes; equal keys keep
 * their input order. */
int plade_sort_pairs(plade_ctx *ctx, const void *keys, const uint32_t *vals, uint32_t n, int key_bytes, int bits,
                     void *keys_out, uint32_t *vals_out);
/* The same sort over up to 16 independent arrays in ONE launch sequence (how the Morton order of the clouds of a group is
 * built): segment s = items [seg_off[s], seg_off[s + 1]) of the u32 keys / values, seg_off ascending with seg_off[0] = 0 and
 * seg_off[nseg] = n; every segment is sorted on its own (stable) and left in its own range. */
int plade_sort_segments(plade_ctx *ctx, const uint32_t *keys, const uint32_t *vals, const uint32_t *seg_off, uint32_t nseg, int bits,
                        uint32_t *keys_out, uint32_t *vals_out);

/* Test seam: the device -> host hand-over every readback of the library goes through (n_ranges arrays of `words` 32-bit
 * words read back through one wait; no reference counterpart).  *mismatches = words that arrived wrong (0 expected). */
int plade_selftest_readback(plade_ctx *ctx, uint32_t n_ranges, uint32_t words, uint32_t *mismatches);

/* Diagnostic: `count` launches, on this context's stream, of a kernel of `blocks` workgroups that returns at once (mbytes = 0) or
 * streams `mbytes` MB of scratch memory; returns when they have finished.  tools/exp_interference.py runs it beside the
 * registrations to measure what foreign kernel boundaries, workgroup dispatches and memory traffic cost them. */
int plade_diag_launches(plade_ctx *ctx, uint32_t count, uint32_t blocks, uint32_t mbytes);
/* PLY ingest of the CLI: replaces load_ply_cloud (code/PLADE/util.cpp:1505-1546) over PlyReader::read
 * (code/PLADE/ply_reader.cpp:46-152, collect_elements :277-386) and rply (code/3rd_party/rply/rply.c).  Reads the `vertex`
 * element's float / double properties x y z (or X Y Z) and nx ny nz of an ascii, binary_little_endian or binary_big_endian
 * file into a malloc'ed n x 6 float array (x y z nx ny nz per point; free with plade_ply_free).  A binary file in the host's
 * byte order whose vertex element is exactly `float x y z nx ny nz` is read with one bulk read.  Returns PLADE_OK, or
 * PLADE_EINVAL with a message in `err` (NUL-terminated, truncated to err_cap) wherever the reference's function returns
 * false: unreadable / malformed file, no vertex points, "the number of points does not equal to the number of normals in the
 * file" (util.cpp:1533-1536), an empty cloud.  Host code only: no context, no GPU. */
int plade_ply_read(const char *path, float **pos_nrm, uint64_t *n, char *err, size_t err_cap);
/* plade_ply_read that also accepts a vertex element without nx ny nz: *has_normals = 0 and NaN in the normal columns (estimate
 * them with plade_estimate_normals / plade_cloud_upload_xyz, stride 6).  A file with normals reads as with plade_ply_read
 * (*has_normals = 1); every other failure keeps plade_ply_read's message.  Free with plade_ply_free.  Host code only. */
int plade_ply_read_points(const char *path, float **pos_nrm, uint64_t *n, int32_t *has_normals, char *err, size_t err_cap);
void plade_ply_free(float *pos_nrm);
/* Seam of the one host-side stage whose tie-breaking shapes the result: the order in which
 * std::sort(sortVec.begin(), sortVec.end(), myCompareGreater) (code/PLADE/util.cpp:335-345, util.h:347-365) leaves clusters
 * of the given sizes -- order[i] = index of the cluster at sorted position i.  mode 0: the library's implementation
 * (exact_sort.h: libstdc++'s introsort with a block-wise partition), 1: std::sort itself, 2 / 3: the block-wise / the
 * sequential partition with the recursion depth limited to `depth_limit` (< 0: the library's 2 lg n).  Host code only: no
 * context, no GPU. */
int plade_diag_cluster_order(const float *sizes, uint32_t n, int32_t mode, int32_t depth_limit, int32_t *order);
/* Host seam of the register form of the reference's least-squares solver (plade_amd/csrc/k_svd.h, RegSolver: cv::solve(...,
 * DECOMP_SVD) of opencv/modules/core/src/lapack.cpp:533-812, 1335-1460 with every loop unrolled over compile-time bounds): the
 * functions the kernels inline, instantiated for the host, so that the arithmetic can be compared with the oracle's
 * restatement where there is no GPU.  kind 0: n systems of ComputeNearstTwoPointsOfTwo3DLine (code/PLADE/util.cpp:1167-1229;
 * a = u1, b = p1, c = u2, d = p2, each n x 3; o1 = point1, o2 = point2); kind 1: of ComputeIntersectionPointOf23DLine
 * (util.cpp:1461-1500; a = v1, b = p1, c = v2, d = p2; o1 = the point, o2 unused).  ok[i]: 1 solved, 0 a column of the system
 * vanished (the kernels hand such a system to the general form, which completes it as lapack.cpp:650-699 does), -1 the
 * reference's guard fired (identical directions / |v1.v2| > 0.9999).  Host code only: no context, no GPU. */
int plade_diag_line_solver_host(int32_t kind, const float *a, const float *b, const float *c, const float *d, uint32_t n,
                                float *o1, float *o2, int32_t *ok);
/* Times `iters` launches of one hot kernel on resident synthetic-shaped data with HIP events on
 * the ctx stream (used by bench.py for the roofline figure): which = "score" | "overlap" | "match". */
int plade_kernel_time(plade_ctx *ctx, const char *which, int iters, double *avg_seconds,
                      double *algorithmic_bytes_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* PLADE_HIP_H */
