// plade_amd/csrc/plade_host.cpp -- the four registration() overloads of code/PLADE/plade.h (and
// PlaneExtraction::detect, load_ply_cloud) on top of the C ABI of libplade_hip.so.  Console messages,
// return values and the swap/invert rule follow code/PLADE/plade.cpp:583-706.
#include "plade.h"
#include "cli_switches.h"
#include "plade_hip.h"
#include "ply_reader.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <iostream>
#include <mutex>
#include <thread>

namespace {

thread_local int g_device = 0;
thread_local plade_ctx *g_ctx = nullptr;
thread_local int g_ctx_device = -1;
// console of the calling thread: std::cout / std::cerr unless the caller collects the messages itself (the CLI's batch
// workers do, so that concurrent registrations do not interleave their lines)
thread_local std::ostream *g_out = nullptr, *g_err = nullptr;
std::ostream &con_out() { return g_out ? *g_out : std::cout; }
std::ostream &con_err() { return g_err ? *g_err : std::cerr; }

// PLADE_TRACE_CLI=1: what the process spends where, on std::cerr (seconds since the first call)
double trace_now() {
    static const auto t0 = std::chrono::steady_clock::now();
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
bool trace_on() { static const bool v = getenv("PLADE_TRACE_CLI") != nullptr; return v; }
void trace(const char *what) {
    if (!trace_on()) return;
    char b[160];
    snprintf(b, sizeof(b), "[plade %8.3f s] %s\n", trace_now(), what);
    std::cerr << b << std::flush;
}

// The list-valued switches (cli_switches.h parses them): each is read once per process, where it is first needed, and what the
// parser has to say about a rejected value goes to std::cerr, not to the calling thread's console.
using cli_switches::GicpSwitch; using cli_switches::M3c2Switch; using cli_switches::FpfhSwitch; using cli_switches::FeatureRegisterSwitch;
using cli_switches::KeypointSwitch; using cli_switches::OutlierSwitch; using cli_switches::ComponentSwitch; using cli_switches::SmoothSwitch;
using cli_switches::SubsampleSwitch; using cli_switches::OrientSwitch; using cli_switches::ScaleSwitch; using cli_switches::DbscanSwitch;
template <class S> S latched(const cli_switches::Parsed<S> &p) {
    if (!p.warning.empty()) std::cerr << p.warning << std::endl;
    return p.value;
}

plade_ctx *context() {
    if (g_ctx && g_ctx_device == g_device) return g_ctx;
    if (g_ctx) { plade_ctx_destroy(g_ctx); g_ctx = nullptr; }
    trace("context: creating");
    if (plade_ctx_create(g_device, &g_ctx) != PLADE_OK) {
        con_err() << "PLADE: cannot create a GPU context on device " << g_device
                  << " (libplade_hip.so needs a gfx950 GPU; there is no CPU fallback)" << std::endl;
        return nullptr;
    }
    g_ctx_device = g_device;
    // opt-in switches of the C++ API / CLI, which have no parameter to carry them (the C ABI's defaults are the
    // reference's values and do not look at the environment): see include/plade_hip.h, plade_params
    plade_params prm;
    plade_default_params(&prm);
    bool changed = false;
    if (const char *w = getenv("PLADE_HOST_WAIT")) { prm.host_wait = (w[0] == 's' && w[1] == 'l') ? 1 : 0; changed = true; }
    if (const char *w = getenv("PLADE_ORIENT_NORMALS")) { prm.orient_normals = atoi(w) != 0; changed = true; }
    if (const char *w = getenv("PLADE_UNORIENTED_NORMALS")) { prm.unoriented_normals = atoi(w) != 0; changed = true; }
    if (const char *w = getenv("PLADE_RANSAC_TOPUP")) { prm.ransac_topup = atoi(w) != 0; changed = true; }
    if (const char *w = getenv("PLADE_CLOSEST_POINT_MODE")) { prm.closest_point_mode = (!strcmp(w, "closed_form") || !strcmp(w, "0")) ? 0 : 1; changed = true; }
    if (changed) (void)plade_set_params(g_ctx, &prm);
    trace("context: ready");
    return g_ctx;
}

// The staging arrays of a worker thread, page-locked: the library then uploads them by asynchronous DMA (~50 GB/s) instead of
// through the runtime's bounce buffer (pageable memory: ~6-10 GB/s, and the call blocks meanwhile) -- at 48 MB per pair the
// difference is most of a long list's wall time.  An array is registered once and again only when its allocation has moved.
struct PinnedVec {
    const float *ptr = nullptr; size_t bytes = 0; plade_ctx *owner = nullptr;
    void release() { if (ptr && owner && owner == g_ctx) (void)plade_host_unpin(owner, ptr); ptr = nullptr; bytes = 0; owner = nullptr; }
    void cover(plade_ctx *ctx, const std::vector<float> &v) {
        const size_t want = v.capacity() * sizeof(float);
        if (ptr == v.data() && bytes == want && owner == ctx) return;
        release();
        if (!ctx || !want) return;
        if (plade_host_pin(ctx, v.data(), want) == PLADE_OK) { ptr = v.data(); bytes = want; owner = ctx; }
    }
};
thread_local PinnedVec g_pins[2 * PLADE_GROUP_MAX];

std::vector<float> flatten(const pcl::PointCloud<pcl::PointNormal> &c) {
    std::vector<float> a(6 * c.size());
    for (size_t i = 0; i < c.size(); ++i) {
        const pcl::PointNormal &p = c.points[i];
        float *o = &a[6 * i];
        o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = p.normal_x; o[4] = p.normal_y; o[5] = p.normal_z;
    }
    return a;
}

void unflatten(const float *rows, size_t n, pcl::PointCloud<pcl::PointNormal> &c) {
    c.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const float *p = rows + 6 * i;
        c.at(i) = pcl::PointNormal(p[0], p[1], p[2], p[3], p[4], p[5]);
    }
}

void to_matrix(const float *T16, Eigen::Matrix<float, 4, 4> &m) {
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m(r, c) = T16[4 * r + c];
}
void to_T16(const Eigen::Matrix<float, 4, 4> &m, float *T16) {
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T16[4 * r + c] = m(r, c);
}

// the library's correspondence array (source, target, source, target, ...) as the C++ API hands it out
std::vector<std::pair<int, int>> to_pairs(const std::vector<int32_t> &corr) {
    std::vector<std::pair<int, int>> out(corr.size() / 2);
    for (size_t k = 0; k < out.size(); ++k) out[k] = {corr[2 * k], corr[2 * k + 1]};
    return out;
}

void pack_planes(const std::vector<PLANE> &planes, std::vector<float> &coef, std::vector<int32_t> &off, std::vector<int32_t> &idx) {
    coef.clear(); off.assign(1, 0); idx.clear();
    for (const PLANE &p : planes) {
        coef.push_back(p.normal.x()); coef.push_back(p.normal.y()); coef.push_back(p.normal.z()); coef.push_back(p.d);
        idx.insert(idx.end(), p.begin(), p.end());
        off.push_back((int32_t)idx.size());
    }
}

struct Watch {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::string str() const {
        double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        char buf[64];
        snprintf(buf, sizeof(buf), "%.3f sec", s);
        return buf;
    }
};

// PLADE_ESTIMATE_NORMALS=<k> (opt-in, 0 / unset = off): a PLY without nx ny nz is accepted and its normals are estimated on the
// GPU (plade_estimate_normals: k nearest neighbours, viewpoint (0, 0, 0) of the file's own frame); files with normals keep them.
// Unset, such a file fails with the reference's message (util.cpp:1533-1536).
int estimate_normals_k() {
    static const int k = [] { const char *w = getenv("PLADE_ESTIMATE_NORMALS"); return w ? atoi(w) : 0; }();
    return k;
}
// read_ply_pos_nrm, or under PLADE_ESTIMATE_NORMALS read_ply_points (*estimate: the file had no normals)
bool read_ply_cloud(const std::string &file_name, std::vector<float> &buf, std::string &err, std::vector<std::string> *warnings,
                    const std::function<void()> *before_grow, bool *estimate) {
    *estimate = false;
    if (!estimate_normals_k()) return plade::read_ply_pos_nrm(file_name, buf, err, warnings, before_grow);
    bool has_normals = true;
    if (!plade::read_ply_points(file_name, buf, has_normals, err, warnings, before_grow)) return false;
    *estimate = !has_normals;
    return true;
}
// the normal columns of an x y z nx ny nz array, estimated in place on the calling thread's context
bool estimate_in_place(const std::string &file_name, std::vector<float> &buf);

// PLADE_REFINE_ICP=1 (opt-in, 0 / unset = off): every pair that registered is refined by point-to-plane ICP on the GPU
// (plade_refine_icp with the default parameters, on the calling thread's context) before its transformation is returned; one
// console line per refined pair.  A refinement that fails keeps PLADE's transformation and prints a warning.  Unset, nothing
// changes.
bool refine_icp_on() {
    static const bool on = [] { const char *w = getenv("PLADE_REFINE_ICP"); return w && atoi(w) != 0; }();
    return on;
}
// T16 (source -> target of the packed arrays) refined in place by `call`; false (T16 unchanged, a warning printed) when the
// refinement fails.  `tag` opens the trace lines, `name` the console's; `cost`: the result's field of that name, if it has one
template <class Result, class Call>
bool refine_by(plade_ctx *ctx, float *T16, const std::string &tag, const char *name, const double Result::*cost, Call call) {
    Result res;
    float out[16];
    trace((tag + ": refining").c_str());
    const int rc = call(out, &res);
    trace((tag + ": done").c_str());
    if (rc != PLADE_OK) {
        con_err() << "warning: " << name << " refinement failed (" << plade_last_error(ctx) << "); PLADE's transformation is kept" << std::endl;
        return false;
    }
    memcpy(T16, out, sizeof(out));
    char b[240], extra[64] = "";
    if (cost) snprintf(extra, sizeof(extra), "cost %.6g, ", res.*cost);
    snprintf(b, sizeof(b), "%s refinement: %d iterations, %s, rmse %.6g, %sfitness %.4f", name, res.iterations,
             res.converged ? "converged" : "not converged", res.rmse, extra, res.fitness);
    con_out() << b << std::endl;
    return true;
}
bool refine_packed(plade_ctx *ctx, float *T16, const float *tg, size_t n_t, const float *sr, size_t n_s) {
    return refine_by<plade_icp_result>(ctx, T16, "icp", "ICP", nullptr, [&](float *out, plade_icp_result *res) {
        return plade_refine_icp(ctx, tg, (uint32_t)n_t, sr, (uint32_t)n_s, T16, nullptr, out, res);
    });
}

// PLADE_REFINE_GICP=1[,<epsilon>] (opt-in, 0 / unset = off): every pair that registered is refined by plane-to-plane ICP on the GPU
// (plade_refine_gicp with the default parameters and the given epsilon, 0 < epsilon <= 1, default 1e-3; 1 = point-to-point) before
// evaluation and merge; one console line per refined pair.  A refinement that fails keeps PLADE's transformation and prints a
// warning.  A value that does not parse prints one warning and refines nothing.  With PLADE_REFINE_ICP also set, this is the
// refinement that runs, and one warning says so.  Unset, nothing changes.  The variable is read when the first pair has registered
// (like PLADE_EVALUATE): the warnings appear there, once per process.
const GicpSwitch &refine_gicp_switch() {
    static const GicpSwitch sw = [] {
        const GicpSwitch g = latched(cli_switches::parse_refine_gicp(getenv("PLADE_REFINE_GICP")));
        if (g.on && refine_icp_on())
            std::cerr << "warning: PLADE_REFINE_ICP and PLADE_REFINE_GICP are both set; the plane-to-plane refinement runs" << std::endl;
        return g;
    }();
    return sw;
}
bool refine_gicp_packed(plade_ctx *ctx, float *T16, const float *tg, size_t n_t, const float *sr, size_t n_s, double epsilon) {
    plade_gicp_params prm;
    plade_gicp_default_params(&prm);
    if (epsilon != 0.0) prm.epsilon = epsilon;
    return refine_by<plade_gicp_result>(ctx, T16, "gicp", "GICP", &plade_gicp_result::cost, [&](float *out, plade_gicp_result *res) {
        return plade_refine_gicp(ctx, tg, (uint32_t)n_t, sr, (uint32_t)n_s, T16, &prm, out, res);
    });
}
// the refinement the environment selects, if any
void refine_selected(plade_ctx *ctx, float *T16, const float *tg, size_t n_t, const float *sr, size_t n_s) {
    const GicpSwitch &g = refine_gicp_switch();
    if (g.on) refine_gicp_packed(ctx, T16, tg, n_t, sr, n_s, g.epsilon);
    else if (refine_icp_on()) refine_packed(ctx, T16, tg, n_t, sr, n_s);
}

// PLADE_EVALUATE=<d> (opt-in, absolute, in the clouds' units): every pair that registered -- after the ICP refinement when that
// is on -- is evaluated at max_dist d (plade_cloud_distances, no per-point outputs) and one console line reports its fitness.
// The pair is evaluated as it was registered (after the target / source switch).  A value that is not a positive finite number
// prints one warning and evaluates nothing; unset, nothing changes.
float evaluate_dist() {
    static const float d = latched(cli_switches::parse_evaluate(getenv("PLADE_EVALUATE")));
    return d;
}
bool evaluate_packed(plade_ctx *ctx, const float *T16, const float *tg, size_t n_t, const float *sr, size_t n_s, float max_dist,
                     plade_distance_summary &s) {
    trace("evaluate: measuring");
    const int rc = plade_cloud_distances(ctx, tg, (uint32_t)n_t, sr, (uint32_t)n_s, 6, T16, max_dist, nullptr, nullptr, nullptr, &s);
    trace("evaluate: done");
    if (rc != PLADE_OK) {
        con_err() << "warning: evaluation failed (" << plade_last_error(ctx) << ")" << std::endl;
        return false;
    }
    return true;
}
void evaluate_line(plade_ctx *ctx, const float *T16, const float *tg, size_t n_t, const float *sr, size_t n_s) {
    const float d = evaluate_dist();
    plade_distance_summary s;
    if (!(d > 0.f) || !evaluate_packed(ctx, T16, tg, n_t, sr, n_s, d, s)) return;
    char b[240];
    snprintf(b, sizeof(b), "evaluation: fitness %.4f, rmse %.6g, %llu of %llu source points within %g", s.fitness, s.rmse,
             (unsigned long long)s.count, (unsigned long long)s.n, (double)d);
    con_out() << b << std::endl;
}

// PLADE_CONSISTENT_NORMALS=<radius>[,<mode>[,<inward>]] (opt-in, 0 / unset = off; the radius absolute, in the clouds' units): the normals
// of both clouds of a pair are put on one side of the surface per component of the graph "closer than radius" (plade_orient_normals:
// the flips follow the minimum spanning forest of the flattest neighbour pairs; mode 0, the default, lets every component vote
// against the origin, mode 1 takes the extreme point along +z; inward 1 inverts the decision), as the last preparation step that
// touches normals -- after PLADE_SMOOTH and PLADE_ESTIMATE_NORMALS, before PLADE_SUBSAMPLE; one console line per cloud.  Positions,
// point count and order stay.  A value that does not parse (radius negative, not finite or so small that its fp32 square is below
// FLT_MIN, mode or inward not 0 or 1, anything behind them) prints one warning and orients nothing; unset, nothing changes.
const OrientSwitch &orient_switch() {
    static const OrientSwitch sw = latched(cli_switches::parse_consistent_normals(getenv("PLADE_CONSISTENT_NORMALS")));
    return sw;
}
// the normal columns of an x y z nx ny nz array oriented in place (view / dir: nullptr = the origin / +z)
bool orient_packed(plade_ctx *ctx, float *rows, size_t n, double radius, int mode, int inward, const float *view, const float *dir,
                   plade_orient_summary &s) {
    plade_orient_params prm;
    plade_orient_default_params(&prm);
    prm.radius = radius; prm.mode = mode; prm.inward = inward;
    if (view) memcpy(prm.viewpoint, view, 12);
    if (dir) memcpy(prm.direction, dir, 12);
    trace("orient: orienting");
    // (in place: the upload of the rows precedes the read-back on the context's stream)
    const int rc = plade_orient_normals(ctx, rows, (uint32_t)n, &prm, rows, nullptr, nullptr, &s);
    trace("orient: done");
    if (rc != PLADE_OK) {
        con_err() << "normal orientation failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    return true;
}
bool orient_in_place(std::vector<float> &buf) {
    const OrientSwitch &sw = orient_switch();
    if (!(sw.radius > 0.0) || buf.empty()) return true;
    plade_ctx *ctx = context();
    if (!ctx) return false;
    plade_orient_summary s;
    if (!orient_packed(ctx, buf.data(), buf.size() / 6, sw.radius, sw.mode, sw.inward, nullptr, nullptr, s)) return false;
    char b[240];
    snprintf(b, sizeof(b), "consistent normals: flipped %u of %u points in %u components (radius %g, %u without a normal, %u rounds)", s.flipped,
             s.n, s.components, sw.radius, s.unoriented, s.rounds);
    con_out() << b << std::endl;
    return true;
}

// PLADE_SUBSAMPLE=<spacing>[,<seed>] (opt-in, 0 / unset = off; the spacing absolute, in the clouds' units): both clouds of a pair are
// thinned to a subset of their own points in which no two are closer than spacing and every dropped point has a kept one closer than
// spacing (plade_subsample_spacing; seed 0 when not given), as the LAST preparation step -- after the filters and after
// PLADE_ESTIMATE_NORMALS, so the normals come from the full density; one console line per cloud.  A value that does not parse (spacing
// negative, not finite or so small that its fp32 square is below FLT_MIN, seed not an integer >= 0, anything behind them) prints one
// warning and thins nothing; unset, nothing changes.
const SubsampleSwitch &subsample_switch() {
    static const SubsampleSwitch sw = latched(cli_switches::parse_subsample(getenv("PLADE_SUBSAMPLE")));
    return sw;
}
// the rows of an x y z nx ny nz array that the subsample keeps (the normal columns, NaN included, keep their bits): into `out`,
// which may be `rows` itself; kept_index: their ascending indices (n words) when wanted
bool subsample_packed(plade_ctx *ctx, const float *rows, size_t n, double spacing, uint64_t seed, float *out, plade_subsample_summary &s,
                      uint32_t *kept_index = nullptr) {
    plade_subsample_params prm;
    plade_subsample_default_params(&prm);
    prm.spacing = spacing; prm.seed = seed;
    trace("subsample: thinning");
    // (in place: the upload of the rows precedes the read-back of the kept ones on the context's stream)
    const int rc = plade_subsample_spacing(ctx, rows, (uint32_t)n, 6, &prm, nullptr, kept_index, out, nullptr, &s);
    trace("subsample: done");
    if (rc != PLADE_OK) {
        con_err() << "subsampling failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    return true;
}
bool subsample_in_place(std::vector<float> &buf) {
    const SubsampleSwitch &sw = subsample_switch();
    if (!(sw.spacing > 0.0) || buf.empty()) return true;
    plade_ctx *ctx = context();
    if (!ctx) return false;
    plade_subsample_summary s;
    if (!subsample_packed(ctx, buf.data(), buf.size() / 6, sw.spacing, sw.seed, buf.data(), s)) return false;
    buf.resize((size_t)s.kept * 6);
    char b[200];
    snprintf(b, sizeof(b), "subsample: kept %u of %u points (spacing %g, %u rounds)", s.kept, s.n, sw.spacing, s.rounds);
    con_out() << b << std::endl;
    return true;
}

// PLADE_DBSCAN=<radius>,<min_points>[,<min_size>[,<keep_largest>]] (opt-in, unset = off; the radius absolute, in the clouds' units): both
// clouds of a pair keep only the points of their DBSCAN clusters (plade_cluster_dbscan: a core point has at least min_points points
// closer than radius, itself included; border points join the cluster of their nearest core point; noise goes) with at least
// min_size points (1 when not given), with keep_largest = m > 0 only the m largest of them, after PLADE_KEEP_COMPONENTS and before
// PLADE_SMOOTH; one console line per cloud.  A value that does not parse (radius not positive and finite or so small that its fp32
// square is below FLT_MIN, min_points or min_size not an integer >= 1, keep_largest not an integer >= 0, anything behind them) prints
// one warning and filters nothing; unset, nothing changes.
const DbscanSwitch &dbscan_switch() {
    static const DbscanSwitch sw = latched(cli_switches::parse_dbscan(getenv("PLADE_DBSCAN")));
    return sw;
}
// the rows (`stride` floats each) that DBSCAN keeps, into `out`, which may be `rows` itself (every float keeps its bits); label: one
// int32 per input point when wanted.  false: a message has been printed
bool dbscan_packed(plade_ctx *ctx, const float *rows, size_t n, uint32_t stride, double radius, int min_points, int min_size, int keep_largest,
                   int32_t *label, float *out, plade_dbscan_summary &s) {
    plade_dbscan_params prm;
    plade_dbscan_default_params(&prm);
    prm.radius = radius; prm.min_points = min_points; prm.min_size = min_size; prm.keep_largest = keep_largest;
    trace("dbscan: clustering");
    // (in place: the upload of the rows precedes the read-back of the kept ones on the context's stream)
    const int rc = plade_cluster_dbscan(ctx, rows, (uint32_t)n, stride, &prm, label, nullptr, nullptr, nullptr, nullptr, out, &s);
    trace("dbscan: done");
    if (rc != PLADE_OK) {
        con_err() << "clustering failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    return true;
}
bool dbscan_in_place(std::vector<float> &buf) {
    const DbscanSwitch &sw = dbscan_switch();
    if (!sw.on || buf.empty()) return true;
    plade_ctx *ctx = context();
    if (!ctx) return false;
    plade_dbscan_summary s;
    if (!dbscan_packed(ctx, buf.data(), buf.size() / 6, 6, sw.radius, sw.min_points, sw.min_size, sw.keep_largest, nullptr, buf.data(), s))
        return false;
    buf.resize((size_t)s.kept * 6);
    char b[280];
    snprintf(b, sizeof(b), "dbscan: kept %llu of %llu points in %llu of %llu clusters (largest %u; %llu core, %llu border, %llu noise)",
             (unsigned long long)s.kept, (unsigned long long)s.n, (unsigned long long)s.kept_clusters, (unsigned long long)s.clusters, s.largest,
             (unsigned long long)s.core, (unsigned long long)s.border, (unsigned long long)s.noise);
    con_out() << b << std::endl;
    return true;
}

// PLADE_M3C2=<radius>,<depth>[,<min_points>[,<reg_error>]] (opt-in, absolute, in the clouds' units): every pair that registered -- after
// the ICP / GICP refinement when that is on -- is compared by M3C2 distances on the GPU (plade_cloud_m3c2: core points = reference
// = the target with its normals, compared = the source under the final transformation; min_points 4 and reg_error 0 when not
// given) and one console line reports the library's summary.  The pair is compared as it was registered (after the target / source
// switch).  A value that does not parse (radius or depth not positive and finite, min_points not an integer >= 2, reg_error negative
// or not finite, anything behind them) prints one warning and compares nothing; unset, nothing changes.
const M3c2Switch &m3c2_switch() {
    static const M3c2Switch sw = latched(cli_switches::parse_m3c2(getenv("PLADE_M3C2")));
    return sw;
}
// M3C2 of the packed source under T16 against the packed reference at the given core points (all x y z nx ny nz rows); dist: one
// double per core point when wanted; significant: one byte 0 / 1 per core point when wanted.  false: a message has been printed
bool m3c2_packed(plade_ctx *ctx, const float *T16, const float *core, size_t m, const float *ref, size_t n_a, const float *cmp, size_t n_b,
                 double radius, double depth, int min_points, double reg_error, double *dist, plade_m3c2_summary &s,
                 uint8_t *significant = nullptr) {
    plade_m3c2_params prm;
    plade_m3c2_default_params(&prm);
    prm.radius = radius; prm.depth = depth; prm.min_points = min_points; prm.reg_error = reg_error;
    trace("m3c2: comparing");
    const int rc = plade_cloud_m3c2(ctx, core, (uint32_t)m, ref, (uint32_t)n_a, 6, cmp, (uint32_t)n_b, 6, T16, &prm, dist, nullptr, significant,
                                    nullptr, nullptr, nullptr, &s);
    trace("m3c2: done");
    if (rc != PLADE_OK) {
        con_err() << "cloud comparison failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    return true;
}
// PLADE_M3C2_CORE=<spacing>[,<seed>] (opt-in, 0 / unset = off; absolute, in the clouds' units; it acts only together with PLADE_M3C2):
// the core points of the comparison are the minimum-spacing subsample of the target (plade_subsample_spacing; seed 0 when not given),
// with their normals, instead of the whole target; the m3c2 line's core-point count shows it.  A value that does not parse (spacing
// negative, not finite or so small that its fp32 square is below FLT_MIN, seed not an integer >= 0, anything behind them) prints one
// warning and the whole target stays the core points; unset, nothing changes.
const SubsampleSwitch &m3c2_core_switch() {
    static const SubsampleSwitch sw = latched(cli_switches::parse_m3c2_core(getenv("PLADE_M3C2_CORE")));
    return sw;
}
// PLADE_M3C2_NORMALS=<r_min>,<r_max>[,<scales>[,<mode>]] (opt-in; absolute, in the clouds' units; it acts only together with PLADE_M3C2):
// the core points of the comparison -- the whole target, or the PLADE_M3C2_CORE subsample -- get their normals from the multi-scale
// estimate on the target (plade_cloud_scale_features at the core points' indices: `scales` radii from r_min to r_max in equal steps,
// 2 .. 8, 4 when not given; mode 0 = the most planar scale, M3C2's rule, 1 = the smallest surface variation; orient = 1, so a new
// normal points to the side of the file's normal), instead of the target file's normals; a core point with no fitted scale carries a
// NaN normal, which M3C2 reports as "no axis".  One console line before the m3c2 line.  A value that does not parse (a radius not
// positive and finite or its fp32 square below FLT_MIN, r_min >= r_max or steps so small that the fp32 squares of the radii do not
// ascend strictly, scales not an integer in [2, 8], mode not 0 or 1, anything behind them) prints one warning and the core points
// keep their normals; unset, nothing changes.
const ScaleSwitch &m3c2_normals_switch() {
    static const ScaleSwitch sw = latched(cli_switches::parse_m3c2_normals(getenv("PLADE_M3C2_NORMALS")));
    return sw;
}
// PLADE_M3C2_CLUSTERS=<radius>[,<min_points>[,<min_size>]] (opt-in; absolute, in the clouds' units; it acts only together with PLADE_M3C2):
// the significant core points of the comparison are grouped into objects of change by DBSCAN on their positions
// (plade_cluster_dbscan; min_points 4 and min_size 1 when not given), and one console line after the m3c2 line reports the clusters
// that hold at least min_size points, the significant core points, the largest cluster and the points left as noise; with no
// significant core point the line carries zeros and the library is not called.  A value that does not parse (radius not positive
// and finite or so small that its fp32 square is below FLT_MIN, min_points or min_size not an integer >= 1, anything behind them)
// prints one warning and clusters nothing; unset, nothing changes.
const DbscanSwitch &m3c2_clusters_switch() {
    static const DbscanSwitch sw = latched(cli_switches::parse_m3c2_clusters(getenv("PLADE_M3C2_CLUSTERS")));
    return sw;
}
// the multi-scale normals of the packed rows at `query` (k ascending indices; nullptr: all n points) into nrm (3 floats per query);
// orient_by_rows: a normal keeps the side of its row's own.  false: a message has been printed
bool scale_normals_packed(plade_ctx *ctx, const float *rows, size_t n, const uint32_t *query, size_t k, const double *radii, int scales,
                          int mode, int min_neighbours, bool orient_by_rows, float *nrm, plade_scale_summary &s) {
    plade_scale_params prm;
    plade_scale_default_params(&prm);
    prm.scales = scales;
    for (int t = 0; t < scales && t < 8; ++t) prm.radii[t] = radii[t];
    prm.mode = mode; prm.min_neighbours = min_neighbours; prm.orient = orient_by_rows ? 1 : 0;
    trace("scales: fitting");
    const int rc = plade_cloud_scale_features(ctx, rows, (uint32_t)n, 6, query, (uint32_t)k, &prm, nullptr, nrm, nullptr, nullptr, nullptr,
                                              nullptr, nullptr, nullptr, &s);
    trace("scales: done");
    if (rc != PLADE_OK) {
        con_err() << "multi-scale normals failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    return true;
}
void m3c2_line(plade_ctx *ctx, const float *T16, const float *tg, size_t n_t, const float *sr, size_t n_s) {
    const M3c2Switch &sw = m3c2_switch();
    if (!sw.on) return;
    const SubsampleSwitch &cs = m3c2_core_switch();
    const ScaleSwitch &ns = m3c2_normals_switch();
    std::vector<float> core;
    std::vector<uint32_t> kept;
    const float *cp = tg;
    size_t m = n_t;
    if (cs.spacing > 0.0 && n_t) {
        core.resize(n_t * 6);
        if (ns.on) kept.resize(n_t);
        plade_subsample_summary ss;
        if (!subsample_packed(ctx, tg, n_t, cs.spacing, cs.seed, core.data(), ss, ns.on ? kept.data() : nullptr)) return;
        cp = core.data(); m = ss.kept;
    }
    if (ns.on && m) {
        if (core.empty()) core.assign(tg, tg + n_t * 6);
        std::vector<float> nrm(m * 3);
        plade_scale_summary qs;
        if (!scale_normals_packed(ctx, tg, n_t, kept.empty() ? nullptr : kept.data(), m, ns.radii, ns.scales, ns.mode, 6, true, nrm.data(), qs))
            return;
        for (size_t i = 0; i < m; ++i) memcpy(&core[6 * i + 3], &nrm[3 * i], 12);
        cp = core.data();
        std::string hist;
        for (int t = 0; t < ns.scales; ++t) hist += " " + std::to_string(qs.chosen_hist[t]);
        char b[280];
        snprintf(b, sizeof(b), "m3c2 normals: %llu of %llu core points fitted (scales%s; largest neighbourhood %u)",
                 (unsigned long long)qs.fitted, (unsigned long long)qs.queries, hist.c_str(), qs.max_count);
        con_out() << b << std::endl;
    }
    const DbscanSwitch &cl = m3c2_clusters_switch();
    std::vector<uint8_t> sig(cl.on ? m : 0);
    plade_m3c2_summary s;
    if (!m3c2_packed(ctx, T16, cp, m, tg, n_t, sr, n_s, sw.radius, sw.depth, sw.min_points, sw.reg_error, nullptr, s, cl.on ? sig.data() : nullptr))
        return;
    char b[280];
    snprintf(b, sizeof(b), "m3c2: %llu of %llu core points valid, %llu significant (mean %.6g, rms %.6g, max %.6g)", (unsigned long long)s.valid,
             (unsigned long long)s.m, (unsigned long long)s.significant, s.mean, s.rms, s.max);
    con_out() << b << std::endl;
    if (!cl.on) return;
    std::vector<float> change;                   // the positions of the significant core points, in core order
    for (size_t i = 0; i < m; ++i)
        if (sig[i]) change.insert(change.end(), cp + 6 * i, cp + 6 * i + 3);
    plade_dbscan_summary d;
    memset(&d, 0, sizeof(d));
    if (!change.empty() && !dbscan_packed(ctx, change.data(), change.size() / 3, 3, cl.radius, cl.min_points, cl.min_size, 0, nullptr, nullptr, d))
        return;
    snprintf(b, sizeof(b), "m3c2 clusters: %llu clusters of %llu significant core points (largest %u, noise %llu)",
             (unsigned long long)d.kept_clusters, (unsigned long long)(change.size() / 3), d.largest, (unsigned long long)d.noise);
    con_out() << b << std::endl;
}

// PLADE_FPFH_MATCH=<radius>[,<min_pairs>[,<max_ratio>]] (opt-in, absolute, in the clouds' units): both clouds of every pair -- registered
// or not -- are described with FPFH on the GPU (plade_cloud_fpfh; min_pairs 5 when not given) and matched in feature space
// (plade_match_features: mutual nearest neighbours, the ratio test when max_ratio is given), and one console line reports the
// described counts, the number of correspondences and, when the pair registered, the share of them with |T s - t| < radius under the
// final transformation (a host loop in fp64).  The pair is described as it was registered (after the target / source switch).  A
// value that does not parse (radius not positive and finite, min_pairs not an integer >= 1, max_ratio negative or not finite,
// anything behind them) prints one warning and does nothing; unset, nothing changes.
const FpfhSwitch &fpfh_switch() {
    static const FpfhSwitch sw = latched(cli_switches::parse_fpfh_match(getenv("PLADE_FPFH_MATCH")));
    return sw;
}
// FPFH of a packed cloud (x y z nx ny nz rows): desc receives n x 33 floats.  false: a message has been printed
bool fpfh_packed(plade_ctx *ctx, const float *rows, size_t n, double radius, int min_pairs, float *desc, plade_fpfh_summary &s) {
    plade_fpfh_params prm;
    plade_fpfh_default_params(&prm);
    prm.radius = radius; prm.min_pairs = min_pairs;
    trace("fpfh: describing");
    const int rc = plade_cloud_fpfh(ctx, rows, (uint32_t)n, &prm, desc, nullptr, nullptr, nullptr, nullptr, &s);
    trace("fpfh: done");
    if (rc != PLADE_OK) {
        con_err() << "cloud description failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    return true;
}
// the correspondences (source, target) of two descriptor tables.  false: a message has been printed
bool match_packed(plade_ctx *ctx, const float *src, size_t ns, const float *tgt, size_t nt, bool mutual, float max_ratio,
                  std::vector<int32_t> &corr) {
    plade_feature_match_params prm;
    plade_feature_match_default_params(&prm);
    prm.mutual = mutual ? 1 : 0; prm.max_ratio = max_ratio;
    std::vector<int32_t> c(2 * ns);
    uint64_t m = 0;
    const int rc = plade_match_features(ctx, src, (uint32_t)ns, tgt, (uint32_t)nt, &prm, nullptr, nullptr, nullptr, c.data(), ns, &m);
    if (rc != PLADE_OK) {
        con_err() << "feature match failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    c.resize(2 * (size_t)m);
    corr.swap(c);
    return true;
}
// T16: the final transformation of a pair that registered, or nullptr
void fpfh_line(plade_ctx *ctx, const float *T16, const float *tg, size_t n_t, const float *sr, size_t n_s) {
    const FpfhSwitch &sw = fpfh_switch();
    if (!sw.on || !ctx) return;
    std::vector<float> ft(33 * n_t), fs(33 * n_s);
    std::vector<int32_t> corr;
    plade_fpfh_summary st, ss;
    if (!fpfh_packed(ctx, tg, n_t, sw.radius, sw.min_pairs, ft.data(), st) || !fpfh_packed(ctx, sr, n_s, sw.radius, sw.min_pairs, fs.data(), ss) ||
        !match_packed(ctx, fs.data(), n_s, ft.data(), n_t, true, sw.max_ratio, corr))
        return;
    const size_t m = corr.size() / 2;
    char b[320];
    int len = snprintf(b, sizeof(b), "fpfh: %llu of %llu target and %llu of %llu source points described, %llu mutual correspondences",
                       (unsigned long long)st.described, (unsigned long long)st.n, (unsigned long long)ss.described, (unsigned long long)ss.n,
                       (unsigned long long)m);
    if (T16) {
        size_t close = 0;
        for (size_t k = 0; k < m; ++k) {
            const float *p = sr + 6 * (size_t)corr[2 * k], *q = tg + 6 * (size_t)corr[2 * k + 1];
            double d2 = 0.0;
            for (int r = 0; r < 3; ++r) {
                const double v = (((double)T16[4 * r] * p[0] + (double)T16[4 * r + 1] * p[1]) + (double)T16[4 * r + 2] * p[2]) + (double)T16[4 * r + 3] - q[r];
                d2 += v * v;
            }
            if (std::sqrt(d2) < sw.radius) ++close;
        }
        snprintf(b + len, sizeof(b) - (size_t)len, ", %.4f of them within the radius", m ? (double)close / (double)m : 0.0);
    }
    con_out() << b << std::endl;
}

// PLADE_FEATURE_REGISTER=<radius>,<inlier_dist>[,<min_inliers>[,<hypotheses>]] (opt-in, absolute, in the clouds' units): a pair whose
// plane registration failed goes through plade_register_features -- FPFH of both clouds at <radius>, their mutual match and the
// RANSAC pose over the correspondences at <inlier_dist> (min_inliers 3 and 65 536 hypotheses when not given).  On success one console
// line reports the inliers, and the pair is from there on a registered pair: its matrix is written and PLADE_REFINE_ICP / GICP /
// EVALUATE / M3C2 / FPFH_MATCH / MERGE apply.  On failure the failure path runs as before, plus one line saying that the features
// did not register the pair either.  A value that does not parse (radius or inlier_dist not positive and finite, min_inliers not an
// integer >= 3, hypotheses not in 1 .. 2^24, anything behind them) prints one warning and does nothing; unset, nothing changes.
const FeatureRegisterSwitch &feature_register_switch() {
    static const FeatureRegisterSwitch sw = latched(cli_switches::parse_feature_register(getenv("PLADE_FEATURE_REGISTER")));
    return sw;
}
// the library's defaults with the values the C++ API and the switches carry
plade_corr_pose_params pose_params(double inlier_dist, int min_inliers, int hypotheses, uint64_t seed) {
    plade_corr_pose_params pp;
    plade_corr_pose_default_params(&pp);
    pp.inlier_dist = inlier_dist; pp.min_inliers = min_inliers; pp.hypotheses = hypotheses; pp.seed = seed;
    return pp;
}
plade_iss_params iss_params(double salient_radius, double non_max_radius, int min_neighbours) {
    plade_iss_params ip;
    plade_iss_default_params(&ip);
    ip.salient_radius = salient_radius; ip.non_max_radius = non_max_radius; ip.min_neighbours = min_neighbours;
    return ip;
}
// FPFH, match and pose of a packed pair in one call.  rc: the library's status (PLADE_EFAIL: the pose failed, T16 = identity)
int register_features_packed(plade_ctx *ctx, float *T16, const float *tg, size_t n_t, const float *sr, size_t n_s, double radius,
                             int min_pairs, double inlier_dist, int min_inliers, int hypotheses, uint64_t seed,
                             plade_corr_pose_result &res, std::vector<int32_t> *corr, uint64_t &m) {
    plade_fpfh_params fp;
    plade_fpfh_default_params(&fp);
    fp.radius = radius; fp.min_pairs = min_pairs;
    const plade_corr_pose_params pp = pose_params(inlier_dist, min_inliers, hypotheses, seed);
    plade_fpfh_summary ss, st;
    if (corr) corr->resize(2 * n_s);
    trace("feature registration: describing, matching, estimating");
    const int rc = plade_register_features(ctx, tg, (uint32_t)n_t, sr, (uint32_t)n_s, &fp, nullptr, &pp, T16, &ss, &st, &res,
                                           corr ? corr->data() : nullptr, n_s, &m);
    trace("feature registration: done");
    if (corr) corr->resize(rc == PLADE_OK || rc == PLADE_EFAIL ? 2 * (size_t)m : 0);
    return rc;
}

// PLADE_FEATURE_KEYPOINTS=<salient_radius>[,<non_max_radius>[,<min_neighbours>]] (opt-in, absolute, in the clouds' units; it acts only
// together with PLADE_FEATURE_REGISTER): the pair whose plane registration failed goes through plade_register_keypoints instead of
// plade_register_features -- the ISS keypoints of the source (non_max_radius = salient_radius and min_neighbours 5 when not given)
// are what is matched against the target's descriptors -- and one more console line, in front of the feature registration's, reports
// the keypoints.  A value that does not parse (a radius not positive and finite, min_neighbours not an integer >= 1, anything behind
// them) prints one warning and is ignored; unset, nothing changes.
const KeypointSwitch &keypoint_switch() {
    static const KeypointSwitch sw = latched(cli_switches::parse_feature_keypoints(getenv("PLADE_FEATURE_KEYPOINTS")));
    return sw;
}
// ISS on the source, FPFH of both clouds, the keypoints' match and the pose of a packed pair in one call.  rc as above
int register_keypoints_packed(plade_ctx *ctx, float *T16, const float *tg, size_t n_t, const float *sr, size_t n_s, double salient_radius,
                              double non_max_radius, int min_neighbours, double radius, int min_pairs, double inlier_dist, int min_inliers,
                              int hypotheses, uint64_t seed, plade_iss_summary &ks, plade_corr_pose_result &res, std::vector<int32_t> *corr,
                              uint64_t &m) {
    const plade_iss_params ip = iss_params(salient_radius, non_max_radius, min_neighbours);
    plade_fpfh_params fp;
    plade_fpfh_default_params(&fp);
    fp.radius = radius; fp.min_pairs = min_pairs;
    const plade_corr_pose_params pp = pose_params(inlier_dist, min_inliers, hypotheses, seed);
    plade_fpfh_summary ss, st;
    if (corr) corr->resize(2 * n_s);
    trace("keypoint registration: detecting, describing, matching, estimating");
    const int rc = plade_register_keypoints(ctx, tg, (uint32_t)n_t, sr, (uint32_t)n_s, &ip, &fp, nullptr, &pp, T16, &ks, &ss, &st, &res,
                                            corr ? corr->data() : nullptr, n_s, &m);
    trace("keypoint registration: done");
    if (corr) corr->resize(rc == PLADE_OK || rc == PLADE_EFAIL ? 2 * (size_t)m : 0);
    return rc;
}
// the second chance of a pair without planes; true: T16 holds the pose and the pair counts as registered
bool feature_register(plade_ctx *ctx, float *T16, const float *tg, size_t n_t, const float *sr, size_t n_s) {
    const FeatureRegisterSwitch &sw = feature_register_switch();
    const KeypointSwitch &kp = keypoint_switch();
    if (!sw.on || !ctx) return false;
    plade_corr_pose_result res;
    plade_iss_summary ks;
    uint64_t m = 0;
    const int rc = kp.on ? register_keypoints_packed(ctx, T16, tg, n_t, sr, n_s, kp.salient_radius, kp.non_max_radius, kp.min_neighbours,
                                                     sw.radius, 5, sw.inlier_dist, sw.min_inliers, sw.hypotheses, 0, ks, res, nullptr, m)
                         : register_features_packed(ctx, T16, tg, n_t, sr, n_s, sw.radius, 5, sw.inlier_dist, sw.min_inliers, sw.hypotheses,
                                                    0, res, nullptr, m);
    if (rc != PLADE_OK) {
        con_err() << "feature registration failed as well: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    char b[200];
    if (kp.on) {
        snprintf(b, sizeof(b), "keypoints: %llu of %llu source points", (unsigned long long)ks.keypoints, (unsigned long long)ks.n);
        con_out() << b << std::endl;
    }
    snprintf(b, sizeof(b), "feature registration: %u of %llu correspondences, rmse %.6g", res.inliers, (unsigned long long)m, res.rmse);
    con_out() << b << std::endl;
    return true;
}

// PLADE_REMOVE_OUTLIERS=<k>[,<alpha>] (opt-in, 0 / unset = off): both clouds of a pair pass the statistical outlier filter on the
// GPU (plade_filter_outliers: k nearest neighbours, threshold mu + alpha sigma, alpha 1 when not given) after they are read and
// before PLADE_ESTIMATE_NORMALS; one console line per cloud.  A value that does not parse (k not an integer in [1, 64], alpha
// negative or not finite, anything behind them) prints one warning and filters nothing; unset, nothing changes.
const OutlierSwitch &remove_outliers_switch() {
    static const OutlierSwitch sw = latched(cli_switches::parse_remove_outliers(getenv("PLADE_REMOVE_OUTLIERS")));
    return sw;
}
// the rows of an x y z nx ny nz array that pass the filter, in place (the normal columns, NaN included, keep their bits)
bool filter_packed(plade_ctx *ctx, std::vector<float> &buf, int k, double alpha, plade_outlier_summary &s) {
    plade_outlier_params prm;
    plade_outlier_default_params(&prm);
    prm.k = k; prm.alpha = alpha;
    const size_t n = buf.size() / 6;
    trace("outliers: filtering");
    // (in place: the upload of the rows precedes the read-back of the kept ones on the context's stream)
    const int rc = plade_filter_outliers(ctx, buf.data(), (uint32_t)n, 6, &prm, nullptr, nullptr, buf.data(), nullptr, nullptr, &s);
    trace("outliers: done");
    if (rc != PLADE_OK) {
        con_err() << "outlier removal failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    buf.resize((size_t)s.kept * 6);
    return true;
}
bool remove_outliers_in_place(std::vector<float> &buf) {
    const OutlierSwitch &sw = remove_outliers_switch();
    if (!sw.k || buf.empty()) return true;
    plade_ctx *ctx = context();
    if (!ctx) return false;
    plade_outlier_summary s;
    if (!filter_packed(ctx, buf, sw.k, sw.alpha, s)) return false;
    char b[200];
    snprintf(b, sizeof(b), "outlier removal: kept %llu of %llu points (threshold %.6g)", (unsigned long long)s.kept,
             (unsigned long long)s.n, s.threshold);
    con_out() << b << std::endl;
    return true;
}

// PLADE_KEEP_COMPONENTS=<radius>[,<min_size>[,<keep_largest>]] (opt-in, 0 / unset = off; the radius absolute, in the clouds' units):
// both clouds of a pair keep only the connected components of the graph "closer than radius" with at least min_size points
// (1 when not given), with keep_largest = m > 0 only the m largest of them (plade_label_components), after PLADE_REMOVE_OUTLIERS and
// before PLADE_ESTIMATE_NORMALS; one console line per cloud.  A value that does not parse (radius negative or not finite, min_size
// not an integer >= 1, keep_largest not an integer >= 0, anything behind them) prints one warning and filters nothing; unset,
// nothing changes.
const ComponentSwitch &keep_components_switch() {
    static const ComponentSwitch sw = latched(cli_switches::parse_keep_components(getenv("PLADE_KEEP_COMPONENTS")));
    return sw;
}
// the rows of an x y z nx ny nz array whose component is kept, in place (the normal columns, NaN included, keep their bits)
bool components_packed(plade_ctx *ctx, std::vector<float> &buf, double radius, int min_size, int max_size, int keep_largest,
                       plade_component_summary &s) {
    plade_component_params prm;
    plade_component_default_params(&prm);
    prm.radius = radius; prm.min_size = min_size; prm.max_size = max_size; prm.keep_largest = keep_largest;
    const size_t n = buf.size() / 6;
    trace("components: labelling");
    // (in place: the upload of the rows precedes the read-back of the kept ones on the context's stream)
    const int rc = plade_label_components(ctx, buf.data(), (uint32_t)n, 6, &prm, nullptr, nullptr, nullptr, nullptr, buf.data(), &s);
    trace("components: done");
    if (rc != PLADE_OK) {
        con_err() << "component filter failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    buf.resize((size_t)s.kept * 6);
    return true;
}
bool keep_components_in_place(std::vector<float> &buf) {
    const ComponentSwitch &sw = keep_components_switch();
    if (!(sw.radius > 0.0) || buf.empty()) return true;
    plade_ctx *ctx = context();
    if (!ctx) return false;
    plade_component_summary s;
    if (!components_packed(ctx, buf, sw.radius, sw.min_size, 0, sw.keep_largest, s)) return false;
    char b[240];
    snprintf(b, sizeof(b), "component filter: kept %llu of %llu points in %llu of %llu components (largest %u)", (unsigned long long)s.kept,
             (unsigned long long)s.n, (unsigned long long)s.kept_components, (unsigned long long)s.components, s.largest);
    con_out() << b << std::endl;
    return true;
}

// PLADE_SMOOTH=<radius>[,<min_neighbours>] (opt-in, 0 / unset = off; the radius absolute, in the clouds' units): both clouds of a
// pair are smoothed by the moving-least-squares plane projection on the GPU (plade_smooth_cloud; min_neighbours 6 when not given)
// after PLADE_REMOVE_OUTLIERS and PLADE_KEEP_COMPONENTS and before PLADE_ESTIMATE_NORMALS: the positions move, the normal columns
// keep their bits (a file without normals gets the k-NN normals of the smoothed positions); one console line per cloud.  A value
// that does not parse (radius negative, not finite or so small that its fp32 square is below FLT_MIN, min_neighbours not an
// integer >= 3, anything behind them) prints one warning and smooths nothing; unset, nothing changes.
const SmoothSwitch &smooth_switch() {
    static const SmoothSwitch sw = latched(cli_switches::parse_smooth(getenv("PLADE_SMOOTH")));
    return sw;
}
// the x y z columns of an x y z nx ny nz array smoothed in place; nrm: the fit's normals (n x 3) when wanted
bool smooth_packed(plade_ctx *ctx, std::vector<float> &buf, double radius, int min_neighbours, std::vector<float> *nrm, plade_smooth_summary &s) {
    plade_smooth_params prm;
    plade_smooth_default_params(&prm);
    prm.radius = radius; prm.min_neighbours = min_neighbours;
    const size_t n = buf.size() / 6;
    std::vector<float> xyz(n * 3);
    if (nrm) nrm->resize(n * 3);
    trace("smooth: fitting");
    const int rc = plade_smooth_cloud(ctx, buf.data(), (uint32_t)n, 6, &prm, xyz.data(), nrm ? nrm->data() : nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, &s);
    trace("smooth: done");
    if (rc != PLADE_OK) {
        con_err() << "smoothing failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    for (size_t i = 0; i < n; ++i) memcpy(&buf[6 * i], &xyz[3 * i], 12);
    return true;
}
bool smooth_in_place(std::vector<float> &buf) {
    const SmoothSwitch &sw = smooth_switch();
    if (!(sw.radius > 0.0) || buf.empty()) return true;
    plade_ctx *ctx = context();
    if (!ctx) return false;
    plade_smooth_summary s;
    if (!smooth_packed(ctx, buf, sw.radius, sw.min_neighbours, nullptr, s)) return false;
    char b[240];
    snprintf(b, sizeof(b), "smoothing: fitted %llu of %llu points (rms displacement %.6g, max %.6g)", (unsigned long long)s.fitted,
             (unsigned long long)s.n, s.rms, s.max);
    con_out() << b << std::endl;
    return true;
}

// PLADE_MERGE=<leaf> (opt-in, absolute, in the clouds' units; 0 = plain concatenation): every pair that registered is merged on
// the GPU (plade_merge_clouds: the target as it is, the source under the pair's final transformation -- after ICP when that is
// on) into <result file>.merged.ply (one pair) or <result file>.<pair index>.merged.ply (a list), in the target file's frame; one
// console line per pair.  The CLI names the result file (plade_set_thread_merge_output).  A value that is not a finite number
// >= 0 prints one warning and merges nothing; unset, nothing changes.
float merge_leaf() {   // < 0: off
    static const float leaf = latched(cli_switches::parse_merge(getenv("PLADE_MERGE")));
    return leaf;
}
thread_local std::string g_merge_result;   // the result file whose name the merged clouds take; empty: no merge
thread_local long g_merge_first = -1;      // index in the list of the first pair of the running call; < 0: a single pair
// k packed clouds under their row-major 4 x 4 transforms (T16: k x 16 or nullptr) -> rows (sum n_c x 6, cut to the output)
bool merge_packed(plade_ctx *ctx, uint32_t k, const float *const *clouds, const uint32_t *n, const float *T16, float leaf,
                  std::vector<float> &rows, plade_merge_summary &s) {
    size_t total = 0;
    for (uint32_t c = 0; c < k; ++c) total += n[c];
    rows.resize(total * 6);
    trace("merge: merging");
    const int rc = plade_merge_clouds(ctx, k, clouds, n, T16, leaf, rows.data(), nullptr, nullptr, &s);
    trace("merge: done");
    if (rc != PLADE_OK) {
        con_err() << "warning: merge failed (" << plade_last_error(ctx) << ")" << std::endl;
        return false;
    }
    rows.resize((size_t)s.n_out * 6);
    return true;
}
// the pair as the FILES name it: T = source file -> target file
void merge_pair(plade_ctx *ctx, const Eigen::Matrix<float, 4, 4> &T, const float *tg, size_t n_t, const float *sr, size_t n_s, long pair) {
    const float leaf = merge_leaf();
    if (leaf < 0.f || g_merge_result.empty() || !ctx) return;
    float T16[32];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { T16[4 * r + c] = r == c ? 1.f : 0.f; T16[16 + 4 * r + c] = T(r, c); }
    const float *clouds[2] = {tg, sr};
    const uint32_t n[2] = {(uint32_t)n_t, (uint32_t)n_s};
    std::vector<float> rows;
    plade_merge_summary s;
    if (!merge_packed(ctx, 2, clouds, n, T16, leaf, rows, s)) return;
    const std::string path = g_merge_result + (pair < 0 ? std::string() : "." + std::to_string(pair)) + ".merged.ply";
    if (!plade::write_ply_pos_nrm(path, rows.data(), (size_t)s.n_out)) {
        con_err() << "warning: writing " << path << " failed" << std::endl;
        return;
    }
    char b[200];
    snprintf(b, sizeof(b), "merge: %llu of %llu points kept, %llu voxels seen by both clouds", (unsigned long long)s.n_out,
             (unsigned long long)s.n_in, (unsigned long long)s.n_shared);
    con_out() << b << std::endl;
}

std::string extension(const std::string &file_name) {  // util.cpp:525-531
    std::string::size_type dot = file_name.find_last_of('.');
    std::string::size_type slash = file_name.find_last_of("/\\");
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return std::string("");
    return std::string(file_name.begin() + dot + 1, file_name.end());
}

}  // namespace

namespace {
bool estimate_in_place(const std::string &file_name, std::vector<float> &buf) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    const int k = estimate_normals_k();
    const float view[3] = {0.f, 0.f, 0.f};
    const size_t n = buf.size() / 6;
    trace("normals: estimating");
    // (in place: the upload of the coordinates precedes the read-back of the result on the context's stream)
    if (plade_estimate_normals(ctx, buf.data(), (uint32_t)n, 6, k, view, buf.data(), nullptr, nullptr) != PLADE_OK) {
        con_err() << "estimating normals failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    con_out() << "no normals in " << file_name << ": estimated from " << k << " nearest neighbours" << std::endl;
    return true;
}
}  // namespace

void plade_cli_trace(const char *what) { trace(what); }
void plade_select_device(int device) { g_device = device; }
int plade_gpu_count() { return plade_device_count(); }

void plade_set_thread_console(std::ostream *out, std::ostream *err) { g_out = out; g_err = err; }
void plade_set_thread_merge_output(const std::string &result_file, long first_pair) { g_merge_result = result_file; g_merge_first = first_pair; }

void plade_release_thread_context() {
    for (PinnedVec &p : g_pins) p.release();     // before the arrays themselves go with the thread
    if (g_ctx) { plade_ctx_destroy(g_ctx); g_ctx = nullptr; g_ctx_device = -1; }
}

std::vector<PLANE> PlaneExtraction::detect(const pcl::PointCloud<pcl::PointNormal> &cloud, unsigned int min_support,
                                           float dist_thresh, float bitmap_reso, float normal_thresh, float overlook_prob) {
    std::vector<PLANE> out;
    if (cloud.size() < 3) {  // plane_extraction.cpp:181-184
        con_err() << "point set has less than 3 points" << std::endl;
        return out;
    }
    plade_ctx *ctx = context();
    if (!ctx) return out;
    std::vector<float> a = flatten(cloud);
    const uint32_t max_planes = 4096;
    std::vector<float> coef(4 * max_planes);
    std::vector<int32_t> off(max_planes + 1), idx(cloud.size());
    uint32_t P = 0;
    int rc = plade_extract_planes(ctx, a.data(), (uint32_t)cloud.size(), min_support, dist_thresh, bitmap_reso, normal_thresh,
                                  overlook_prob, coef.data(), off.data(), idx.data(), max_planes, &P);
    if (rc != PLADE_OK) { con_err() << "plane extraction failed: " << plade_last_error(ctx) << std::endl; return out; }
    for (uint32_t i = 0; i < P; ++i) {
        PLANE pl(idx.begin() + off[i], idx.begin() + off[i + 1]);
        pl.normal = Eigen::Vector3f(coef[4 * i], coef[4 * i + 1], coef[4 * i + 2]);
        pl.d = coef[4 * i + 3];
        out.push_back(pl);
    }
    return out;
}

// plade.h:74-79 / plade.cpp:31-580
bool registration(Eigen::Matrix<float, 4, 4> &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                  pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud, const std::vector<PLANE> &target_planes,
                  const std::vector<PLANE> &source_planes) {
    con_out() << "#point in target point cloud: " << target_cloud->size() << std::endl;
    con_out() << "#point in source point cloud: " << source_cloud->size() << std::endl;
    con_out() << "#planes in target point cloud: " << target_planes.size() << std::endl;
    con_out() << "#planes in source point cloud: " << source_planes.size() << std::endl;
    plade_ctx *ctx = context();
    if (!ctx) return false;
    std::vector<float> tg = flatten(*target_cloud), sr = flatten(*source_cloud), tc, sc;
    std::vector<int32_t> to, ti, so, si;
    pack_planes(target_planes, tc, to, ti);
    pack_planes(source_planes, sc, so, si);
    float T16[16];
    Watch w;
    con_out() << "registration..." << std::endl;
    int rc = plade_registration_planes(ctx, tg.data(), (uint32_t)target_cloud->size(), sr.data(), (uint32_t)source_cloud->size(),
                                       tc.data(), to.data(), ti.data(), (uint32_t)target_planes.size(), sc.data(), so.data(),
                                       si.data(), (uint32_t)source_planes.size(), T16);
    if (rc != PLADE_OK) {
        con_err() << (rc == PLADE_EFAIL ? "registration failed: no matched result found" : plade_last_error(ctx)) << std::endl;
        return false;
    }
    to_matrix(T16, transformation);
    con_out() << "done. time: " << w.str() << std::endl;
    return true;
}

// plade.h:91-96 / plade.cpp:583-599
bool registration(Eigen::Matrix<float, 4, 4> &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                  pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud, int ransac_min_support_target,
                  int ransac_min_support_source) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    std::vector<float> tg = flatten(*target_cloud), sr = flatten(*source_cloud);
    float T16[16];
    Watch w;
    con_out() << "extracting planes and registering...\n";
    int rc = plade_registration_minsupport(ctx, tg.data(), (uint32_t)target_cloud->size(), sr.data(), (uint32_t)source_cloud->size(),
                                           ransac_min_support_target, ransac_min_support_source, T16);
    if (rc != PLADE_OK) {
        con_err() << (rc == PLADE_EFAIL ? plade_last_error(ctx) : plade_last_error(ctx)) << std::endl;
        return false;
    }
    to_matrix(T16, transformation);
    con_out() << "done. time: " << w.str() << std::endl;
    return true;
}

namespace {

// What follows a pair's registration, after its caller has printed the library's error or "done. time:" -- the single-pair path
// and the group share it.  A pair that did not register gets its second chance (PLADE_FEATURE_REGISTER: a pair without planes);
// a registered pair the selected refinement and the evaluation, M3C2 and FPFH lines.  false: the pair stays unregistered
bool pair_tail(plade_ctx *ctx, bool registered, float *T16, const float *tg, size_t n_t, const float *sr, size_t n_s) {
    if (!registered && !feature_register(ctx, T16, tg, n_t, sr, n_s)) {
        fpfh_line(ctx, nullptr, tg, n_t, sr, n_s);
        return false;
    }
    refine_selected(ctx, T16, tg, n_t, sr, n_s);
    evaluate_line(ctx, T16, tg, n_t, sr, n_s);
    m3c2_line(ctx, T16, tg, n_t, sr, n_s);
    fpfh_line(ctx, T16, tg, n_t, sr, n_s);
    return true;
}

// body of registration(T, target, source) (plade.cpp:638-662) on packed x y z nx ny nz arrays
bool register_packed(Eigen::Matrix<float, 4, 4> &transformation, const float *tg, size_t n_t, const float *sr, size_t n_s) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    con_out() << "extracting planes for both point clouds...\n";
    float T16[16];
    Watch w;
    int rc = plade_registration(ctx, tg, (uint32_t)n_t, sr, (uint32_t)n_s, T16);
    if (rc != PLADE_OK) con_err() << plade_last_error(ctx) << std::endl;
    else con_out() << "done. time: " << w.str() << std::endl;
    if (!pair_tail(ctx, rc == PLADE_OK, T16, tg, n_t, sr, n_s)) return false;
    to_matrix(T16, transformation);
    return true;
}

// what every cloud goes through once its file is read: the filters that are switched on, in their order, then the normals of a
// file that had none (estimate), then the consistent orientation and the subsample when they are switched on.  false: a message has
// been printed
bool prepare_loaded(const std::string &file_name, std::vector<float> &buf, bool estimate) {
    if (!remove_outliers_in_place(buf) || !keep_components_in_place(buf) || !dbscan_in_place(buf) || !smooth_in_place(buf)) return false;
    if (estimate && !buf.empty() && !estimate_in_place(file_name, buf)) return false;
    return orient_in_place(buf) && subsample_in_place(buf);
}

// a PLY file straight into a packed array (no pcl::PointCloud in between: at GPU speeds the 48 B/point
// intermediate and its page faults cost several registrations); `buf` is reused from call to call
bool load_packed(const std::string &file_name, std::vector<float> &buf) {
    std::string err;
    std::vector<std::string> warnings;
    bool estimate = false;
    if (!read_ply_cloud(file_name, buf, err, &warnings, nullptr, &estimate)) {
        if (!err.empty()) con_err() << err << std::endl;
        return false;
    }
    for (auto &w : warnings) con_out() << w << std::endl;
    return prepare_loaded(file_name, buf, estimate) && !buf.empty();
}

}  // namespace

// plade.h:58-61 / plade.cpp:638-662
bool registration(Eigen::Matrix<float, 4, 4> &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                  pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud) {
    std::vector<float> tg = flatten(*target_cloud), sr = flatten(*source_cloud);
    return register_packed(transformation, tg.data(), target_cloud->size(), sr.data(), source_cloud->size());
}

// plade.h:44-47 / plade.cpp:665-706
bool registration(Eigen::Matrix<float, 4, 4> &transformation, const std::string &target_cloud_file,
                  const std::string &source_cloud_file) {
    con_out() << "target file: " << target_cloud_file << std::endl;
    con_out() << "source file: " << source_cloud_file << std::endl;
    if (extension(target_cloud_file) != "ply" || extension(source_cloud_file) != "ply") {
        con_err() << "only PLY format is accepted" << std::endl;
        return false;
    }
    thread_local std::vector<float> target_buf, source_buf;   // one pair of staging arrays per worker thread
    trace("pair: reading the two files");
    if (!load_packed(target_cloud_file, target_buf)) {
        con_err() << "loading target point cloud failed" << std::endl;
        return false;
    }
    if (!load_packed(source_cloud_file, source_buf)) {
        con_err() << "loading source point cloud failed" << std::endl;
        return false;
    }
    const float *tg = target_buf.data(), *sr = source_buf.data();
    size_t n_t = target_buf.size() / 6, n_s = source_buf.size() / 6;
    bool switched = false;
    if (n_s >= n_t * 1.2f) {
        std::swap(tg, sr);
        std::swap(n_t, n_s);
        switched = true;
        con_out() << "---->>> ATTENTION: target and source have been switched for efficiency <<<----" << std::endl;
    }
    transformation.setIdentity();
    trace("pair: files read");
    bool status = register_packed(transformation, tg, n_t, sr, n_s);
    trace("pair: registered");
    if (!status) {
        con_err() << "registration failed" << std::endl;
        return false;
    }
    if (switched) transformation = transformation.inverse();
    if (merge_leaf() >= 0.f)
        merge_pair(context(), transformation, target_buf.data(), target_buf.size() / 6, source_buf.data(), source_buf.size() / 6, g_merge_first);
    return true;
}

// Batch extension: see plade.h.  The per-pair part of the file overload above (messages, extension check, loading, the
// target/source switch, plade.cpp:665-706) runs pair by pair; the pairs that got that far are registered as one group.
void registration_group(size_t count, Eigen::Matrix<float, 4, 4> *transformations, const std::string *target_cloud_files,
                        const std::string *source_cloud_files, bool *ok, std::ostream *const *out, std::ostream *const *err) {
    constexpr size_t GMAX = PLADE_GROUP_MAX;
    static_assert(GMAX == registration_group_max, "plade.h states the group limit of include/plade_hip.h");
    if (count > GMAX) count = GMAX;
    thread_local std::vector<float> bufs[2 * GMAX];   // staging arrays of this worker thread, reused from group to group
    struct Item { size_t pair; const float *tg, *sr; size_t n_t, n_s; bool switched; };
    std::vector<Item> items;
    // The files of the group are read side by side (a 1M-point binary PLY is ~10 ms of parsing and copying; sixteen of them one
    // after the other would take longer than the group's registration); what the loads have to say is kept and printed below,
    // pair by pair, where the sequential run prints it.
    struct Loaded { bool tried = false, ok = false, estimate = false; std::string err; std::vector<std::string> warnings; };
    Loaded loaded[2 * GMAX];
    {
        std::vector<float> *const b = bufs;
        std::vector<std::thread> readers;
        for (size_t i = 0; i < count; ++i) {
            if (extension(target_cloud_files[i]) != "ply" || extension(source_cloud_files[i]) != "ply") continue;
            for (int side = 0; side < 2; ++side) {
                const std::string *file = side ? &source_cloud_files[i] : &target_cloud_files[i];
                Loaded *l = &loaded[2 * i + side];
                std::vector<float> *buf = &b[2 * i + side];
                l->tried = true;
                // (an array that has to grow moves: its page-locked registration is released BEFORE the old block is freed -- a
                //  registration left on freed memory fails the next one of whatever block takes the address; advisor r5)
                PinnedVec *pin = &g_pins[2 * i + side];
                readers.emplace_back([file, l, buf, pin]() {
                    const std::function<void()> before_grow = [pin]() { pin->release(); };
                    l->ok = read_ply_cloud(*file, *buf, l->err, &l->warnings, &before_grow, &l->estimate) && !buf->empty();
                });
            }
        }
        // the worker's GPU context (HIP start-up on first use, streams, the first work areas) is set up while the files load
        trace("group: reading");
        (void)context();
        for (auto &t : readers) t.join();
        trace("group: files read");
    }
    auto report = [&](const Loaded &l, const std::string &file, std::vector<float> &buf) {   // load_packed's messages
        if (!l.ok && !l.err.empty()) con_err() << l.err << std::endl;
        if (l.ok || l.err.empty()) for (auto &w : l.warnings) con_out() << w << std::endl;
        return l.ok && prepare_loaded(file, buf, l.estimate) && !buf.empty();
    };
    for (size_t i = 0; i < count; ++i) {
        ok[i] = false;
        transformations[i].setIdentity();
        plade_set_thread_console(out ? out[i] : nullptr, err ? err[i] : nullptr);
        con_out() << "target file: " << target_cloud_files[i] << std::endl;
        con_out() << "source file: " << source_cloud_files[i] << std::endl;
        if (extension(target_cloud_files[i]) != "ply" || extension(source_cloud_files[i]) != "ply") {
            con_err() << "only PLY format is accepted" << std::endl;
            continue;
        }
        if (!report(loaded[2 * i], target_cloud_files[i], bufs[2 * i])) { con_err() << "loading target point cloud failed" << std::endl; continue; }
        if (!report(loaded[2 * i + 1], source_cloud_files[i], bufs[2 * i + 1])) { con_err() << "loading source point cloud failed" << std::endl; continue; }
        Item it{i, bufs[2 * i].data(), bufs[2 * i + 1].data(), bufs[2 * i].size() / 6, bufs[2 * i + 1].size() / 6, false};
        if (it.n_s >= it.n_t * 1.2f) {
            std::swap(it.tg, it.sr);
            std::swap(it.n_t, it.n_s);
            it.switched = true;
            con_out() << "---->>> ATTENTION: target and source have been switched for efficiency <<<----" << std::endl;
        }
        con_out() << "extracting planes for both point clouds...\n";
        items.push_back(it);
    }
    plade_set_thread_console(nullptr, nullptr);
    if (items.empty()) return;
    plade_ctx *ctx = context();
    for (size_t q = 0; q < 2 * GMAX; ++q) if (!bufs[q].empty()) g_pins[q].cover(ctx, bufs[q]);
    trace("group: staging arrays page-locked");
    const uint32_t k = (uint32_t)items.size();
    const float *tg[GMAX], *sr[GMAX];
    uint32_t n_t[GMAX], n_s[GMAX];
    float T16[16 * GMAX];
    int32_t status[GMAX];
    for (uint32_t q = 0; q < k; ++q) { tg[q] = items[q].tg; sr[q] = items[q].sr; n_t[q] = (uint32_t)items[q].n_t; n_s[q] = (uint32_t)items[q].n_s; status[q] = PLADE_EDEVICE; }
    Watch w;
    int rc = ctx ? plade_registration_pairs(ctx, k, tg, n_t, sr, n_s, 0, nullptr, nullptr, nullptr, nullptr, T16, status) : PLADE_EDEVICE;
    trace("group: registered");
    for (uint32_t q = 0; q < k; ++q) {
        const Item &it = items[q];
        plade_set_thread_console(out ? out[it.pair] : nullptr, err ? err[it.pair] : nullptr);
        const bool registered = rc == PLADE_OK && status[q] == PLADE_OK;
        if (!registered) {
            const plade_ctx *pc = ctx ? (rc != PLADE_OK ? ctx : plade_pair_ctx(ctx, q)) : nullptr;
            if (pc) con_err() << plade_last_error(pc) << std::endl;
        } else con_out() << "done. time: " << w.str() << std::endl;
        if (!pair_tail(ctx, registered, T16 + 16 * q, it.tg, it.n_t, it.sr, it.n_s)) {
            con_err() << "registration failed" << std::endl;
            continue;
        }
        to_matrix(T16 + 16 * q, transformations[it.pair]);
        if (it.switched) transformations[it.pair] = transformations[it.pair].inverse();
        if (merge_leaf() >= 0.f)
            merge_pair(ctx, transformations[it.pair], bufs[2 * it.pair].data(), bufs[2 * it.pair].size() / 6, bufs[2 * it.pair + 1].data(),
                       bufs[2 * it.pair + 1].size() / 6, g_merge_first < 0 ? (long)it.pair : g_merge_first + (long)it.pair);
        ok[it.pair] = true;
    }
    plade_set_thread_console(nullptr, nullptr);
}

// fine alignment after registration(): see plade.h
bool refine_registration(Eigen::Matrix<float, 4, 4> &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                         pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    std::vector<float> tg = flatten(*target_cloud), sr = flatten(*source_cloud);
    float T16[16];
    to_T16(transformation, T16);
    if (!refine_packed(ctx, T16, tg.data(), target_cloud->size(), sr.data(), source_cloud->size())) return false;
    to_matrix(T16, transformation);
    return true;
}

// fine alignment by plane-to-plane ICP: see plade.h
bool refine_registration_gicp(Eigen::Matrix<float, 4, 4> &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                              pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud, double epsilon) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    std::vector<float> tg = flatten(*target_cloud), sr = flatten(*source_cloud);
    float T16[16];
    to_T16(transformation, T16);
    if (!refine_gicp_packed(ctx, T16, tg.data(), target_cloud->size(), sr.data(), source_cloud->size(), epsilon)) return false;
    to_matrix(T16, transformation);
    return true;
}

// registration quality: see plade.h
bool evaluate_registration(const Eigen::Matrix4f &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                           pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud, float max_dist, RegistrationQuality &out) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    std::vector<float> tg = flatten(*target_cloud), sr = flatten(*source_cloud);
    float T16[16];
    to_T16(transformation, T16);
    plade_distance_summary s;
    if (!evaluate_packed(ctx, T16, tg.data(), target_cloud->size(), sr.data(), source_cloud->size(), max_dist, s)) return false;
    out.n = s.n; out.count = s.count; out.plane_count = s.plane_count;
    out.fitness = s.fitness; out.rmse = s.rmse; out.mean = s.mean; out.max = s.max; out.plane_rmse = s.plane_rmse;
    return true;
}

// outlier removal: see plade.h
bool remove_outliers(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, pcl::PointCloud<pcl::PointNormal> &filtered, int k, double alpha,
                     OutlierRemoval *info) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    std::vector<float> buf = flatten(*cloud);
    plade_outlier_summary s;
    if (!filter_packed(ctx, buf, k, alpha, s)) return false;
    unflatten(buf.data(), (size_t)s.kept, filtered);
    if (info) { info->n = s.n; info->kept = s.kept; info->mu = s.mu; info->sigma = s.sigma; info->threshold = s.threshold; }
    return true;
}

// connected components: see plade.h
bool keep_components(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, pcl::PointCloud<pcl::PointNormal> &filtered, double radius, int min_size,
                     int max_size, int keep_largest, ComponentFilter *info) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    std::vector<float> buf = flatten(*cloud);
    plade_component_summary s;
    if (!components_packed(ctx, buf, radius, min_size, max_size, keep_largest, s)) return false;
    unflatten(buf.data(), (size_t)s.kept, filtered);
    if (info) { info->n = s.n; info->components = s.components; info->kept_components = s.kept_components; info->kept = s.kept; info->largest = s.largest; }
    return true;
}

// DBSCAN: see plade.h
bool cluster_cloud(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, pcl::PointCloud<pcl::PointNormal> &filtered, std::vector<int32_t> &labels,
                   double radius, int min_points, int min_size, int keep_largest, CloudClusters *info) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    std::vector<float> buf = flatten(*cloud);
    std::vector<int32_t> lab(cloud->size());
    plade_dbscan_summary s;
    if (!dbscan_packed(ctx, buf.data(), cloud->size(), 6, radius, min_points, min_size, keep_largest, lab.data(), buf.data(), s)) return false;
    unflatten(buf.data(), (size_t)s.kept, filtered);
    labels.swap(lab);
    if (info) {
        info->n = s.n; info->clusters = s.clusters; info->core = s.core; info->border = s.border; info->noise = s.noise;
        info->kept_clusters = s.kept_clusters; info->kept = s.kept; info->largest = s.largest;
    }
    return true;
}

// subsampling: see plade.h
bool subsample_cloud(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, pcl::PointCloud<pcl::PointNormal> &subset, double spacing, uint64_t seed,
                     CloudSubsample *info) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    std::vector<float> buf = flatten(*cloud);
    plade_subsample_summary s;
    if (!subsample_packed(ctx, buf.data(), cloud->size(), spacing, seed, buf.data(), s)) return false;
    unflatten(buf.data(), (size_t)s.kept, subset);
    if (info) { info->n = s.n; info->kept = s.kept; info->rounds = s.rounds; }
    return true;
}

// consistent normal orientation: see plade.h
bool orient_cloud_normals(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, pcl::PointCloud<pcl::PointNormal> &oriented, double radius, int mode,
                          bool inward, const float *reference, NormalOrientation *info) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    std::vector<float> buf = flatten(*cloud);
    plade_orient_summary s;
    if (!orient_packed(ctx, buf.data(), cloud->size(), radius, mode, inward ? 1 : 0, mode == 0 ? reference : nullptr,
                       mode == 0 ? nullptr : reference, s))
        return false;
    unflatten(buf.data(), (size_t)s.n, oriented);
    if (info) {
        info->n = s.n; info->unoriented = s.unoriented; info->components = s.components; info->flipped = s.flipped;
        info->tree_edges = s.tree_edges; info->rounds = s.rounds; info->tree_key_sum = s.tree_key_sum;
    }
    return true;
}

// smoothing: see plade.h
bool smooth_cloud(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, pcl::PointCloud<pcl::PointNormal> &smoothed, double radius, int min_neighbours,
                  bool use_fit_normals, CloudSmoothing *info) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    std::vector<float> buf = flatten(*cloud), nrm;
    plade_smooth_summary s;
    if (!smooth_packed(ctx, buf, radius, min_neighbours, use_fit_normals ? &nrm : nullptr, s)) return false;
    const size_t n = buf.size() / 6;
    smoothed.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const float *p = &buf[6 * i], *q = use_fit_normals ? &nrm[3 * i] : p + 3;
        smoothed.at(i) = pcl::PointNormal(p[0], p[1], p[2], q[0], q[1], q[2]);
    }
    if (info) { info->n = s.n; info->fitted = s.fitted; info->rms = s.rms; info->max = s.max; info->max_count = s.max_count; }
    return true;
}

// multi-scale normals: see plade.h
bool multiscale_normals(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, pcl::PointCloud<pcl::PointNormal> &with_normals,
                        const std::vector<double> &radii, int mode, int min_neighbours, bool orient_by_cloud_normals, CloudScales *info) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    if (!cloud) { con_err() << "multiscale_normals: null cloud" << std::endl; return false; }
    const std::vector<float> buf = flatten(*cloud);
    const size_t n = buf.size() / 6;
    std::vector<float> nrm(n * 3);
    plade_scale_summary s;
    // (more than eight radii: the count goes through as it is and the library refuses it)
    if (!scale_normals_packed(ctx, buf.data(), n, nullptr, n, radii.data(), (int)std::min<size_t>(radii.size(), 9), mode, min_neighbours,
                              orient_by_cloud_normals, nrm.data(), s))
        return false;
    with_normals.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const float *p = &buf[6 * i], *q = &nrm[3 * i];
        with_normals.at(i) = pcl::PointNormal(p[0], p[1], p[2], q[0], q[1], q[2]);
    }
    if (info) {
        info->queries = s.queries; info->fitted = s.fitted; info->max_count = s.max_count;
        for (int t = 0; t < 8; ++t) info->chosen_hist[t] = s.chosen_hist[t];
    }
    return true;
}

// change detection: see plade.h
bool compare_clouds(const Eigen::Matrix4f &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr reference_cloud,
                    pcl::PointCloud<pcl::PointNormal>::Ptr compared_cloud, double radius, double depth, std::vector<double> &distances,
                    CloudComparison *info, int min_points, double reg_error) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    if (!reference_cloud || !compared_cloud) { con_err() << "compare_clouds: null cloud" << std::endl; return false; }
    std::vector<float> ref = flatten(*reference_cloud), cmp = flatten(*compared_cloud);
    float T16[16];
    to_T16(transformation, T16);
    std::vector<double> dist(reference_cloud->size());
    plade_m3c2_summary s;
    if (!m3c2_packed(ctx, T16, ref.data(), reference_cloud->size(), ref.data(), reference_cloud->size(), cmp.data(), compared_cloud->size(),
                     radius, depth, min_points, reg_error, dist.data(), s))
        return false;
    distances.swap(dist);
    if (info) {
        info->m = s.m; info->valid = s.valid; info->significant = s.significant;
        info->mean = s.mean; info->rms = s.rms; info->max = s.max; info->max_count = s.max_count;
    }
    return true;
}

// point descriptors and their match: see plade.h
bool describe_cloud(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, double radius, std::vector<float> &features, CloudDescription *info,
                    int min_pairs) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    if (!cloud) { con_err() << "describe_cloud: null cloud" << std::endl; return false; }
    std::vector<float> rows = flatten(*cloud), desc(33 * cloud->size());
    plade_fpfh_summary s;
    if (!fpfh_packed(ctx, rows.data(), cloud->size(), radius, min_pairs, desc.data(), s)) return false;
    features.swap(desc);
    if (info) { info->n = s.n; info->described = s.described; info->mean_pairs = s.mean_pairs; info->max_pairs = s.max_pairs; }
    return true;
}
bool match_features(const std::vector<float> &source_features, const std::vector<float> &target_features,
                    std::vector<std::pair<int, int>> &correspondences, bool mutual, float max_ratio) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    if (source_features.size() % 33 || target_features.size() % 33) {
        con_err() << "match_features: a table of descriptors holds 33 floats per point" << std::endl;
        return false;
    }
    std::vector<int32_t> corr;
    if (!match_packed(ctx, source_features.data(), source_features.size() / 33, target_features.data(), target_features.size() / 33, mutual,
                      max_ratio, corr))
        return false;
    correspondences = to_pairs(corr);
    return true;
}

// the pose from correspondences, and FPFH -> match -> pose in one call: see plade.h
namespace {
void fill_pose_estimate(PoseEstimate *info, const plade_corr_pose_result &r, uint64_t m) {
    if (!info) return;
    info->correspondences = m;
    info->hypotheses = r.hypotheses; info->scored = r.scored; info->best_hypothesis = r.best_hypothesis; info->best_count = r.best_count;
    info->inliers = r.inliers; info->refinements = r.refinements; info->rmse = r.rmse; info->fitness = r.fitness;
}
}  // namespace
bool estimate_pose_from_correspondences(Eigen::Matrix4f &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                                        pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud,
                                        const std::vector<std::pair<int, int>> &correspondences, double inlier_dist, PoseEstimate *info,
                                        int min_inliers, int hypotheses, uint64_t seed) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    if (!target_cloud || !source_cloud) { con_err() << "estimate_pose_from_correspondences: null cloud" << std::endl; return false; }
    std::vector<float> tg = flatten(*target_cloud), sr = flatten(*source_cloud);
    std::vector<int32_t> corr(2 * correspondences.size());
    for (size_t k = 0; k < correspondences.size(); ++k) { corr[2 * k] = correspondences[k].first; corr[2 * k + 1] = correspondences[k].second; }
    const plade_corr_pose_params pp = pose_params(inlier_dist, min_inliers, hypotheses, seed);
    plade_corr_pose_result res;
    float T16[16];
    const int rc = plade_estimate_pose_corr(ctx, sr.data(), (uint32_t)source_cloud->size(), 6, tg.data(), (uint32_t)target_cloud->size(), 6,
                                            corr.data(), correspondences.size(), &pp, T16, nullptr, nullptr, nullptr, nullptr, nullptr, &res);
    if (rc != PLADE_OK) {
        con_err() << "pose estimation failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    to_matrix(T16, transformation);
    fill_pose_estimate(info, res, correspondences.size());
    return true;
}
bool register_by_features(Eigen::Matrix4f &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                          pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud, double radius, double inlier_dist, PoseEstimate *info,
                          std::vector<std::pair<int, int>> *correspondences, int min_inliers, int hypotheses, int min_pairs, uint64_t seed) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    if (!target_cloud || !source_cloud) { con_err() << "register_by_features: null cloud" << std::endl; return false; }
    std::vector<float> tg = flatten(*target_cloud), sr = flatten(*source_cloud);
    plade_corr_pose_result res;
    std::vector<int32_t> corr;
    uint64_t m = 0;
    float T16[16];
    const int rc = register_features_packed(ctx, T16, tg.data(), target_cloud->size(), sr.data(), source_cloud->size(), radius, min_pairs,
                                            inlier_dist, min_inliers, hypotheses, seed, res, correspondences ? &corr : nullptr, m);
    if (rc != PLADE_OK) {
        con_err() << "feature registration failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    to_matrix(T16, transformation);
    fill_pose_estimate(info, res, m);
    if (correspondences) *correspondences = to_pairs(corr);
    return true;
}

// keypoints, and the registration from the keypoints' features: see plade.h
bool detect_keypoints(pcl::PointCloud<pcl::PointNormal>::Ptr cloud, double salient_radius, std::vector<int> &keypoints,
                      KeypointDetection *info, double non_max_radius, int min_neighbours, double gamma21, double gamma32) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    if (!cloud) { con_err() << "detect_keypoints: null cloud" << std::endl; return false; }
    std::vector<float> rows = flatten(*cloud);
    plade_iss_params ip = iss_params(salient_radius, non_max_radius, min_neighbours);
    ip.gamma21 = gamma21; ip.gamma32 = gamma32;
    std::vector<uint32_t> index(cloud->size());
    uint64_t k = 0;
    plade_iss_summary s;
    trace("keypoints: detecting");
    const int rc = plade_cloud_keypoints_iss(ctx, rows.data(), (uint32_t)cloud->size(), 6, &ip, nullptr, index.data(), index.size(), &k,
                                             nullptr, nullptr, nullptr, nullptr, nullptr, &s);
    trace("keypoints: done");
    if (rc != PLADE_OK) {
        con_err() << "keypoint detection failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    std::vector<int> out(index.begin(), index.begin() + (size_t)k);
    keypoints.swap(out);
    if (info) { info->n = s.n; info->salient = s.salient; info->keypoints = s.keypoints; info->max_count = s.max_count; }
    return true;
}
bool register_by_keypoints(Eigen::Matrix4f &transformation, pcl::PointCloud<pcl::PointNormal>::Ptr target_cloud,
                           pcl::PointCloud<pcl::PointNormal>::Ptr source_cloud, double radius, double inlier_dist, double salient_radius,
                           PoseEstimate *info, KeypointDetection *detection, std::vector<std::pair<int, int>> *correspondences,
                           double non_max_radius, int min_neighbours, int min_inliers, int hypotheses, int min_pairs, uint64_t seed) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    if (!target_cloud || !source_cloud) { con_err() << "register_by_keypoints: null cloud" << std::endl; return false; }
    std::vector<float> tg = flatten(*target_cloud), sr = flatten(*source_cloud);
    plade_corr_pose_result res;
    plade_iss_summary ks;
    std::vector<int32_t> corr;
    uint64_t m = 0;
    float T16[16];
    const int rc = register_keypoints_packed(ctx, T16, tg.data(), target_cloud->size(), sr.data(), source_cloud->size(), salient_radius,
                                             non_max_radius, min_neighbours, radius, min_pairs, inlier_dist, min_inliers, hypotheses, seed, ks,
                                             res, correspondences ? &corr : nullptr, m);
    if (rc != PLADE_OK) {
        con_err() << "keypoint registration failed: " << plade_last_error(ctx) << std::endl;
        return false;
    }
    to_matrix(T16, transformation);
    fill_pose_estimate(info, res, m);
    if (detection) { detection->n = ks.n; detection->salient = ks.salient; detection->keypoints = ks.keypoints; detection->max_count = ks.max_count; }
    if (correspondences) *correspondences = to_pairs(corr);
    return true;
}

// merging registered clouds: see plade.h
bool merge_clouds(const std::vector<pcl::PointCloud<pcl::PointNormal>::Ptr> &clouds, const std::vector<Eigen::Matrix4f> &transformations,
                  float leaf, pcl::PointCloud<pcl::PointNormal> &merged, CloudMerge *info) {
    plade_ctx *ctx = context();
    if (!ctx) return false;
    if (clouds.empty() || clouds.size() > 16 || (!transformations.empty() && transformations.size() != clouds.size())) {
        con_err() << "merge_clouds: 1 to 16 clouds and one transformation per cloud (or none) are required" << std::endl;
        return false;
    }
    std::vector<std::vector<float>> flat;
    std::vector<const float *> ptr;
    std::vector<uint32_t> n;
    std::vector<float> T16;
    for (size_t c = 0; c < clouds.size(); ++c) {
        if (!clouds[c]) { con_err() << "merge_clouds: null cloud" << std::endl; return false; }
        flat.push_back(flatten(*clouds[c]));
        n.push_back((uint32_t)clouds[c]->size());
        if (!transformations.empty())
            for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) T16.push_back(transformations[c](r, q));
    }
    for (auto &f : flat) ptr.push_back(f.data());
    std::vector<float> rows;
    plade_merge_summary s;
    if (!merge_packed(ctx, (uint32_t)clouds.size(), ptr.data(), n.data(), T16.empty() ? nullptr : T16.data(), leaf, rows, s)) return false;
    unflatten(rows.data(), (size_t)s.n_out, merged);
    if (info) { info->n_in = s.n_in; info->n_out = s.n_out; info->n_shared = s.n_shared; info->max_count = s.max_count; }
    return true;
}

bool load_ply_cloud(const std::string &file_name, pcl::PointCloud<pcl::PointNormal> &cloud) {
    std::vector<float> pos_nrm;
    std::string err;
    std::vector<std::string> warnings;
    bool estimate = false;
    if (!read_ply_cloud(file_name, pos_nrm, err, &warnings, nullptr, &estimate)) {
        if (!err.empty()) con_err() << err << std::endl;
        return false;
    }
    for (auto &w : warnings) con_out() << w << std::endl;
    if (!prepare_loaded(file_name, pos_nrm, estimate)) return false;
    unflatten(pos_nrm.data(), pos_nrm.size() / 6, cloud);
    return cloud.size() > 0;
}
