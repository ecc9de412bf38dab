// oracle/plade_oracle.cpp -- TEST INFRASTRUCTURE ONLY.
//
// CPU restatement, written from scratch, of PLADE's registration hot path
// (SURVEY.md section 8a rows A3-A13).  It is the parity checker for the HIP
// path and the timed single-thread CPU baseline ("port"); it is never linked
// into, imported by or called from the product (plade_amd/, libplade_hip.so).
//
// Every function cites the reference file:line it follows (paths relative to
// /root/reference).  fp32 expressions are evaluated in the reference's own
// operation order (see oracle/orc_math.h); compile with -ffp-contract=off.
//
// Pinning status (details in DESIGN.md):
//   pinned against the real reference pieces via oracle/_ref + tests/golden:
//     A3 score, A4 connected component, A5 LS fit, A7 radius match (libann),
//     A8 umeyama + OBB eigensolver (Eigen), A12 overlap + A13 kNN/radius
//     semantics (FLANN).
//   "parity unpinned" (PCL / PLADE glue cannot be compiled here: no Boost):
//     VoxelGrid ordering, clustering, plane-consistency, penetration filter and
//     the driver plade.cpp:31-580 are restated from source reading only.
//   closest points of two lines (util.cpp:1183-1226, 1467-1497): two modes (orc_set_closest_point_mode).
//     mode 0 (default, what the HIP path computes): the exact closed form in fp64;
//     mode 1 "svd_fp32": cv::solve(A, B, X, DECOMP_SVD) restated operation for operation --
//     JacobiSVDImpl_<float> + SVBkSbImpl_ of OpenCV 2.4 (3rd_party/opencv/modules/core/src/lapack.cpp:
//     533-710, 751-812, 1335-1460), driven exactly like the reference.  OpenCV itself cannot be
//     built here (cmake-generated headers), so mode 1 is "restated, unpinned by a build"; it measures
//     what the closed form changes downstream (tests/test_oracle_golden.py::test_a6_*).
#include "plade_oracle.h"
#include "orc_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <cmath>
#include <cfloat>
#include <vector>
#include <map>
#include <string>
#include <algorithm>
#include <numeric>
#include <chrono>
#include <unordered_map>

using namespace orc;

namespace {

inline V3 ld3(const float *p) { return V3(p[0], p[1], p[2]); }
inline void st3(float *p, V3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }

// ---------------------------------------------------------------------------
// Exact fixed-radius / kNN search over an xyz cloud with FLANN's distance
// (flann/algorithms/dist.h:74-98: result += diff*diff in x,y,z order, fp32)
// and FLANN's strict `dist < radius` test (flann/util/result_set.h:479,582).
// A uniform grid replaces the kd-tree: the result SET is identical because the
// predicate is evaluated on the same fp32 distance.
struct GridIndex {
    const V3 *pts = nullptr;
    int n = 0;
    float cell = 1.f, inv = 1.f;
    V3 mn;
    int dx = 1, dy = 1, dz = 1;
    std::vector<int> start;  // dx*dy*dz + 1
    std::vector<int> items;

    static inline float d2(V3 q, V3 p) {
        float ax = q.x - p.x, ay = q.y - p.y, az = q.z - p.z;
        float r = ax * ax;
        r += ay * ay;
        r += az * az;
        return r;
    }
    inline int cx(float v, float o, int d) const {
        int c = (int)std::floor((v - o) * inv);
        return c < 0 ? 0 : (c >= d ? d - 1 : c);
    }
    void build(const V3 *p, int count, float cell_size) {
        pts = p; n = count;
        if (n == 0) { start.assign(2, 0); dx = dy = dz = 1; return; }
        V3 mx = p[0]; mn = p[0];
        for (int i = 1; i < n; ++i) {
            mn.x = std::min(mn.x, p[i].x); mn.y = std::min(mn.y, p[i].y); mn.z = std::min(mn.z, p[i].z);
            mx.x = std::max(mx.x, p[i].x); mx.y = std::max(mx.y, p[i].y); mx.z = std::max(mx.z, p[i].z);
        }
        cell = cell_size;
        for (;;) {
            inv = 1.f / cell;
            double ex = std::floor((mx.x - mn.x) * inv) + 1, ey = std::floor((mx.y - mn.y) * inv) + 1,
                   ez = std::floor((mx.z - mn.z) * inv) + 1;
            if (ex * ey * ez <= 4.0e6) { dx = (int)ex; dy = (int)ey; dz = (int)ez; break; }
            cell *= 2.f;
        }
        start.assign((size_t)dx * dy * dz + 1, 0);
        std::vector<int> cid(n);
        for (int i = 0; i < n; ++i) {
            int c = cx(p[i].x, mn.x, dx) + dx * (cx(p[i].y, mn.y, dy) + dy * cx(p[i].z, mn.z, dz));
            cid[i] = c;
            start[c + 1]++;
        }
        for (size_t i = 1; i < start.size(); ++i) start[i] += start[i - 1];
        items.resize(n);
        std::vector<int> fill(start.begin(), start.end() - 1);
        for (int i = 0; i < n; ++i) items[fill[cid[i]]++] = i;
    }
    // f(index, d2) for every point with d2 < r2 (strict).  The cell window is
    // padded by one cell so fp rounding of the window can never drop a hit.
    template <class F>
    void radius(V3 q, float r2, F f) const {
        if (n == 0) return;
        float r = std::sqrt(r2) * 1.0001f + 1e-30f;
        int x0 = cx(q.x - r, mn.x, dx), x1 = cx(q.x + r, mn.x, dx);
        int y0 = cx(q.y - r, mn.y, dy), y1 = cx(q.y + r, mn.y, dy);
        int z0 = cx(q.z - r, mn.z, dz), z1 = cx(q.z + r, mn.z, dz);
        // points outside the grid bbox clamp to border cells; a query far outside still works
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                int base = dx * (y + dy * z);
                for (int k = start[base + x0]; k < start[base + x1 + 1]; ++k) {
                    int i = items[k];
                    float d = d2(q, pts[i]);
                    if (d < r2) f(i, d);
                }
            }
    }
    // k smallest squared distances, ascending (values only; ties are value-identical)
    void knn_d2(V3 q, int k, std::vector<float> &out) const {
        out.clear();
        if (n == 0) return;
        if (k > n) k = n;
        int qx = cx(q.x, mn.x, dx), qy = cx(q.y, mn.y, dy), qz = cx(q.z, mn.z, dz);
        std::vector<float> heap;  // max-heap of best k
        int maxring = std::max(dx, std::max(dy, dz));
        for (int ring = 0; ring <= maxring; ++ring) {
            // once we hold k candidates and the next ring cannot contain anything closer, stop
            if ((int)heap.size() == k) {
                float lim = (ring - 1) * cell;  // every point in ring >= `ring` is farther than this
                // distance from q to the boundary of the (ring-1) box is >= (ring-1)*cell - (offset within cell) .. use conservative bound
                float worst = heap.front();
                float safe = lim - cell;  // conservative (q may sit anywhere in its cell)
                if (safe > 0 && safe * safe > worst) break;
            }
            int x0 = qx - ring, x1 = qx + ring, y0 = qy - ring, y1 = qy + ring, z0 = qz - ring, z1 = qz + ring;
            for (int z = std::max(z0, 0); z <= std::min(z1, dz - 1); ++z)
                for (int y = std::max(y0, 0); y <= std::min(y1, dy - 1); ++y) {
                    bool edge_zy = (z == z0 || z == z1 || y == y0 || y == y1);
                    for (int x = std::max(x0, 0); x <= std::min(x1, dx - 1); ++x) {
                        if (!edge_zy && x != x0 && x != x1) continue;  // only the shell
                        int c = x + dx * (y + dy * z);
                        for (int kk = start[c]; kk < start[c + 1]; ++kk) {
                            float d = d2(q, pts[items[kk]]);
                            if ((int)heap.size() < k) { heap.push_back(d); std::push_heap(heap.begin(), heap.end()); }
                            else if (d < heap.front()) {
                                std::pop_heap(heap.begin(), heap.end());
                                heap.back() = d;
                                std::push_heap(heap.begin(), heap.end());
                            }
                        }
                    }
                }
        }
        std::sort(heap.begin(), heap.end());
        out = heap;
    }
};

// r2 as pcl::KdTreeFLANN::radiusSearch forms it (kdtree_flann.hpp:193):
// static_cast<float>(radius * radius) with `double radius`.
inline float pcl_r2(double radius) { return static_cast<float>(radius * radius); }

// pcl::transformPointCloud, dense branch (pcl-1.8.1/common/include/pcl/common/impl/transforms.hpp:69-71)
inline V3 pcl_transform(const float *T /*4x4 row-major*/, V3 p) {
    return V3(T[0] * p.x + T[1] * p.y + T[2] * p.z + T[3], T[4] * p.x + T[5] * p.y + T[6] * p.z + T[7],
              T[8] * p.x + T[9] * p.y + T[10] * p.z + T[11]);
}
inline void make_T(const M3 &R, V3 t, float *T) {
    for (int r = 0; r < 3; ++r) { T[4 * r] = R.m[r][0]; T[4 * r + 1] = R.m[r][1]; T[4 * r + 2] = R.m[r][2]; }
    T[3] = t.x; T[7] = t.y; T[11] = t.z;
    T[12] = T[13] = T[14] = 0.f; T[15] = 1.f;
}

// ---------------------------------------------------------------------------
// A3  point-to-plane inlier test.
// ransac/FlatNormalThreshPointCompatibilityFunc.h:14-23, ransac/Plane.h:31-34,
// ransac/basic.h:80-86 (dot = ((x*x') + (y*y')) + (z*z')), visitor
// ransac/ScorePrimitiveShapeVisitor.h:39-46.
inline float schnabel_dot(const float *a, const float *b) {
    float s = a[0] * b[0];
    s += a[1] * b[1];
    s += a[2] * b[2];
    return s;
}
inline bool plane_compatible(const float *plane4, const float *pn, float eps, float cos_thresh) {
    float dist = std::fabs(plane4[3] - schnabel_dot(plane4, pn));
    if (dist < eps) return std::fabs(schnabel_dot(plane4, pn + 3)) >= cos_thresh;
    return false;
}

// ---------------------------------------------------------------------------
// A4  bitmap connected component for planes.
// ransac/GfxTL/HyperplaneCoordinateSystem.h:81-93 (AutoCAD arbitrary axis),
// PlanePrimitiveShape.cpp:164-207 (Parameters/BitmapExtent/InBitmap),
// BitmapPrimitiveShape.h:101-150 (BuildBitmap), BitmapPrimitiveShape.cpp:97-205,
// Bitmap.cpp:154-260 (DilateCross), 459-570 (ErodeCross), 633-834 (Components).
struct HCS { float a0[3], a1[3]; };
inline void gfx_normalize(float *v) {
    // GfxTL VectorXD::Normalize: v /= Length(), Length = sqrt(sum of squares sequentially)
    float l = v[0] * v[0];
    l += v[1] * v[1];
    l += v[2] * v[2];
    l = std::sqrt(l);
    v[0] /= l; v[1] /= l; v[2] /= l;
}
inline void gfx_cross(const float *a, const float *b, float *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
inline HCS hcs_from_normal(const float *n) {
    HCS h;
    const float ey[3] = {0, 1, 0}, ez[3] = {0, 0, 1};
    if (std::fabs(n[0]) < 0.015625f && std::fabs(n[1]) < 0.015625f) gfx_cross(ey, n, h.a0);
    else gfx_cross(ez, n, h.a0);
    gfx_normalize(h.a0);
    gfx_cross(n, h.a0, h.a1);
    gfx_normalize(h.a1);
    return h;
}

void dilate_cross(const std::vector<char> &b, int ue, int ve, std::vector<char> &o) {
    // 4-neighbourhood OR, no wrapping (planes: uwrap = vwrap = false)
    for (int v = 0; v < ve; ++v)
        for (int u = 0; u < ue; ++u) {
            bool r = b[v * ue + u];
            if (u > 0) r = r || b[v * ue + u - 1];
            if (u < ue - 1) r = r || b[v * ue + u + 1];
            if (v > 0) r = r || b[(v - 1) * ue + u];
            if (v < ve - 1) r = r || b[(v + 1) * ue + u];
            o[v * ue + u] = r;
        }
}
void erode_cross(const std::vector<char> &b, int ue, int ve, std::vector<char> &o) {
    // 4-neighbourhood AND over the neighbours that exist (border pixels only test
    // in-image neighbours: Bitmap.cpp:459-570 spells each border case out that way)
    for (int v = 0; v < ve; ++v)
        for (int u = 0; u < ue; ++u) {
            bool r = b[v * ue + u];
            if (u > 0) r = r && b[v * ue + u - 1];
            if (u < ue - 1) r = r && b[v * ue + u + 1];
            if (v > 0) r = r && b[(v - 1) * ue + u];
            if (v < ve - 1) r = r && b[(v + 1) * ue + u];
            o[v * ue + u] = r;
        }
}
// 8-connected components; labels numbered by raster-first pixel (Bitmap.cpp:633-834:
// temp labels are handed out in raster order and merged towards the smaller id).
// Returns number of foreground components; comp[i] = 0 background, 1.. component id.
int components8(const std::vector<char> &b, int ue, int ve, std::vector<int> &comp, std::vector<size_t> &sizes) {
    comp.assign(b.size(), 0);
    sizes.assign(1, 0);
    std::vector<int> stack;
    int cur = 0;
    for (int i = 0; i < ue * ve; ++i) {
        if (!b[i]) { sizes[0]++; continue; }
        if (comp[i]) continue;
        ++cur;
        sizes.push_back(0);
        comp[i] = cur;
        stack.push_back(i);
        while (!stack.empty()) {
            int p = stack.back();
            stack.pop_back();
            sizes[cur]++;
            int pu = p % ue, pv = p / ue;
            for (int dv = -1; dv <= 1; ++dv)
                for (int du = -1; du <= 1; ++du) {
                    int u = pu + du, v = pv + dv;
                    if (u < 0 || v < 0 || u >= ue || v >= ve) continue;
                    int q = v * ue + u;
                    if (b[q] && !comp[q]) { comp[q] = cur; stack.push_back(q); }
                }
        }
    }
    return cur;
}

int connected_component(const float *pos_nrm, const float *normal, const float *point,
                        std::vector<int> &indices, float eps, bool filtering) {
    size_t size = indices.size();
    if (!size) return 0;
    HCS h = hcs_from_normal(normal);
    std::vector<std::pair<float, float>> params(size);
    float mnu = INFINITY, mnv = INFINITY, mxu = -INFINITY, mxv = -INFINITY;
    for (size_t i = 0; i < size; ++i) {
        const float *p = pos_nrm + 6 * (size_t)indices[i];
        float pp[3] = {p[0] - point[0], p[1] - point[1], p[2] - point[2]};
        // Vec3f::dot(const float*) (ransac/basic.h:88-91): a*x + b*y + c*z left to right
        params[i].first = pp[0] * h.a0[0] + pp[1] * h.a0[1] + pp[2] * h.a0[2];
        params[i].second = pp[0] * h.a1[0] + pp[1] * h.a1[1] + pp[2] * h.a1[2];
        mnu = std::min(mnu, params[i].first); mxu = std::max(mxu, params[i].first);
        mnv = std::min(mnv, params[i].second); mxv = std::max(mxv, params[i].second);
    }
    size_t ue = size_t(std::ceil((mxu - mnu) / eps)) + 1;
    size_t ve = size_t(std::ceil((mxv - mnv) / eps)) + 1;
    if (ue < 2) ue = 2;
    if (ve < 2) ve = 2;
    std::vector<char> bmp(ue * ve, 0), tmp(ue * ve, 0);
    std::vector<size_t> bidx(size);
    for (size_t i = 0; i < size; ++i) {
        int bu = (int)std::floor((params[i].first - mnu) / eps);
        int bv = (int)std::floor((params[i].second - mnv) / eps);
        bu = std::min(std::max(bu, 0), (int)ue - 1);
        bv = std::min(std::max(bv, 0), (int)ve - 1);
        bidx[i] = bu + bv * ue;
        bmp[bidx[i]] = 1;
    }
    if (filtering) {
        dilate_cross(bmp, (int)ue, (int)ve, tmp);
        erode_cross(tmp, (int)ue, (int)ve, bmp);
    }
    std::vector<int> comp;
    std::vector<size_t> sizes;
    int nc = components8(bmp, (int)ue, (int)ve, comp, sizes);
    if (nc < 1) return 0;  // labels.size() <= 1
    int best = 1;
    for (int i = 2; i <= nc; ++i)
        if (sizes[best] < sizes[i]) best = i;
    size_t off = 0;
    for (size_t i = 0; i < size; ++i)
        if (comp[bidx[i]] == best) { std::swap(indices[off], indices[i]); ++off; }
    return (int)off;
}

// ---------------------------------------------------------------------------
// A5  LS plane refit: mean (ransac/GfxTL/Mean.h:31-46, fp32 sequential),
// covariance about the mean (GfxTL/Covariance.h CovarianceMatrix), Jacobi
// eigen-decomposition (GfxTL/Jacobi.h), normal = eigenvector of the smallest
// |eigenvalue| (GfxTL/Plane.h:56-95); Plane(mean, normal) (ransac/Plane.cpp:21-26).
// The eigen-solve here is a plain cyclic Jacobi in double on the fp32 covariance:
// the reference's own fp32 accumulation order noise (~1e-4 relative on d at 1e5
// points) is larger than any difference between symmetric eigen-solvers, and the
// parity bar for this row is a tolerance (tests/test_oracle_vs_ref.py).
void jacobi_sym3(double a[3][3], double d[3], double v[3][3]) {
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) v[i][j] = i == j;
    const double scale = std::fabs(a[0][0]) + std::fabs(a[1][1]) + std::fabs(a[2][2]);
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = std::fabs(a[0][1]) + std::fabs(a[0][2]) + std::fabs(a[1][2]);
        if (off <= 1e-24 * scale) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (std::fabs(a[p][q]) < 1e-300) continue;
                double theta = (a[q][q] - a[p][p]) / (2 * a[p][q]);
                double t = (theta >= 0 ? 1 : -1) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
                double c = 1 / std::sqrt(t * t + 1), s = t * c;
                for (int k = 0; k < 3; ++k) {
                    double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {
                    double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq; v[k][q] = s * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < 3; ++i) d[i] = a[i][i];
}

void ls_fit(const float *pos_nrm, const int *indices, int m, float *out7) {
    float mean[3] = {0, 0, 0}, tw = 0;
    for (int i = 0; i < m; ++i) {
        const float *p = pos_nrm + 6 * (size_t)indices[i];
        mean[0] += 1.f * p[0]; mean[1] += 1.f * p[1]; mean[2] += 1.f * p[2];
        tw += 1.f;
    }
    if (tw) { mean[0] /= tw; mean[1] /= tw; mean[2] /= tw; }
    float c[3][3] = {{0}};
    float tot = 0;
    for (int i = 0; i < m; ++i) {
        const float *p = pos_nrm + 6 * (size_t)indices[i];
        float d[3] = {p[0] - mean[0], p[1] - mean[1], p[2] - mean[2]};
        for (int r = 0; r < 3; ++r) for (int k = r; k < 3; ++k) c[r][k] += d[r] * d[k];
        tot += 1.f;
    }
    double a[3][3], ev[3], v[3][3];
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) a[r][k] = (k >= r ? c[r][k] : c[k][r]) / (tot ? tot : 1.f);
    jacobi_sym3(a, ev, v);
    int mi = 0;
    for (int i = 1; i < 3; ++i) if (std::fabs(ev[i]) < std::fabs(ev[mi])) mi = i;
    float nrm[3] = {(float)v[0][mi], (float)v[1][mi], (float)v[2][mi]};
    for (int k = 0; k < 3; ++k) { out7[k] = nrm[k]; out7[3 + k] = mean[k]; }
    // m_dist = m_pos.dot(m_normal)  (Vec3f::dot, sequential)
    out7[6] = schnabel_dot(mean, nrm);
}

// ---------------------------------------------------------------------------
// A13  average_spacing (code/PLADE/util.cpp:1619-1648)
float average_spacing(const std::vector<V3> &pts, int k, int samples) {
    size_t num = pts.size();
    if (num == 0) return 0.f;
    // grid cell: aim at ~8 points per cell from the bbox volume/surface heuristics
    V3 mn = pts[0], mx = pts[0];
    for (auto &p : pts) {
        mn.x = std::min(mn.x, p.x); mn.y = std::min(mn.y, p.y); mn.z = std::min(mn.z, p.z);
        mx.x = std::max(mx.x, p.x); mx.y = std::max(mx.y, p.y); mx.z = std::max(mx.z, p.z);
    }
    double ex = mx.x - mn.x, ey = mx.y - mn.y, ez = mx.z - mn.z;
    double area = 2 * (ex * ey + ey * ez + ex * ez);
    float cell = (float)std::sqrt(std::max(area, 1e-12) / (double)num) * 2.f;
    if (!(cell > 0)) cell = 1.f;
    GridIndex g;
    g.build(pts.data(), (int)num, cell);
    double total = 0.0;
    size_t step = 1;
    if (num > (size_t)samples) step = num / samples;
    size_t total_count = 0;
    std::vector<float> d2;
    for (size_t i = 0; i < num; i += step) {
        g.knn_d2(pts[i], k, d2);
        int nbs = (int)d2.size();
        if (nbs <= 1) continue;
        double avg = 0.0;
        for (int j = 1; j < nbs; ++j) avg += std::sqrt(d2[j]);  // std::sqrt(float)
        total += (avg / nbs);
        ++total_count;
    }
    return static_cast<float>(total / total_count);
}

// pcl::VoxelGrid<PointT>::applyFilter, no field filter, min_points_per_voxel = 0,
// downsample_all_data = true -> CentroidPoint (AccumulatorXYZ: float sum / n)
// (pcl-1.8.1/filters/include/pcl/filters/impl/voxel_grid.hpp:214-262, 310-345, 416-426;
//  common/include/pcl/common/impl/accumulators.hpp:65-84).  Called via
// DownSamplePointCloud (code/PLADE/util.h:161-184).
struct CPI {
    unsigned idx, pi;
    bool operator<(const CPI &o) const { return idx < o.idx; }
};
int voxel_downsample(const std::vector<V3> &in, float leaf, int sort_mode, std::vector<V3> &out) {
    out.clear();
    if (in.empty() || leaf <= 0) return -1;
    float inv = 1.f / leaf;  // Eigen::Array4f::Ones() / leaf_size_.array()
    V3 mn(FLT_MAX, FLT_MAX, FLT_MAX), mx(-FLT_MAX, -FLT_MAX, -FLT_MAX);
    for (auto &p : in) {
        mn.x = std::min(mn.x, p.x); mn.y = std::min(mn.y, p.y); mn.z = std::min(mn.z, p.z);
        mx.x = std::max(mx.x, p.x); mx.y = std::max(mx.y, p.y); mx.z = std::max(mx.z, p.z);
    }
    int64_t ddx = (int64_t)((mx.x - mn.x) * inv) + 1, ddy = (int64_t)((mx.y - mn.y) * inv) + 1,
            ddz = (int64_t)((mx.z - mn.z) * inv) + 1;
    if (ddx * ddy * ddz > (int64_t)INT32_MAX) { out = in; return 1; }  // "leaf size too small": output = input
    int minb[3] = {(int)std::floor(mn.x * inv), (int)std::floor(mn.y * inv), (int)std::floor(mn.z * inv)};
    int maxb[3] = {(int)std::floor(mx.x * inv), (int)std::floor(mx.y * inv), (int)std::floor(mx.z * inv)};
    int divb[3] = {maxb[0] - minb[0] + 1, maxb[1] - minb[1] + 1, maxb[2] - minb[2] + 1};
    int mul[3] = {1, divb[0], divb[0] * divb[1]};
    std::vector<CPI> iv;
    iv.reserve(in.size());
    for (size_t i = 0; i < in.size(); ++i) {
        const V3 &p = in[i];
        int i0 = (int)(std::floor(p.x * inv) - (float)minb[0]);
        int i1 = (int)(std::floor(p.y * inv) - (float)minb[1]);
        int i2 = (int)(std::floor(p.z * inv) - (float)minb[2]);
        iv.push_back(CPI{(unsigned)(i0 * mul[0] + i1 * mul[1] + i2 * mul[2]), (unsigned)i});
    }
    if (sort_mode == 0) std::sort(iv.begin(), iv.end());  // as PCL: unstable
    else std::stable_sort(iv.begin(), iv.end());
    size_t index = 0;
    while (index < iv.size()) {
        size_t i = index + 1;
        while (i < iv.size() && iv[i].idx == iv[index].idx) ++i;
        V3 acc(0, 0, 0);
        for (size_t li = index; li < i; ++li) {
            const V3 &p = in[iv[li].pi];
            acc.x += p.x; acc.y += p.y; acc.z += p.z;
        }
        float cnt = (float)(i - index);  // xyz / n  with size_t n -> float scalar
        out.push_back(V3(acc.x / cnt, acc.y / cnt, acc.z / cnt));
        index = i;
    }
    return 0;
}

// ComputeBoundingBox (code/PLADE/util.h:186-248) with pcl::compute3DCentroid /
// computeCovarianceMatrixNormalized (pcl-1.8.1/common/include/pcl/common/impl/centroid.hpp:79-121,
// 250-300), SelfAdjointEigenSolver, transformPointCloud, getMinMax3D.
struct OBB {
    V3 center;
    double width, height, depth;
    V3 corners[8];
};
// sum_mode 0: PCL's order -- compute3DCentroid / computeCovarianceMatrixNormalized add the points one after the other in
// fp32 (centroid.hpp:79-121, 250-300).  sum_mode 1: the order of the GPU path (k_obb_units): lane t of 1024 adds the points
// t, t + 1024, t + 2048, ... one after the other, then the 1024 lane sums are added in lane order -- a re-association of
// the same fp32 additions (a 150 000-point serial chain is what a GPU cannot run; the strided lanes are what it sums in
// parallel with coalesced reads).  The two differ by a few ulp of the sums.
int bounding_box(const std::vector<V3> &pts, OBB &o, bool want_corners, int sum_mode = 0) {
    if (pts.empty()) return -1;
    const size_t n = pts.size(), LANES = 1024;
    float c[3] = {0, 0, 0};
    if (sum_mode == 0) {
        for (auto &p : pts) { c[0] += p.x; c[1] += p.y; c[2] += p.z; }
    } else {
        for (size_t t = 0; t < LANES; ++t) {
            float s[3] = {0, 0, 0};
            for (size_t i = t; i < n; i += LANES) { s[0] += pts[i].x; s[1] += pts[i].y; s[2] += pts[i].z; }
            c[0] += s[0]; c[1] += s[1]; c[2] += s[2];
        }
    }
    float nf = (float)pts.size();
    c[0] /= nf; c[1] /= nf; c[2] /= nf;
    M3 cov;
    memset(&cov, 0, sizeof(cov));
    auto add_point = [&](M3 &acc, const V3 &p) {
        float px = p.x - c[0], py = p.y - c[1], pz = p.z - c[2];
        acc.m[1][1] += py * py;
        acc.m[1][2] += py * pz;
        acc.m[2][2] += pz * pz;
        float qx = px * px, qy = py * px, qz = pz * px;  // pt *= pt.x()
        acc.m[0][0] += qx;
        acc.m[0][1] += qy;
        acc.m[0][2] += qz;
    };
    if (sum_mode == 0) {
        for (auto &p : pts) add_point(cov, p);
    } else {
        for (size_t t = 0; t < LANES; ++t) {
            M3 s;
            memset(&s, 0, sizeof(s));
            for (size_t i = t; i < n; i += LANES) add_point(s, pts[i]);
            cov.m[1][1] += s.m[1][1]; cov.m[1][2] += s.m[1][2]; cov.m[2][2] += s.m[2][2];
            cov.m[0][0] += s.m[0][0]; cov.m[0][1] += s.m[0][1]; cov.m[0][2] += s.m[0][2];
        }
    }
    cov.m[1][0] = cov.m[0][1]; cov.m[2][0] = cov.m[0][2]; cov.m[2][1] = cov.m[1][2];
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) cov.m[r][k] /= nf;
    float ev[3];
    M3 E;
    selfadjoint_eig3(cov, ev, E);
    // eigDx.col(2) = eigDx.col(0).cross(eigDx.col(1))
    V3 c0(E.m[0][0], E.m[1][0], E.m[2][0]), c1(E.m[0][1], E.m[1][1], E.m[2][1]);
    V3 c2 = cross(c0, c1);
    E.m[0][2] = c2.x; E.m[1][2] = c2.y; E.m[2][2] = c2.z;
    // p2w = [E^T | -1.f * (E^T * centroid)]
    M3 Et = transpose(E);
    V3 cen(c[0], c[1], c[2]);
    V3 t = -1.f * mul(Et, cen);
    float P[16];
    make_T(Et, t, P);
    V3 mn(FLT_MAX, FLT_MAX, FLT_MAX), mx(-FLT_MAX, -FLT_MAX, -FLT_MAX);
    for (auto &p : pts) {
        V3 q = pcl_transform(P, p);
        mn.x = std::min(mn.x, q.x); mn.y = std::min(mn.y, q.y); mn.z = std::min(mn.z, q.z);
        mx.x = std::max(mx.x, q.x); mx.y = std::max(mx.y, q.y); mx.z = std::max(mx.z, q.z);
    }
    V3 mean_diag = 0.5f * (mx + mn);
    o.center = mul(E, mean_diag) + cen;
    o.width = mx.x - mn.x;   // float subtraction, widened
    o.depth = mx.y - mn.y;
    o.height = mx.z - mn.z;
    if (want_corners) {
        float x = mn.x, y = mn.y, z = mn.z;
        double w = o.width, d = o.depth, h = o.height;
        V3 cs[8] = {mn,
                    V3(x, (float)(y + d), z),
                    V3(x, (float)(y + d), (float)(z + h)),
                    V3(x, y, (float)(z + h)),
                    V3((float)(x + w), y, (float)(z + h)),
                    V3((float)(x + w), (float)(y + d), z),
                    V3((float)(x + w), y, z),
                    V3((float)(x + w), (float)(y + d), (float)(z + h))};
        float Q[16];
        make_T(E, cen, Q);
        for (int i = 0; i < 8; ++i) o.corners[i] = pcl_transform(Q, cs[i]);
    }
    return 0;
}

// ProjectPoints2Plane (code/PLADE/util.h:292-340), finite-point branch.
inline V3 project_to_plane(V3 p, const float *pl) {
    float A = pl[0], B = pl[1], C = pl[2], D = pl[3];
    float k = -(A * p.x + B * p.y + C * p.z + D) / (A * A + B * B + C * C);
    return V3(p.x + k * A, p.y + k * B, p.z + k * C);
}

// ---------------------------------------------------------------------------
// A6  lines
// ComputeIntersectionLineOfTwoPlanes (code/PLADE/util.cpp:626-676); 2x2 inverse as
// cv::Mat::inv does it for CV_64F 2x2 (opencv/modules/core/src/lapack.cpp:1036-1073)
// and the 2x1 product in double.
int intersection_line(const float *pl1, const float *pl2, V3 &vec, V3 &pt) {
    V3 p1(pl1[0], pl1[1], pl1[2]), p2(pl2[0], pl2[1], pl2[2]);
    normalize(p1);
    normalize(p2);
    if (std::fabs(dot(p1, p2)) > 0.95) return -1;  // float |.| compared with the double literal
    vec = cross(p1, p2);
    normalize(vec);
    double b0 = -pl1[3], b1 = -pl2[3];
    auto solve = [&](float a00, float a01, float a10, float a11, double &r0, double &r1) {
        double A00 = a00, A01 = a01, A10 = a10, A11 = a11;
        double d = A00 * A11 - A01 * A10;
        if (d != 0.) {
            d = 1. / d;
            double i00 = A11 * d, i11 = A00 * d, i01 = -A01 * d, i10 = -A10 * d;
            r0 = i00 * b0 + i01 * b1;
            r1 = i10 * b0 + i11 * b1;
        } else { r0 = r1 = 0; }  // unreachable: guarded by the 1e-6 float test
    };
    double r0, r1;
    if (std::fabs(pl1[0] * pl2[1] - pl2[0] * pl1[1]) > 1e-6) {
        solve(pl1[0], pl1[1], pl2[0], pl2[1], r0, r1);
        pt = V3((float)r0, (float)r1, 0.f);
    } else if (std::fabs(pl1[0] * pl2[2] - pl2[0] * pl1[2]) > 1e-6) {
        solve(pl1[0], pl1[2], pl2[0], pl2[2], r0, r1);
        pt = V3((float)r0, 0.f, (float)r1);
    } else if (std::fabs(pl1[1] * pl2[2] - pl2[1] * pl1[2]) > 1e-6) {
        solve(pl1[1], pl1[2], pl2[1], pl2[2], r0, r1);
        pt = V3(0.f, (float)r0, (float)r1);
    } else return -1;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// cv::solve(A, B, X, cv::DECOMP_SVD) for CV_32F and one right-hand side, restated from OpenCV 2.4
// (code/3rd_party/opencv/modules/core/src/lapack.cpp): cv::solve :1335-1460 transposes A into `At` (n rows of m),
// runs JacobiSVD(At, w, Vt, m, n) (:533-699, the one-sided Jacobi of Hestenes on the rows of At; float data, double
// accumulators, eps = FLT_EPSILON * 2, minval = FLT_MIN, at most max(m, 30) sweeps) and back-substitutes with
// SVBkSb(m, n, w, u = At (uT), v = Vt (vT), b, nb = 1) (:751-812, eps = (float)(DBL_EPSILON * 2)).
// The SSE2 paths of VBLAS<float>::givens (:421-437) perform the same fp32 operations as the scalar tail, lane by lane.
static int g_cp_mode = 1;            // 1 svd_fp32 = the reference's arithmetic (default), 0 closed form (fp64)

struct CvRng {                       // cv::RNG (core/operations.hpp: MWC, state * 4164903690 + carry)
    uint64_t state;
    unsigned next() { state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32); return (unsigned)state; }
};

// At: n rows of m floats (row stride m); W: n; Vt: n x n
void cv_jacobi_svd_f32(float *At, float *_W, float *Vt, int m, int n) {
    const double minval = FLT_MIN;
    const float eps = FLT_EPSILON * 2;
    const int n1 = n;
    std::vector<double> W(n);
    int i, j, k, iter, max_iter = std::max(m, 30);
    float c, s;
    double sd;
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) { float t = At[i * m + k]; sd += (double)t * t; }
        W[i] = sd;
        for (k = 0; k < n; k++) Vt[i * n + k] = 0;
        Vt[i * n + i] = 1;
    }
    for (iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (i = 0; i < n - 1; i++)
            for (j = i + 1; j < n; j++) {
                float *Ai = At + i * m, *Aj = At + j * m;
                double a = W[i], p = 0, b = W[j];
                for (k = 0; k < m; k++) p += (double)Ai[k] * Aj[k];
                if (std::abs(p) <= eps * std::sqrt((double)a * b)) continue;
                p *= 2;
                double beta = a - b, gamma = hypot_glibc235((double)p, beta);   // hypot(): see orc_math.h
                if (beta < 0) {
                    double delta = (gamma - beta) * 0.5;
                    s = (float)std::sqrt(delta / gamma);
                    c = (float)(p / (gamma * s * 2));
                } else {
                    c = (float)std::sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * c * 2));
                }
                a = b = 0;
                for (k = 0; k < m; k++) {
                    float t0 = c * Ai[k] + s * Aj[k];
                    float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                float *Vi = Vt + i * n, *Vj = Vt + j * n;
                for (k = 0; k < n; k++) {
                    float t0 = c * Vi[k] + s * Vj[k];
                    float t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0; Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) { float t = At[i * m + k]; sd += (double)t * t; }
        W[i] = std::sqrt(sd);
    }
    for (i = 0; i < n - 1; i++) {
        j = i;
        for (k = i + 1; k < n; k++) if (W[j] < W[k]) j = k;
        if (i != j) {
            std::swap(W[i], W[j]);
            for (k = 0; k < m; k++) std::swap(At[i * m + k], At[j * m + k]);
            for (k = 0; k < n; k++) std::swap(Vt[i * n + k], Vt[j * n + k]);
        }
    }
    for (i = 0; i < n; i++) _W[i] = (float)W[i];
    CvRng rng{0x12345678};
    for (i = 0; i < n1; i++) {
        sd = i < n ? W[i] : 0;
        while (sd <= minval) {
            // a zero singular value: a random vector, orthogonalised against the left singular vectors found so far
            const float val0 = (float)(1. / m);
            for (k = 0; k < m; k++) { float val = (rng.next() & 256) != 0 ? val0 : -val0; At[i * m + k] = val; }
            for (iter = 0; iter < 2; iter++)
                for (j = 0; j < i; j++) {
                    sd = 0;
                    for (k = 0; k < m; k++) sd += At[i * m + k] * At[j * m + k];
                    float asum = 0;
                    for (k = 0; k < m; k++) {
                        float t = (float)(At[i * m + k] - sd * At[j * m + k]);
                        At[i * m + k] = t;
                        asum += std::abs(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (k = 0; k < m; k++) At[i * m + k] *= asum;
                }
            sd = 0;
            for (k = 0; k < m; k++) { float t = At[i * m + k]; sd += (double)t * t; }
            sd = std::sqrt(sd);
        }
        s = (float)(1 / sd);
        for (k = 0; k < m; k++) At[i * m + k] *= s;
    }
}

// x (n) = V * inv(W) * U^T * b for one right-hand side; u = At rows (uT), v = Vt rows (vT)
void cv_svbksb_f32(int m, int n, const float *w, const float *u, const float *v, const float *b, float *x) {
    const float eps = (float)(DBL_EPSILON * 2);
    double threshold = 0;
    const int nm = std::min(m, n);
    for (int i = 0; i < n; i++) x[i] = 0;
    for (int i = 0; i < nm; i++) threshold += w[i];
    threshold *= eps;
    for (int i = 0; i < nm; i++, u += m, v += n) {
        double wi = w[i];
        if ((double)std::abs(wi) <= threshold) continue;
        wi = 1 / wi;
        double s = 0;
        for (int j = 0; j < m; j++) s += u[j] * b[j];     // float product, double accumulator (lapack.cpp:791-793)
        s *= wi;
        for (int j = 0; j < n; j++) x[j] = (float)(x[j] + s * v[j]);
    }
}

// A: m x n row-major, B: m, X: n
void cv_solve_svd_f32(const float *A, const float *B, float *X, int m, int n) {
    std::vector<float> At((size_t)n * m), W(n), Vt((size_t)n * n);
    for (int r = 0; r < m; ++r) for (int c = 0; c < n; ++c) At[(size_t)c * m + r] = A[(size_t)r * n + c];   // transpose(src, a)
    cv_jacobi_svd_f32(At.data(), W.data(), Vt.data(), m, n);
    cv_svbksb_f32(m, n, W.data(), At.data(), Vt.data(), B, X);
}

// the 9 x 9 system of util.cpp:1183-1220 and its solution (point1 = X[0..2], point2 = X[4..6])
void closest_points_svd(const V3 &u1, const V3 &p1, const V3 &u2, const V3 &p2, const V3 &dir, V3 &q1, V3 &q2) {
    float A[81] = {0}, B[9] = {0}, X[9];
    auto a = [&](int r, int c) -> float & { return A[r * 9 + c]; };
    a(0, 0) = 1; a(0, 3) = -u1.x; a(1, 1) = 1; a(1, 3) = -u1.y; a(2, 2) = 1; a(2, 3) = -u1.z;
    a(3, 4) = 1; a(3, 7) = -u2.x; a(4, 5) = 1; a(4, 7) = -u2.y; a(5, 6) = 1; a(5, 7) = -u2.z;
    a(6, 0) = -1; a(6, 4) = 1; a(6, 8) = -dir.x; a(7, 1) = -1; a(7, 5) = 1; a(7, 8) = -dir.y; a(8, 2) = -1; a(8, 6) = 1; a(8, 8) = -dir.z;
    B[0] = p1.x; B[1] = p1.y; B[2] = p1.z; B[3] = p2.x; B[4] = p2.y; B[5] = p2.z;
    cv_solve_svd_f32(A, B, X, 9, 9);
    q1 = V3(X[0], X[1], X[2]);
    q2 = V3(X[4], X[5], X[6]);
}

// ComputeNearstTwoPointsOfTwo3DLine (code/PLADE/util.cpp:1167-1229).
// Mutates u1,u2 (normalised in place, exactly like the reference's non-const refs).
// Closest points: exact closed form in fp64 (DEVIATION from the fp32 9x9 SVD, see header).
int closest_points(V3 &u1, const V3 &p1, V3 &u2, const V3 &p2, V3 &q1, V3 &q2, double &len) {
    normalize(u1);
    normalize(u2);
    if (u1.x == u2.x && u1.y == u2.y && u1.z == u2.z) return -1;
    if (g_cp_mode == 1) {   // util.cpp:1176-1226 with the real solver's arithmetic
        V3 dir = cross(u1, u2);
        normalize(dir);
        closest_points_svd(u1, p1, u2, p2, dir, q1, q2);
        len = norm(q1 - q2);
        return 0;
    }
    double ax = u1.x, ay = u1.y, az = u1.z, bx = u2.x, by = u2.y, bz = u2.z;
    double wx = (double)p1.x - p2.x, wy = (double)p1.y - p2.y, wz = (double)p1.z - p2.z;
    double a = ax * ax + ay * ay + az * az;
    double b = ax * bx + ay * by + az * bz;
    double c = bx * bx + by * by + bz * bz;
    double d = ax * wx + ay * wy + az * wz;
    double e = bx * wx + by * wy + bz * wz;
    double den = a * c - b * b;
    double t1 = (b * e - c * d) / den;
    double t2 = (a * e - b * d) / den;
    q1 = V3((float)(p1.x + t1 * ax), (float)(p1.y + t1 * ay), (float)(p1.z + t1 * az));
    q2 = V3((float)(p2.x + t2 * bx), (float)(p2.y + t2 * by), (float)(p2.z + t2 * bz));
    len = norm(q1 - q2);  // (point1 - point2).norm() in float, widened
    return 0;
}

// ComputeIntersectionPointOf23DLine (code/PLADE/util.cpp:1461-1500): least-squares
// point of two lines = midpoint of the common perpendicular (closed form, fp64;
// DEVIATION from the fp32 6x5 SVD solve).
int intersection_point_2lines(const V3 &v1, const V3 &p1, const V3 &v2, const V3 &p2, V3 &out) {
    if (std::fabs(dot(v1, v2)) > 0.9999) return -1;
    if (g_cp_mode == 1) {   // the 6 x 5 system of util.cpp:1467-1497
        float A[30] = {0}, B[6], X[5];
        A[0 * 5 + 0] = 1; A[0 * 5 + 3] = -v1.x; A[1 * 5 + 1] = 1; A[1 * 5 + 3] = -v1.y; A[2 * 5 + 2] = 1; A[2 * 5 + 3] = -v1.z;
        A[3 * 5 + 0] = 1; A[3 * 5 + 4] = -v2.x; A[4 * 5 + 1] = 1; A[4 * 5 + 4] = -v2.y; A[5 * 5 + 2] = 1; A[5 * 5 + 4] = -v2.z;
        B[0] = p1.x; B[1] = p1.y; B[2] = p1.z; B[3] = p2.x; B[4] = p2.y; B[5] = p2.z;
        cv_solve_svd_f32(A, B, X, 6, 5);
        out = V3(X[0], X[1], X[2]);
        return 0;
    }
    double ax = v1.x, ay = v1.y, az = v1.z, bx = v2.x, by = v2.y, bz = v2.z;
    double wx = (double)p1.x - p2.x, wy = (double)p1.y - p2.y, wz = (double)p1.z - p2.z;
    double a = ax * ax + ay * ay + az * az, b = ax * bx + ay * by + az * bz, c = bx * bx + by * by + bz * bz;
    double d = ax * wx + ay * wy + az * wz, e = bx * wx + by * wy + bz * wz;
    double den = a * c - b * b;
    double t1 = (b * e - c * d) / den, t2 = (a * e - b * d) / den;
    double x1 = p1.x + t1 * ax, y1 = p1.y + t1 * ay, z1 = p1.z + t1 * az;
    double x2 = p2.x + t2 * bx, y2 = p2.y + t2 * by, z2 = p2.z + t2 * bz;
    out = V3((float)(0.5 * (x1 + x2)), (float)(0.5 * (y1 + y2)), (float)(0.5 * (z1 + z2)));
    return 0;
}

struct Line {
    V3 vec, pt;
    int sp[2];
};

// ComputeDescriptorVectorForPairLines, method22 (code/PLADE/util.cpp:533-577).
// d[0] (the scaled line distance) is filled by the caller.
void descriptor22(const Line &l1, const Line &l2, const std::vector<V3> &normals, float *d, V3 &newLine1,
                  V3 &newLine2) {
    V3 l1sp1 = normals[l1.sp[0]], l1sp2 = normals[l1.sp[1]], l2sp1 = normals[l2.sp[0]], l2sp2 = normals[l2.sp[1]];
    float angle1 = std::fabs(dot(l1.vec, l2sp1)), angle2 = std::fabs(dot(l1.vec, l2sp2));
    V3 n2a, n2b, n1a, n1b;
    if (angle1 <= angle2) { n2a = l2sp1; n2b = l2sp2; } else { n2a = l2sp2; n2b = l2sp1; }
    newLine2 = cross(n2a, n2b);
    angle1 = std::fabs(dot(l2.vec, l1sp1));
    angle2 = std::fabs(dot(l2.vec, l1sp2));
    if (angle1 <= angle2) { n1a = l1sp1; n1b = l1sp2; } else { n1a = l1sp2; n1b = l1sp1; }
    newLine1 = cross(n1a, n1b);
    d[1] = dot(newLine1, newLine2);
    d[2] = dot(n1a, n1b);
    d[3] = dot(n2a, n2b);
    d[4] = dot(newLine1, n2a);
    d[5] = dot(newLine1, n2b);
    d[6] = dot(newLine2, n1a);
    d[7] = dot(newLine2, n1b);
}

// ---------------------------------------------------------------------------
// A7  KdTreeSearchNDim<VectorXf,8>::find_neighbors(p, 0, 0.04, ...)
// (ann_1.1.2/include/ANN/ANN.h:978-1029): coordinates widened to double, squared
// distance accumulated in dimension order, in range <=> dist <= double(float(r*r))
// (ann_1.1.2/src/kd_fix_rad_search.cpp:148-183), sorted ascending, ties by index.
struct Match { int q, t; double d2; };
void match_descriptors(const float *qry, int dq, const float *tgt, int dt, float radius,
                       std::vector<int64_t> &offsets, std::vector<int> &nbr, std::vector<double> &dist2) {
    offsets.assign(dq + 1, 0);
    nbr.clear();
    dist2.clear();
    if (radius < 0) return;
    float sqRadF = radius * radius;
    double sqRad = sqRadF;
    // accelerate: sort targets by dim 0, window |q0 - t0| <= radius (+slack), then exact test
    std::vector<int> order(dt);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return tgt[8 * (size_t)a] < tgt[8 * (size_t)b]; });
    std::vector<float> key(dt);
    for (int i = 0; i < dt; ++i) key[i] = tgt[8 * (size_t)order[i]];
    std::vector<std::pair<double, int>> hits;
    for (int q = 0; q < dq; ++q) {
        const float *pq = qry + 8 * (size_t)q;
        hits.clear();
        if (dt > 0) {
            float lo = pq[0] - radius * 1.001f - 1e-6f, hi = pq[0] + radius * 1.001f + 1e-6f;
            int a = (int)(std::lower_bound(key.begin(), key.end(), lo) - key.begin());
            int b = (int)(std::upper_bound(key.begin(), key.end(), hi) - key.begin());
            if (!(pq[0] == pq[0])) { a = 0; b = 0; }  // NaN query never matches (NaN <= x false)
            for (int k = a; k < b; ++k) {
                const float *pt = tgt + 8 * (size_t)order[k];
                double dist = 0;
                bool in = true;
                for (int d = 0; d < 8; ++d) {
                    double t = (double)pq[d] - (double)pt[d];
                    dist += t * t;
                    if (dist > sqRad) { in = false; break; }
                }
                if (in && dist <= sqRad) hits.push_back(std::make_pair(dist, order[k]));
            }
        }
        std::sort(hits.begin(), hits.end());
        for (auto &h : hits) { nbr.push_back(h.second); dist2.push_back(h.first); }
        offsets[q + 1] = (int64_t)nbr.size();
    }
}

// ---------------------------------------------------------------------------
// A12  ComputeOverlap<PointXYZ> (code/PLADE/util.h:611-647) as driven by
// code/PLADE/plade.cpp:547-562.
int overlap_count(const std::vector<V3> &src_ds, const GridIndex &tgt_grid, const std::vector<V3> &tgt_ds,
                  const float *T16, V3 center, float src_radius, float inlier_dist) {
    float R2 = pcl_r2((double)src_radius);
    float r2 = pcl_r2((double)inlier_dist);
    // coarse region U = { t : |t - c'|^2 < R2 }
    std::vector<V3> sub;
    tgt_grid.radius(center, R2, [&](int i, float) { sub.push_back(tgt_ds[i]); });
    if (sub.empty()) return -1;
    GridIndex g;
    g.build(sub.data(), (int)sub.size(), inlier_dist > 0 ? inlier_dist : 1.f);
    int count = 0;
    for (auto &p : src_ds) {
        V3 q = pcl_transform(T16, p);
        bool hit = false;
        g.radius(q, r2, [&](int, float) { hit = true; });
        if (hit) ++count;
    }
    return count;
}

// pcl::getEulerAngles (pcl-1.8.1/common/include/pcl/common/impl/eigen.hpp:664-669):
// unqualified atan2/asin on float arguments -> the double C functions, narrowed on store.
inline void euler_angles(const M3 &R, float &roll, float &pitch, float &yaw) {
    roll = (float)std::atan2((double)R.m[2][1], (double)R.m[2][2]);
    pitch = (float)std::asin((double)-R.m[2][0]);
    yaw = (float)std::atan2((double)R.m[1][0], (double)R.m[0][0]);
}

// ClusterTransformation (util.cpp:1245-1277) = PCL ConditionalEuclideanClustering::segment
// (pcl-1.8.1/segmentation/.../conditional_euclidean_clustering.hpp:42-138) with EnforceSimilarity (util.cpp:1232-1243) on
// the Euler angles.  Pinned against the FLANN composition of the same loop (oracle/ref/ref_shim.cpp
// ref_cluster_transforms, tests/golden/g10_cluster.npz).
inline void cluster_transforms(const std::vector<V3> &iT, const std::vector<V3> &eul, float distanceThreshold, float g_angle,
                               std::vector<std::vector<int>> &clusters) {
    clusters.clear();
    GridIndex g;
    g.build(iT.data(), (int)iT.size(), distanceThreshold > 0 ? distanceThreshold : 1.f);
    float r2 = pcl_r2((double)distanceThreshold);
    std::vector<char> processed(iT.size(), 0);
    std::vector<std::pair<float, int>> nn;
    for (int seed = 0; seed < (int)iT.size(); ++seed) {
        if (processed[seed]) continue;
        std::vector<int> cur;
        cur.push_back(seed);
        processed[seed] = 1;
        for (size_t cii = 0; cii < cur.size(); ++cii) {
            int a = cur[cii];
            nn.clear();
            g.radius(iT[a], r2, [&](int i, float d) { nn.push_back(std::make_pair(d, i)); });
            if (nn.empty()) continue;
            // sorted results, nn_indices[0] skipped (hpp:101).  The entry at distance 0 with the
            // smallest index stands in for "first in FLANN order" (the point itself unless an
            // exact duplicate exists).
            std::sort(nn.begin(), nn.end());
            for (size_t nii = 1; nii < nn.size(); ++nii) {
                int b = nn[nii].second;
                if (processed[b]) continue;
                // Eigen::VectorXf(3).squaredNorm(): sequential
                float t0 = eul[a].x - eul[b].x, t1 = eul[a].y - eul[b].y, t2 = eul[a].z - eul[b].z;
                float sq = (t0 * t0 + t1 * t1) + t2 * t2;
                if (sq < g_angle) { cur.push_back(b); processed[b] = 1; }
            }
        }
        clusters.push_back(cur);
    }
}

struct LengthIndex { float length; int index; };
inline bool cmp_greater(const LengthIndex &a, const LengthIndex &b) { return a.length > b.length; }
inline bool cmp_less(const LengthIndex &a, const LengthIndex &b) { return a.length < b.length; }

struct PlaneInfo {
    std::vector<V3> ds;        // per-plane voxel-downsampled points
    GridIndex grid;            // over ds
    V3 corners8[8];
    V3 four[4];                // projected first four OBB corners
    V3 center;
    float radius;
};

struct CloudSide {
    std::vector<V3> ds;        // whole cloud downsampled
    V3 bcenter;
    double radius;
    std::vector<PlaneInfo> planes;
    std::vector<float> coef;   // P x 4
    std::vector<V3> normals;
    std::vector<Line> lines;
};

using Clock = std::chrono::steady_clock;
inline double secs(Clock::time_point a, Clock::time_point b) {
    return std::chrono::duration<double>(b - a).count();
}

}  // namespace

struct orc_reg {
    std::map<std::string, std::vector<char>> blobs;
    template <class T>
    void put(const std::string &name, const T *data, size_t count) {
        std::vector<char> &b = blobs[name];
        b.resize(count * sizeof(T));
        if (count) memcpy(b.data(), data, count * sizeof(T));
    }
    template <class T>
    void put1(const std::string &name, T v) { put(name, &v, 1); }
};

namespace {

// One of the two walks of AreTwoPlanesPenetrable along the common segment (util.cpp:1379-1405 / :1416-1442):
// A = the cloud whose points are classified against planeB; B = the gate cloud.  Pinned against the FLANN composition of
// the same loop (oracle/ref/ref_shim.cpp ref_pen_walk, tests/golden/g11_penetration.npz).
void pen_walk(const std::vector<V3> &ptsA, const GridIndex &gA, const GridIndex &gB, const float *planeB, V3 startPoint, V3 direc,
              float length, float searchRadius, float minDistance, int &positiveNum, int &negativeNum, int &skipped) {
    const float half_r2 = pcl_r2((double)(searchRadius / 2)), full_r2 = pcl_r2((double)searchRadius);
    positiveNum = negativeNum = skipped = 0;
    std::vector<char> check(ptsA.size(), 1);
    for (float dist = 0; dist < length; dist += searchRadius) {
        V3 sp = startPoint + dist * direc;
        int cnt = 0;
        gB.radius(sp, half_r2, [&](int, float) { ++cnt; });
        if (cnt < 2) { ++skipped; continue; }  // radiusSearch(..., max_nn = 2) < 2
        gA.radius(sp, full_r2, [&](int i, float) {
            if (check[i]) {
                check[i] = 0;
                const V3 &p = ptsA[i];
                float td = planeB[0] * p.x + planeB[1] * p.y + planeB[2] * p.z + planeB[3];
                if (std::fabs(td) > minDistance) { if (td >= 0) positiveNum++; else negativeNum++; }
            }
        });
    }
}

// AreTwoPlanesPenetrable (code/PLADE/util.cpp:1279-1458).  `au` (orc_penetration_items): where the pair left the function,
// the common segment and both walks' counts; with it the second walk runs also where the first fails its thresholds
// (the verdict is the same: it needs both).
int planes_penetrable(const float *plane1, const float *plane2, const V3 *corners1, const V3 *corners2,
                      const std::vector<V3> &pts1, const GridIndex &g1, const std::vector<V3> &pts2,
                      const GridIndex &g2, bool &pen, float searchRadius, int minPointsNum, float minDistance,
                      orc_pen_record *au = nullptr) {
    pen = false;
    V3 lineVec, linePoint;
    if (au) au->status = ORC_PEN_NO_LINE;
    if (0 != intersection_line(plane1, plane2, lineVec, linePoint)) return -1;
    auto edge_hits = [&](const V3 *c, std::vector<V3> &out) {
        const int num = 4;
        for (int i = 1; i <= num; ++i) {
            V3 tl = c[i % num] - c[(i - 1) % num];
            normalize(tl);
            V3 ip;
            if (0 != intersection_point_2lines(lineVec, linePoint, tl, c[i - 1], ip)) continue;
            if (dot(c[(i - 1) % num] - ip, c[i % num] - ip) > 0) continue;
            out.push_back(ip);
        }
    };
    std::vector<V3> ip1, ip2;
    edge_hits(corners1, ip1);
    edge_hits(corners2, ip2);
    if (au) au->status = ip1.empty() ? ORC_PEN_NO_HITS : ORC_PEN_HIT_COUNT;
    if (ip1.empty()) { pen = false; return 0; } else if (ip1.size() != 2) return -1;
    if (au) au->status = ip2.empty() ? ORC_PEN_NO_HITS : ORC_PEN_HIT_COUNT;
    if (ip2.empty()) { pen = false; return 0; } else if (ip2.size() != 2) return -1;
    V3 direc = ip1[1] - ip1[0];
    normalize(direc);
    V3 inter[4] = {ip1[0], ip1[1], ip2[0], ip2[1]};
    LengthIndex lv[4];
    for (int i = 0; i < 4; ++i) { lv[i].length = dot(inter[i] - inter[0], direc); lv[i].index = i; }
    std::sort(lv, lv + 4, cmp_less);
    if (au) au->status = ORC_PEN_NO_OVERLAP;
    if (0 == (lv[0].index / 2 - lv[1].index / 2)) { pen = false; return 0; }
    V3 startPoint = inter[lv[1].index], endPoint = inter[lv[2].index];
    float length = norm(endPoint - startPoint);
    int pos[2] = {0, 0}, neg[2] = {0, 0}, skipped[2] = {0, 0};
    auto ratio_ok = [&](int w) { return !(double(std::max(pos[w], neg[w])) / std::min(pos[w], neg[w] + 1) > 5); };
    pen_walk(pts1, g1, g2, plane2, startPoint, direc, length, searchRadius, minDistance, pos[0], neg[0], skipped[0]);
    const bool ok0 = !(pos[0] < minPointsNum || neg[0] < minPointsNum) && ratio_ok(0);
    bool ok1 = false;
    if (ok0 || au) {
        pen_walk(pts2, g2, g1, plane1, startPoint, direc, length, searchRadius, minDistance, pos[1], neg[1], skipped[1]);
        ok1 = !(pos[1] < minPointsNum && neg[1] < minPointsNum) && ratio_ok(1);
    }
    pen = ok0 && ok1;
    if (au) {
        au->status = ORC_PEN_WALKED;
        for (int q = 0; q < 4; ++q) au->plane1[q] = plane1[q];
        st3(au->start, startPoint); st3(au->direc, direc);
        au->length = length;
        au->nsteps = 0;
        for (float dist = 0; dist < length; dist += searchRadius) au->nsteps++;   // the walks' own loop (pen_walk)
        for (int w = 0; w < 2; ++w) { au->positive[w] = pos[w]; au->negative[w] = neg[w]; au->skipped[w] = skipped[w]; }
        au->verdict = pen ? 1 : 0;
    }
    return 0;
}

// per-cloud preparation: plade.cpp:75-172 (target) / 290-381 (source)
int prepare_side(orc_reg *h, const char *tag, const float *pos_nrm, int n, const float *planes,
                 const int *offsets, const int *idx, int np, float leaf, int sort_mode, CloudSide &S) {
    std::vector<V3> all(n);
    for (int i = 0; i < n; ++i) all[i] = ld3(pos_nrm + 6 * (size_t)i);
    voxel_downsample(all, leaf, sort_mode, S.ds);
    OBB ob;
    if (0 != bounding_box(S.ds, ob, false, sort_mode)) return -1;
    S.bcenter = ob.center;
    S.radius = std::max(std::max(ob.width, ob.height), ob.depth) / 2;
    h->put(std::string(tag) + "_ds", (const float *)S.ds.data(), S.ds.size() * 3);
    h->put(std::string(tag) + "_bcenter", (const float *)&S.bcenter, 3);
    h->put1(std::string(tag) + "_radius", S.radius);
    S.coef.assign(planes, planes + 4 * (size_t)np);
    S.normals.resize(np);
    for (int i = 0; i < np; ++i) S.normals[i] = ld3(planes + 4 * (size_t)i);
    S.planes.resize(np);
    std::vector<float> pcr(4 * (size_t)np), pfour(12 * (size_t)np);
    std::vector<int> pds_off(np + 1, 0);
    std::vector<float> pds_all;
    for (int i = 0; i < np; ++i) {
        PlaneInfo &pi = S.planes[i];
        std::vector<V3> tmp;
        tmp.reserve(offsets[i + 1] - offsets[i]);
        for (int j = offsets[i]; j < offsets[i + 1]; ++j) tmp.push_back(ld3(pos_nrm + 6 * (size_t)idx[j]));
        voxel_downsample(tmp, leaf, sort_mode, pi.ds);
        OBB pb;
        bounding_box(pi.ds, pb, true, sort_mode);
        for (int k = 0; k < 8; ++k) pi.corners8[k] = pb.corners[k];
        for (int k = 0; k < 4; ++k) pi.four[k] = project_to_plane(pb.corners[k], planes + 4 * (size_t)i);
        pi.center = (pi.four[0] + pi.four[2]) / 2.f;
        pi.radius = norm(pi.four[0] - pi.four[2]) / 2.f;
        pi.grid.build(pi.ds.data(), (int)pi.ds.size(), leaf * 5.f / 4.f);
        st3(&pcr[4 * (size_t)i], pi.center);
        pcr[4 * (size_t)i + 3] = pi.radius;
        for (int k = 0; k < 4; ++k) st3(&pfour[12 * (size_t)i + 3 * k], pi.four[k]);
        pds_off[i + 1] = pds_off[i] + (int)pi.ds.size();
        pds_all.insert(pds_all.end(), (const float *)pi.ds.data(), (const float *)pi.ds.data() + 3 * pi.ds.size());
    }
    h->put(std::string(tag) + "_plane_center_radius", pcr.data(), pcr.size());
    h->put(std::string(tag) + "_plane_four", pfour.data(), pfour.size());
    h->put(std::string(tag) + "_plane_ds_offsets", pds_off.data(), pds_off.size());
    h->put(std::string(tag) + "_plane_ds", pds_all.data(), pds_all.size());
    // intersection lines
    S.lines.clear();
    for (int i = 0; i < np; ++i)
        for (int j = i + 1; j < np; ++j) {
            Line L;
            if (0 != intersection_line(planes + 4 * (size_t)i, planes + 4 * (size_t)j, L.vec, L.pt)) continue;
            V3 tv = L.pt - S.bcenter;
            double dt = dot(tv, L.vec);
            double distance = std::sqrt((double)sqnorm(tv) - dt * dt);
            if (distance > S.radius) continue;
            // ComputeMeanDistanceOfLine2Plane x2 (util.h:389-426): results unused downstream,
            // but each call re-normalises the stored line vector in place.
            normalize(L.vec);
            normalize(L.vec);
            L.sp[0] = i; L.sp[1] = j;
            S.lines.push_back(L);
        }
    std::vector<float> ld(S.lines.size() * 8);
    for (size_t i = 0; i < S.lines.size(); ++i) {
        st3(&ld[8 * i], S.lines[i].vec); st3(&ld[8 * i + 3], S.lines[i].pt);
        ld[8 * i + 6] = (float)S.lines[i].sp[0]; ld[8 * i + 7] = (float)S.lines[i].sp[1];
    }
    h->put(std::string(tag) + "_lines", ld.data(), ld.size());
    return 0;
}

}  // namespace

extern "C" {

int orc_score_plane(const float *pos_nrm, const int32_t *shape_index, int n, const float *plane4, float eps,
                    float cos_thresh, int32_t *idx_out, int32_t *count_out) {
    int c = 0;
    for (int i = 0; i < n; ++i) {
        if (shape_index && shape_index[i] != -1) continue;
        if (plane_compatible(plane4, pos_nrm + 6 * (size_t)i, eps, cos_thresh)) {
            if (idx_out) idx_out[c] = i;
            ++c;
        }
    }
    *count_out = c;
    return 0;
}

int orc_plane_from_points(const float *t, float *plane4) {
    // n = (p2-p1) x (p3-p2); reject |n|^2 < 1e-6; normalise; dist = p1.n  (ransac/Plane.cpp:29-38)
    float a[3] = {t[3] - t[0], t[4] - t[1], t[5] - t[2]}, b[3] = {t[6] - t[3], t[7] - t[4], t[8] - t[5]};
    float nrm[3];
    gfx_cross(a, b, nrm);
    float sq = nrm[0] * nrm[0];
    sq += nrm[1] * nrm[1];
    sq += nrm[2] * nrm[2];
    if (sq < 1E-6f) return 0;
    // Vec3f::normalize (ransac/basic.h): divide by sqrt of the sequential sum of squares
    float l = std::sqrt(sq);
    nrm[0] /= l; nrm[1] /= l; nrm[2] /= l;
    plane4[0] = nrm[0]; plane4[1] = nrm[1]; plane4[2] = nrm[2];
    plane4[3] = schnabel_dot(t, nrm);
    return 1;
}

int orc_connected_component(const float *pos_nrm, int n, const float *normal3, const float *point3,
                            const int32_t *indices, int m, float bitmap_eps, int do_filtering, int32_t *kept_out) {
    (void)n;
    std::vector<int> ind(indices, indices + m);
    int kept = connected_component(pos_nrm, normal3, point3, ind, bitmap_eps, do_filtering != 0);
    for (int i = 0; i < kept; ++i) kept_out[i] = ind[i];
    return kept;
}

int orc_ls_fit(const float *pos_nrm, int n, const int32_t *indices, int m, float *out7) {
    (void)n;
    ls_fit(pos_nrm, indices, m, out7);
    return 0;
}

float orc_weighted_score(const float *pos_nrm, int n, const float *normal3, const float *point3,
                         const int32_t *indices, int m, float eps) {
    (void)n;
    float dist0 = schnabel_dot(point3, normal3);
    float score = 0;
    for (int i = 0; i < m; ++i) {
        const float *p = pos_nrm + 6 * (size_t)indices[i];
        float d = std::fabs(dist0 - schnabel_dot(normal3, p));
        score += std::exp(-d * d / (2.f / 9.f * eps * eps));  // ransac/ScoreComputer.h:10-16
    }
    return score;
}

float orc_cloud_scale(const float *pn, int n) {
    // plane_extraction.cpp:71-80 incl. the Z bug: maxZ stays -FLT_MAX, minZ ends as z of the last point
    float minX = FLT_MAX, minY = FLT_MAX, minZ = FLT_MAX, maxX = -FLT_MAX, maxY = -FLT_MAX, maxZ = -FLT_MAX;
    for (int i = 0; i < n; ++i) {
        float x = pn[6 * (size_t)i], y = pn[6 * (size_t)i + 1], z = pn[6 * (size_t)i + 2];
        minX = std::min(x, minX); minY = std::min(y, minY); minZ = std::min(z, minZ);
        maxX = std::max(x, maxX); maxY = std::max(y, maxY); minZ = std::max(z, maxZ);
    }
    float dx = maxX - minX, dy = maxY - minY, dz = maxZ - minZ;  // ransac/PointCloud.h:94-98
    return std::max(std::max(dx, dy), dz);
}

float orc_average_spacing(const float *xyz, int n, int stride, int k, int samples) {
    std::vector<V3> pts(n);
    for (int i = 0; i < n; ++i) pts[i] = ld3(xyz + (size_t)stride * i);
    return average_spacing(pts, k, samples);
}

int orc_voxel_downsample(const float *xyz, int n, int stride, float leaf, int sort_mode, float *out_xyz,
                         int32_t *n_out) {
    std::vector<V3> pts(n), out;
    for (int i = 0; i < n; ++i) pts[i] = ld3(xyz + (size_t)stride * i);
    int rc = voxel_downsample(pts, leaf, sort_mode, out);
    *n_out = (int)out.size();
    if (out_xyz) memcpy(out_xyz, out.data(), out.size() * 12);
    return rc;
}

int orc_bounding_box(const float *xyz, int n, float *center3, double *whd3, float *corners24) {
    return orc_bounding_box_mode(xyz, n, 0, center3, whd3, corners24);
}
int orc_bounding_box_mode(const float *xyz, int n, int sum_mode, float *center3, double *whd3, float *corners24) {
    std::vector<V3> pts(n);
    for (int i = 0; i < n; ++i) pts[i] = ld3(xyz + 3 * (size_t)i);
    OBB o;
    if (0 != bounding_box(pts, o, corners24 != nullptr, sum_mode)) return -1;
    st3(center3, o.center);
    whd3[0] = o.width; whd3[1] = o.height; whd3[2] = o.depth;
    if (corners24) for (int i = 0; i < 8; ++i) st3(corners24 + 3 * i, o.corners[i]);
    return 0;
}

int orc_intersection_line(const float *a4, const float *b4, float *vec3, float *point3) {
    V3 v, p;
    int rc = intersection_line(a4, b4, v, p);
    if (rc == 0) { st3(vec3, v); st3(point3, p); }
    return rc;
}

int orc_closest_points(const float *u1, const float *p1, const float *u2, const float *p2, float *q1, float *q2,
                       double *len) {
    V3 a = ld3(u1), b = ld3(u2), x, y;
    int rc = closest_points(a, ld3(p1), b, ld3(p2), x, y, *len);
    if (rc == 0) { st3(q1, x); st3(q2, y); }
    return rc;
}

int64_t orc_match_descriptors(const float *qry, int dq, const float *tgt, int dt, float radius,
                              int64_t *offsets_out, int32_t *nbr_out, double *dist2_out, int64_t cap) {
    std::vector<int64_t> off;
    std::vector<int> nb;
    std::vector<double> d2;
    match_descriptors(qry, dq, tgt, dt, radius, off, nb, d2);
    memcpy(offsets_out, off.data(), off.size() * 8);
    int64_t m = std::min<int64_t>((int64_t)nb.size(), cap);
    if (nbr_out) memcpy(nbr_out, nb.data(), m * 4);
    if (dist2_out) memcpy(dist2_out, d2.data(), m * 8);
    return (int64_t)nb.size();
}

void orc_umeyama3(const float *src9, const float *dst9, float *R9) {
    V3 s[3] = {ld3(src9), ld3(src9 + 3), ld3(src9 + 6)}, d[3] = {ld3(dst9), ld3(dst9 + 3), ld3(dst9 + 6)};
    M3 R = umeyama_rotation3(s, d);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R9[3 * r + c] = R.m[r][c];
}

void orc_selfadjoint_eig3(const float *cov9, float *evals3, float *evecs9) {
    M3 c, e;
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) c.m[r][k] = cov9[3 * r + k];
    selfadjoint_eig3(c, evals3, e);
    // same post-step as util.h:201 so the output is comparable with ref_selfadjoint_eig3
    V3 c0(e.m[0][0], e.m[1][0], e.m[2][0]), c1(e.m[0][1], e.m[1][1], e.m[2][1]);
    V3 c2 = cross(c0, c1);
    e.m[0][2] = c2.x; e.m[1][2] = c2.y; e.m[2][2] = c2.z;
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) evecs9[3 * r + k] = e.m[r][k];
}

int orc_overlap_count(const float *src_ds, int ns, const float *tgt_ds, int nt, const float *T16,
                      const float *center3, float src_radius, float inlier_dist) {
    std::vector<V3> s(ns), t(nt);
    for (int i = 0; i < ns; ++i) s[i] = ld3(src_ds + 3 * (size_t)i);
    for (int i = 0; i < nt; ++i) t[i] = ld3(tgt_ds + 3 * (size_t)i);
    GridIndex g;
    g.build(t.data(), nt, inlier_dist > 0 ? inlier_dist * 4.f : 1.f);
    return overlap_count(s, g, t, T16, ld3(center3), src_radius, inlier_dist);
}

orc_reg *orc_reg_create(void) { return new orc_reg; }
// G10 / G11 seams of the restatement (see cluster_transforms, pen_walk)
int orc_cluster_transforms(const float *t_xyz, const float *euler, int m, float distance_threshold, float g_angle, int *cluster_of) {
    std::vector<V3> T(m), E(m);
    for (int i = 0; i < m; ++i) { T[i] = ld3(t_xyz + 3 * (size_t)i); E[i] = ld3(euler + 3 * (size_t)i); }
    std::vector<std::vector<int>> clusters;
    if (m > 0) cluster_transforms(T, E, distance_threshold, g_angle, clusters);
    for (size_t c = 0; c < clusters.size(); ++c)
        for (int i : clusters[c]) cluster_of[i] = (int)c;
    return (int)clusters.size();
}
void orc_euler_angles(const float *R9, float *rpy3) {
    M3 R;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R.m[r][c] = R9[3 * r + c];
    euler_angles(R, rpy3[0], rpy3[1], rpy3[2]);
}
int orc_pen_walk(const float *pts_a, int na, const float *pts_b, int nb, const float *plane_b4, const float *start3,
                 const float *direc3, float length, float searchRadius, float minDistance, int *positive, int *negative,
                 int *skipped) {
    std::vector<V3> A(na), B(nb);
    for (int i = 0; i < na; ++i) A[i] = ld3(pts_a + 3 * (size_t)i);
    for (int i = 0; i < nb; ++i) B[i] = ld3(pts_b + 3 * (size_t)i);
    GridIndex ga, gb;
    ga.build(A.data(), na, searchRadius > 0 ? searchRadius : 1.f);
    gb.build(B.data(), nb, searchRadius > 0 ? searchRadius : 1.f);
    pen_walk(A, ga, gb, plane_b4, ld3(start3), ld3(direc3), length, searchRadius, minDistance, *positive, *negative, *skipped);
    return 0;
}

// Every triple (candidate, source plane, target plane) of the penetration filter's loop (util.cpp:450-519), none skipped:
// the loop of orc_registration below without its two `break`s, on the filter's own tables.
int orc_penetration_items(const float *cand, int K, const float *s_coef, const float *s_center, const float *s_four,
                          const float *s_pts, const int32_t *s_off, int ps, const float *t_coef, const float *t_center,
                          const float *t_four, const float *t_pts, const int32_t *t_off, int pt, float lengthThreshold,
                          float angleThreshold, orc_pen_record *records) {
    std::vector<std::vector<V3>> tds(pt);
    std::vector<GridIndex> tgrid(pt);
    for (int j1 = 0; j1 < pt; ++j1) {
        for (int q = t_off[j1]; q < t_off[j1 + 1]; ++q) tds[j1].push_back(ld3(t_pts + 3 * (size_t)q));
        tgrid[j1].build(tds[j1].data(), (int)tds[j1].size(), lengthThreshold > 0 ? lengthThreshold : 1.f);
    }
    for (int k = 0; k < K; ++k) {
        const float *c = cand + 12 * (size_t)k;
        M3 R;
        for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) R.m[r][q] = c[3 * r + q];
        const V3 T = ld3(c + 9);
        float T16[16];
        make_T(R, T, T16);
        for (int i1 = 0; i1 < ps; ++i1) {
            V3 pn = mul(R, ld3(s_coef + 4 * (size_t)i1));
            float plane1[4] = {pn.x, pn.y, pn.z, 0};
            plane1[3] = -(-s_coef[4 * (size_t)i1 + 3] + dot_seq(pn, T));
            std::vector<V3> tp;
            for (int q = s_off[i1]; q < s_off[i1 + 1]; ++q) tp.push_back(pcl_transform(T16, ld3(s_pts + 3 * (size_t)q)));
            V3 four[4], tfour[4];
            for (int q = 0; q < 4; ++q) four[q] = pcl_transform(T16, ld3(s_four + 12 * (size_t)i1 + 3 * q));
            GridIndex tg;
            bool built = false;
            V3 c2m = mul(R, ld3(s_center + 3 * (size_t)i1)) + T;
            for (int j1 = 0; j1 < pt; ++j1) {
                orc_pen_record &rec = records[((size_t)k * ps + i1) * pt + j1];
                memset(&rec, 0, sizeof(rec));
                rec.k = k; rec.i1 = i1; rec.j1 = j1; rec.status = ORC_PEN_GATED;
                V3 plane_A = ld3(t_coef + 4 * (size_t)j1);
                double c2p = (std::fabs(dot(plane_A, c2m) + t_coef[4 * (size_t)j1 + 3]) +
                              std::fabs(dot(pn, ld3(t_center + 3 * (size_t)j1)) + plane1[3])) / 2;
                if (c2p < lengthThreshold && dot(pn, plane_A) > angleThreshold) continue;
                if (!built) { tg.build(tp.data(), (int)tp.size(), lengthThreshold > 0 ? lengthThreshold : 1.f); built = true; }
                for (int q = 0; q < 4; ++q) tfour[q] = ld3(t_four + 12 * (size_t)j1 + 3 * q);
                bool isPen = false;
                planes_penetrable(plane1, t_coef + 4 * (size_t)j1, four, tfour, tp, tg, tds[j1], tgrid[j1], isPen,
                                  (float)(double)lengthThreshold, 10, (float)((double)lengthThreshold / 2), &rec);
            }
        }
    }
    return 0;
}

void orc_set_closest_point_mode(int mode) { g_cp_mode = mode == 1 ? 1 : 0; }
int orc_intersection_point(const float *v1, const float *p1, const float *v2, const float *p2, float *out) {
    V3 o;
    const int rc = intersection_point_2lines(ld3(v1), ld3(p1), ld3(v2), ld3(p2), o);
    if (rc == 0) st3(out, o);
    return rc;
}
void orc_solve_svd_f32(const float *A, const float *B, float *X, int m, int n) { cv_solve_svd_f32(A, B, X, m, n); }
double orc_hypot(double x, double y) { return hypot_glibc235(x, y); }
double orc_libm_hypot(double x, double y) { return hypot(x, y); }

void orc_reg_destroy(orc_reg *h) { delete h; }
int orc_dump_get(orc_reg *h, const char *name, const void **ptr, int64_t *nbytes) {
    auto it = h->blobs.find(name);
    if (it == h->blobs.end()) return -1;
    *ptr = it->second.data();
    *nbytes = (int64_t)it->second.size();
    return 0;
}

// registration(T, target, source, target_planes, source_planes): code/PLADE/plade.cpp:31-580
int orc_registration(orc_reg *h, const float *tgt_pn, int nt, const float *src_pn, int ns, const float *tgt_planes,
                     const int32_t *tgt_off, const int32_t *tgt_idx, int pt, const float *src_planes,
                     const int32_t *src_off, const int32_t *src_idx, int ps, int sort_mode, int max_candidates,
                     float *T16_out) {
    return orc_registration_sampled(h, tgt_pn, nt, src_pn, ns, tgt_planes, tgt_off, tgt_idx, pt, src_planes, src_off, src_idx, ps,
                                    sort_mode, max_candidates, 1, T16_out);
}

int orc_registration_sampled(orc_reg *h, const float *tgt_pn, int nt, const float *src_pn, int ns, const float *tgt_planes,
                             const int32_t *tgt_off, const int32_t *tgt_idx, int pt, const float *src_planes,
                             const int32_t *src_off, const int32_t *src_idx, int ps, int sort_mode, int max_candidates,
                             int pen_stride, float *T16_out) {
    h->blobs.clear();
    std::vector<double> tim;
    std::string tim_names;
    auto t0 = Clock::now();
    auto lap = [&](const char *name) {
        auto t1 = Clock::now();
        tim.push_back(secs(t0, t1));
        tim_names += name;
        tim_names += ";";
        t0 = t1;
    };
    for (int i = 0; i < 16; ++i) T16_out[i] = (i % 5 == 0) ? 1.f : 0.f;

    // plade.cpp:41  average_spacing(source_cloud, 6)
    const float average_space = orc_average_spacing(src_pn, ns, 6, 6, 10000);
    h->put1("average_spacing", average_space);
    lap("spacing");
    // plade.cpp:46-56
    float downSampleDistance = average_space * 4;
    float lengthThreshold = average_space * 5;
    float angleThreshold = 5.0 / 180 * M_PI;
    float cosAngleThreshold = cos(angleThreshold);
    float scale = lengthThreshold / cos(M_PI_2 - angleThreshold);
    h->put1("scale", scale);

    CloudSide M, C;  // main (target), current (source)
    if (0 != prepare_side(h, "tgt", tgt_pn, nt, tgt_planes, tgt_off, tgt_idx, pt, downSampleDistance, sort_mode, M))
        return 0;
    lap("prepare_tgt");

    // ConstructPairLinesKdTree (util.cpp:706-1165), tree "22" only
    const size_t Lm = M.lines.size();
    struct PairLine { V3 lineVec1, lineVec2, p1, p2; int i1, i2; };
    std::vector<PairLine> lf22;
    std::vector<float> tdesc;
    {
        float angleThresh = cos(10.0 / 180 * M_PI);
        struct NP { V3 p1, p2; double len; };
        std::vector<NP> ll(Lm * Lm);
        for (size_t i = 0; i < Lm; ++i)
            for (size_t j = 0; j < Lm; ++j) {
                if (i == j) continue;
                Line &l1 = M.lines[i];
                Line &l2 = M.lines[j];
                NP &e = ll[i * Lm + j];
                if (i > j) { NP &o = ll[j * Lm + i]; e.p1 = o.p2; e.p2 = o.p1; e.len = o.len; }
                else {
                    if (0 != closest_points(l1.vec, l1.pt, l2.vec, l2.pt, e.p1, e.p2, e.len)) e.len = -1;
                    e.len = e.len / scale;
                }
                if (std::fabs(dot(l1.vec, l2.vec)) > angleThresh) continue;
                PairLine pl;
                pl.p1 = e.p1; pl.p2 = e.p2; pl.i1 = (int)i; pl.i2 = (int)j;
                float d[8];
                descriptor22(l1, l2, M.normals, d, pl.lineVec1, pl.lineVec2);
                d[0] = (float)e.len;
                lf22.push_back(pl);
                tdesc.insert(tdesc.end(), d, d + 8);
            }
        // plade.cpp:258-285 recomputes all i<j closest points: results unused, but the
        // in-place normalisations still run.
        for (size_t i = 0; i < Lm; ++i)
            for (size_t j = i + 1; j < Lm; ++j) { normalize(M.lines[i].vec); normalize(M.lines[j].vec); }
    }
    h->put("tgt_desc", tdesc.data(), tdesc.size());
    lap("tgt_descriptors");

    if (0 != prepare_side(h, "src", src_pn, ns, src_planes, src_off, src_idx, ps, downSampleDistance, sort_mode, C))
        return 0;
    lap("prepare_src");

    // plade.cpp:451-482 source line-pair table
    const size_t Lc = C.lines.size();
    struct NPL { V3 p1, p2; double len; };
    std::vector<NPL> cl(Lc * Lc);
    for (size_t i = 0; i < Lc; ++i)
        for (size_t j = 0; j < Lc; ++j) {
            NPL &e = cl[i * Lc + j];
            if (i > j) { NPL &o = cl[j * Lc + i]; e.p1 = o.p2; e.p2 = o.p1; e.len = o.len; }
            else if (i < j) {
                if (0 != closest_points(C.lines[i].vec, C.lines[i].pt, C.lines[j].vec, C.lines[j].pt, e.p1, e.p2, e.len))
                    e.len = -1;
                e.len = e.len / scale;
            }
        }
    // plade.cpp:511-521
    std::vector<std::pair<int, int>> toMatch;
    {
        float angleThresh = cos(10.0 / 180 * M_PI);
        for (int i = 0; i < (int)Lc; ++i)
            for (int j = i + 1; j < (int)Lc; ++j) {
                if (std::fabs(dot(C.lines[i].vec, C.lines[j].vec)) > angleThresh) continue;
                toMatch.push_back(std::make_pair(i, j));
            }
    }
    // MatchingLines (util.cpp:31-520)
    std::vector<PairLine> qlines(toMatch.size());
    std::vector<float> qdesc(toMatch.size() * 8);
    for (size_t k = 0; k < toMatch.size(); ++k) {
        int i = toMatch[k].first, j = toMatch[k].second;
        PairLine &pl = qlines[k];
        pl.p1 = cl[i * Lc + j].p1; pl.p2 = cl[i * Lc + j].p2; pl.i1 = i; pl.i2 = j;
        float *d = &qdesc[8 * k];
        descriptor22(C.lines[i], C.lines[j], C.normals, d, pl.lineVec1, pl.lineVec2);
        d[0] = (float)cl[i * Lc + j].len;
    }
    h->put("src_desc", qdesc.data(), qdesc.size());
    lap("src_descriptors");

    std::vector<int64_t> moff;
    std::vector<int> mnbr;
    std::vector<double> md2;
    match_descriptors(qdesc.data(), (int)toMatch.size(), tdesc.data(), (int)lf22.size(), 0.04f, moff, mnbr, md2);
    h->put("match_offsets", moff.data(), moff.size());
    h->put("match_nbr", mnbr.data(), mnbr.size());
    h->put("match_dist2", md2.data(), md2.size());
    lap("match");

    // util.cpp:303-327: one (R,T) per (query, neighbour)
    std::vector<M3> iR;
    std::vector<V3> iT;
    iR.reserve(mnbr.size());
    iT.reserve(mnbr.size());
    for (size_t q = 0; q < toMatch.size(); ++q)
        for (int64_t k = moff[q]; k < moff[q + 1]; ++k) {
            const PairLine &ql = qlines[q];
            const PairLine &tl = lf22[mnbr[k]];
            // ComputeTransformationUsingTwoVecAndOnePoint (util.cpp:604-624)
            V3 s[3] = {ql.lineVec1, ql.lineVec2, cross(ql.lineVec1, ql.lineVec2)};
            V3 d[3] = {tl.lineVec1, tl.lineVec2, cross(tl.lineVec1, tl.lineVec2)};
            M3 R = umeyama_rotation3(s, d);
            V3 T = tl.p1 - mul(R, ql.p1);
            iR.push_back(R);
            iT.push_back(T);
        }
    {
        std::vector<float> rt(iR.size() * 12);
        for (size_t i = 0; i < iR.size(); ++i) {
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) rt[12 * i + 3 * r + c] = iR[i].m[r][c];
            st3(&rt[12 * i + 9], iT[i]);
        }
        h->put("initial_RT", rt.data(), rt.size());
    }
    lap("transforms");

    // ClusterTransformation (util.cpp:1245-1277) = PCL ConditionalEuclideanClustering
    // (pcl-1.8.1/segmentation/.../conditional_euclidean_clustering.hpp:42-138) with
    // EnforceSimilarity (util.cpp:1232-1243)
    std::vector<std::vector<int>> clusters;
    if (!iR.empty()) {
        const float distanceThreshold = (double)lengthThreshold / 2;  // parameter.lengthThreshold is double
        const float g_angle = (double)angleThreshold / 2;
        std::vector<V3> eul(iR.size());
        for (size_t i = 0; i < iR.size(); ++i) euler_angles(iR[i], eul[i].x, eul[i].y, eul[i].z);
        cluster_transforms(iT, eul, distanceThreshold, g_angle, clusters);
    }
    {
        std::vector<int> cs(clusters.size()), cseed(clusters.size());
        for (size_t i = 0; i < clusters.size(); ++i) { cs[i] = (int)clusters[i].size(); cseed[i] = clusters[i][0]; }
        h->put("cluster_sizes", cs.data(), cs.size());
        h->put("cluster_seeds", cseed.data(), cseed.size());
    }
    lap("cluster");

    // util.cpp:333-401
    std::vector<LengthIndex> sortVec(clusters.size());
    for (size_t i = 0; i < sortVec.size(); ++i) { sortVec[i].index = (int)i; sortVec[i].length = (float)clusters[i].size(); }
    std::sort(sortVec.begin(), sortVec.end(), cmp_greater);
    std::vector<std::vector<std::pair<int, int>>> matches;
    std::vector<M3> Rs;
    std::vector<V3> Ts;
    const float cosAngleTh = (float)(double)cosAngleThreshold;
    const float maxRadius = (float)M.radius;  // parameter.maxRadius is float
    for (size_t si = 0; si < sortVec.size(); ++si) {
        int k = clusters[sortVec[si].index][0];
        const M3 &R = iR[k];
        const V3 &T = iT[k];
        V3 tc = mul(R, C.bcenter) + T;
        if (norm(tc - M.bcenter) > maxRadius) continue;
        std::vector<std::pair<int, int>> pm;
        for (int i1 = 0; i1 < ps; ++i1) {
            V3 n1 = C.normals[i1];
            V3 plane1 = mul(R, n1);
            float d = -(-C.coef[4 * (size_t)i1 + 3] + dot_seq(plane1, T));
            V3 srcCenter2Dest = mul(R, C.planes[i1].center) + T;
            for (int j1 = 0; j1 < pt; ++j1) {
                V3 plane_A = M.normals[j1];
                if (dot(plane1, plane_A) < cosAngleTh) continue;
                double c2p = (std::fabs(dot(plane_A, srcCenter2Dest) + M.coef[4 * (size_t)j1 + 3]) +
                              std::fabs(dot(plane1, M.planes[j1].center) + d)) / 2;
                if (c2p > lengthThreshold) continue;
                double distance = norm(srcCenter2Dest - M.planes[j1].center);
                if (distance / (C.planes[i1].radius + M.planes[j1].radius) > 1) continue;
                pm.push_back(std::make_pair(i1, j1));
                break;
            }
        }
        matches.push_back(pm);
        Rs.push_back(R);
        Ts.push_back(T);
    }
    {
        std::vector<int> mc(matches.size());
        for (size_t i = 0; i < matches.size(); ++i) mc[i] = (int)matches[i].size();
        h->put("plane_match_counts", mc.data(), mc.size());
    }
    lap("plane_consistency");

    // util.cpp:403-445
    size_t maxMatchNum = 0;
    for (auto &m : matches) maxMatchNum = std::max(maxMatchNum, m.size());
    std::vector<std::vector<int>> matchedPlanes;
    if (maxMatchNum > 0) {
        int matchedCount = 0;
        for (size_t i = maxMatchNum; i >= 2; i--) {
            std::vector<int> tmp;
            for (size_t j = 0; j < matches.size(); ++j)
                if (i == matches[j].size()) { tmp.push_back((int)j); matchedCount++; }
            matchedPlanes.push_back(tmp);
            if (matchedCount >= max_candidates) break;
        }
    }
    // util.cpp:449-519 penetration filter
    struct Result { std::vector<std::pair<int, int>> mp; M3 R; V3 T; int src_index; };
    std::vector<Result> results;
    std::vector<int> tested, penflag;
    {
        int count = 0;
        bool stop = false;
        for (size_t m = 0; m < matchedPlanes.size() && !stop; ++m)
            for (size_t i = 0; i < matchedPlanes[m].size(); ++i) {
                if (count++ > max_candidates) { stop = true; break; }
                int index = matchedPlanes[m][i];
                if (pen_stride > 1 && (int)tested.size() % pen_stride != 0) {   // sampled run: candidate not evaluated
                    tested.push_back(index);
                    penflag.push_back(-1);
                    continue;
                }
                float T16[16];
                make_T(Rs[index], Ts[index], T16);
                bool isPen = false;
                for (int i1 = 0; i1 < ps; ++i1) {
                    isPen = false;
                    V3 n1 = C.normals[i1];
                    V3 pn = mul(Rs[index], n1);
                    float plane1[4] = {pn.x, pn.y, pn.z, 0};
                    plane1[3] = -(-C.coef[4 * (size_t)i1 + 3] + dot_seq(pn, Ts[index]));
                    const PlaneInfo &sp = C.planes[i1];
                    std::vector<V3> tp(sp.ds.size());
                    for (size_t q = 0; q < tp.size(); ++q) tp[q] = pcl_transform(T16, sp.ds[q]);
                    V3 four[4];
                    for (int q = 0; q < 4; ++q) four[q] = pcl_transform(T16, sp.four[q]);
                    GridIndex tg;
                    bool built = false;
                    V3 c2m = mul(Rs[index], sp.center) + Ts[index];
                    for (int j1 = 0; j1 < pt; ++j1) {
                        V3 plane_A = M.normals[j1];
                        double c2p = (std::fabs(dot(plane_A, c2m) + M.coef[4 * (size_t)j1 + 3]) +
                                      std::fabs(dot(pn, M.planes[j1].center) + plane1[3])) / 2;
                        if (c2p < lengthThreshold && dot(pn, plane_A) > angleThreshold) continue;
                        if (!built) { tg.build(tp.data(), (int)tp.size(), lengthThreshold); built = true; }
                        if (0 != planes_penetrable(plane1, &M.coef[4 * (size_t)j1], four, M.planes[j1].four, tp, tg,
                                                   M.planes[j1].ds, M.planes[j1].grid, isPen,
                                                   (float)(double)lengthThreshold, 10,
                                                   (float)((double)lengthThreshold / 2)))
                            continue;
                        if (isPen) break;
                    }
                    if (isPen) break;
                }
                tested.push_back(index);
                penflag.push_back(isPen ? 1 : 0);
                if (isPen) continue;
                Result r;
                r.mp = matches[index]; r.R = Rs[index]; r.T = Ts[index]; r.src_index = index;
                results.push_back(r);
            }
    }
    h->put("pen_tested", tested.data(), tested.size());
    {
        std::vector<float> pc(12 * tested.size());
        for (size_t i = 0; i < tested.size(); ++i) {
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) pc[12 * i + 3 * r + c] = Rs[tested[i]].m[r][c];
            st3(&pc[12 * i + 9], Ts[tested[i]]);
        }
        h->put("pen_candidates", pc.data(), pc.size());
    }
    h->put("pen_flags", penflag.data(), penflag.size());
    lap("penetration");
    if (pen_stride > 1 || results.empty()) {   // a sampled run ends here: the verification needs every flag
        h->put("timing", tim.data(), tim.size());
        h->put("timing_names", tim_names.data(), tim_names.size());
        return 0;
    }

    // plade.cpp:545-575 verification
    GridIndex tg;
    tg.build(M.ds.data(), (int)M.ds.size(), downSampleDistance * 4.f);
    std::vector<LengthIndex> ov(results.size());
    std::vector<int> counts(results.size());
    std::vector<float> cand(results.size() * 16), centers(results.size() * 3);
    for (size_t i = 0; i < results.size(); ++i) {
        float T16[16];
        make_T(results[i].R, results[i].T, T16);
        memcpy(&cand[16 * i], T16, 64);
        V3 cc = mul(results[i].R, C.bcenter) + results[i].T;
        st3(&centers[3 * i], cc);
        int cnt = overlap_count(C.ds, tg, M.ds, T16, cc, (float)C.radius, downSampleDistance);
        counts[i] = cnt;
        float ratio = 0.f;
        if (cnt >= 0) ratio = (float)(double(cnt) / std::min(C.ds.size(), M.ds.size()));
        ov[i].index = (int)i;
        ov[i].length = (float)(0.2 * (results[i].mp.size() / double(ps)) + 0.8 * ratio);
    }
    h->put("candidates", cand.data(), cand.size());
    h->put("candidate_centers", centers.data(), centers.size());
    h->put("overlap_counts", counts.data(), counts.size());
    {
        std::vector<float> sc(ov.size());
        for (size_t i = 0; i < ov.size(); ++i) sc[i] = ov[i].length;
        h->put("scores", sc.data(), sc.size());
    }
    std::sort(ov.begin(), ov.end(), cmp_greater);
    int best = ov[0].index;
    make_T(results[best].R, results[best].T, T16_out);
    h->put1("best_index", best);
    lap("verify");
    h->put("timing", tim.data(), tim.size());
    h->put("timing_names", tim_names.data(), tim_names.size());
    return 1;
}

}  // extern "C"
