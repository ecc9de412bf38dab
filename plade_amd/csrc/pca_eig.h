// plade_amd/csrc/pca_eig.h -- the closed-form fp64 eigen-solve of a 3 x 3 symmetric covariance that the PCA normals
// (k_normals.hip, pca_store) and the moving-least-squares fit (k_smooth.hip) share: one function, the same arithmetic on both.
#pragma once
#include "common.h"

namespace plade {

// fp64 3-vector helpers of the eigen-solve
struct d3 { double x, y, z; };
__device__ __forceinline__ d3 dcross(d3 u, d3 v) { return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }
__device__ __forceinline__ double ddot(d3 u, d3 v) { return u.x * v.x + u.y * v.y + u.z * v.z; }

// C = the six entries of the upper triangle.  false: C is exactly zero (nothing is written).  Otherwise n = the unit eigenvector
// of the smallest eigenvalue l0 (its sign is the caller's), tr = the trace.
__device__ __forceinline__ bool pca_eig(double c00, double c01, double c02, double c11, double c12, double c22, d3 &n, double &l0_out,
                                        double &tr_out) {
    if (c00 == 0.0 && c01 == 0.0 && c02 == 0.0 && c11 == 0.0 && c12 == 0.0 && c22 == 0.0) return false;
    // eigenvalues: trigonometric solution of det(C - l I) = 0 on the shifted, scaled matrix
    const double tr = c00 + c11 + c22, q = tr / 3.0;
    const double b00 = c00 - q, b11 = c11 - q, b22 = c22 - q;
    const double p2 = b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * (c01 * c01 + c02 * c02 + c12 * c12);
    double l0 = q;
    if (p2 > 0.0) {
        const double pp = sqrt(p2 / 6.0);
        const double i00 = b00 / pp, i11 = b11 / pp, i22 = b22 / pp, i01 = c01 / pp, i02 = c02 / pp, i12 = c12 / pp;
        double r = 0.5 * (i00 * (i11 * i22 - i12 * i12) - i01 * (i01 * i22 - i12 * i02) + i02 * (i01 * i12 - i11 * i02));
        r = fmin(1.0, fmax(-1.0, r));
        const double phi = acos(r) / 3.0;
        l0 = q + 2.0 * pp * cos(phi + 2.0943951023931954923);   // the smallest root (2 pi / 3)
    }
    // eigenvector of l0: the largest cross product of two rows of C - l0 I; when all of them vanish (a line: the
    // eigenspace of l0 is a plane) any vector orthogonal to the largest row
    const d3 r0 = {c00 - l0, c01, c02}, r1 = {c01, c11 - l0, c12}, r2 = {c02, c12, c22 - l0};
    const d3 x01 = dcross(r0, r1), x02 = dcross(r0, r2), x12 = dcross(r1, r2);
    const double n01 = ddot(x01, x01), n02 = ddot(x02, x02), n12 = ddot(x12, x12);
    d3 v = x01;
    double vn = n01;
    if (n02 > vn) { v = x02; vn = n02; }
    if (n12 > vn) { v = x12; vn = n12; }
    const double q0 = ddot(r0, r0), q1 = ddot(r1, r1), q2 = ddot(r2, r2);
    double rmax = q0;
    d3 rr = r0;
    if (q1 > rmax) { rr = r1; rmax = q1; }
    if (q2 > rmax) { rr = r2; rmax = q2; }
    if (!(vn > 1e-20 * rmax * rmax)) {
        if (rmax > 0.0) {
            const double ax = fabs(rr.x), ay = fabs(rr.y), az = fabs(rr.z);
            const d3 e = ax <= ay && ax <= az ? d3{1.0, 0.0, 0.0} : ay <= az ? d3{0.0, 1.0, 0.0} : d3{0.0, 0.0, 1.0};
            v = dcross(rr, e);
        } else {
            v = {0.0, 0.0, 1.0};   // isotropic: every direction is an eigenvector
        }
        vn = ddot(v, v);
    }
    const double s = 1.0 / sqrt(vn);
    n = {v.x * s, v.y * s, v.z * s};
    l0_out = l0;
    tr_out = tr;
    return true;
}

// The three eigenvalues l1 >= l2 >= l3 of the same matrix by the same closed form (the keypoint detector, k_keypoints.hip): q, p2,
// pp, r and phi exactly as above; the largest and the smallest root from the cosine, the middle one from the trace; then ordered
// (rounding can swap two that nearly coincide).  p2 = 0: all three are q.
__device__ __forceinline__ void sym3_eigenvalues(double c00, double c01, double c02, double c11, double c12, double c22, double &l1,
                                                 double &l2, double &l3) {
    const double tr = c00 + c11 + c22, q = tr / 3.0;
    const double b00 = c00 - q, b11 = c11 - q, b22 = c22 - q;
    const double p2 = b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * (c01 * c01 + c02 * c02 + c12 * c12);
    double lmax = q, lmid = q, lmin = q;
    if (p2 > 0.0) {
        const double pp = sqrt(p2 / 6.0);
        const double i00 = b00 / pp, i11 = b11 / pp, i22 = b22 / pp, i01 = c01 / pp, i02 = c02 / pp, i12 = c12 / pp;
        double r = 0.5 * (i00 * (i11 * i22 - i12 * i12) - i01 * (i01 * i22 - i12 * i02) + i02 * (i01 * i12 - i11 * i02));
        r = fmin(1.0, fmax(-1.0, r));
        const double phi = acos(r) / 3.0;
        lmax = q + 2.0 * pp * cos(phi);
        lmin = q + 2.0 * pp * cos(phi + 2.0943951023931954923);
        lmid = tr - lmax - lmin;
    }
    const double hi = fmax(lmax, lmid), lo = fmin(lmax, lmid);
    l1 = fmax(hi, lmin);
    l3 = fmin(lo, lmin);
    l2 = fmax(lo, fmin(hi, lmin));
}

}  // namespace plade
