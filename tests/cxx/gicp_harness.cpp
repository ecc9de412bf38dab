// tests/cxx/gicp_harness.cpp -- drives refine_registration_gicp() of plade_amd/csrc/plade.h the way a user of the C++ API would.
// Usage: gicp_harness target.ply source.ply T.txt epsilon
// T.txt holds the 16 values of the start transformation (source -> target, row-major).  Prints "@ok <0|1>" and "@T" with the 16
// values of the transformation afterwards as hexadecimal floats; then calls the function again with the source moved 1000 units
// away (too few correspondences) and prints "@far <returned> <1 when the transformation is untouched>".
#include "plade.h"

#include <cstdio>
#include <iostream>

static void show(const char *tag, const Eigen::Matrix<float, 4, 4> &T) {
    std::cout << tag;
    char b[64];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            snprintf(b, sizeof(b), " %a", (double)T(r, c));
            std::cout << b;
        }
    std::cout << std::endl;
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    pcl::PointCloud<pcl::PointNormal>::Ptr target(new pcl::PointCloud<pcl::PointNormal>), source(new pcl::PointCloud<pcl::PointNormal>);
    if (!load_ply_cloud(argv[1], *target) || !load_ply_cloud(argv[2], *source)) return 3;
    FILE *f = fopen(argv[3], "r");
    if (!f) return 4;
    Eigen::Matrix<float, 4, 4> T0;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            double v;
            if (fscanf(f, "%lf", &v) != 1) return 5;
            T0(r, c) = (float)v;
        }
    fclose(f);
    const double epsilon = atof(argv[4]);
    Eigen::Matrix<float, 4, 4> T = T0;
    const bool ok = refine_registration_gicp(T, target, source, epsilon);
    std::cout << "@ok " << (ok ? 1 : 0) << std::endl;
    show("@T", T);
    // a failure: false, the transformation untouched
    for (size_t i = 0; i < source->size(); ++i) source->at(i).x += 1000.f;
    Eigen::Matrix<float, 4, 4> U = T0;
    const bool far_ok = refine_registration_gicp(U, target, source, epsilon);
    bool same = true;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) same = same && U(r, c) == T0(r, c);
    std::cout << "@far " << (far_ok ? 1 : 0) << " " << (same ? 1 : 0) << std::endl;
    return 0;
}
