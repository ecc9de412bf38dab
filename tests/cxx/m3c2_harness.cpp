// tests/cxx/m3c2_harness.cpp -- drives compare_clouds() of plade_amd/csrc/plade.h the way a user of the C++ API would.
// Usage: m3c2_harness reference.ply compared.ply radius depth min_points reg_error tx ty tz out.bin
// Compares the two files' clouds (transformation = the translation tx ty tz, compared -> reference) and writes the distances to
// out.bin as doubles, one per point of the reference.  One "@info" line with the summary; "@refused <0|1> <size of distances
// afterwards> <info.m afterwards>" for a call with an invalid radius.
#include "plade.h"

#include <cstdio>
#include <iostream>

int main(int argc, char **argv) {
    if (argc != 11) return 2;
    const double radius = atof(argv[3]), depth = atof(argv[4]), reg_error = atof(argv[6]);
    const int min_points = atoi(argv[5]);
    pcl::PointCloud<pcl::PointNormal>::Ptr ref(new pcl::PointCloud<pcl::PointNormal>), cmp(new pcl::PointCloud<pcl::PointNormal>);
    if (!load_ply_cloud(argv[1], *ref) || !load_ply_cloud(argv[2], *cmp)) return 3;
    Eigen::Matrix4f T = Eigen::Matrix4f::Identity();
    T(0, 3) = (float)atof(argv[7]); T(1, 3) = (float)atof(argv[8]); T(2, 3) = (float)atof(argv[9]);
    std::vector<double> dist;
    CloudComparison s;
    if (!compare_clouds(T, ref, cmp, radius, depth, dist, &s, min_points, reg_error)) return 5;
    char b[280];
    snprintf(b, sizeof(b), "@info %llu %llu %llu %.17g %.17g %.17g %u", (unsigned long long)s.m, (unsigned long long)s.valid,
             (unsigned long long)s.significant, s.mean, s.rms, s.max, s.max_count);
    std::cout << b << std::endl;
    FILE *f = fopen(argv[10], "wb");
    if (!f) return 4;
    fwrite(dist.data(), sizeof(double), dist.size(), f);
    fclose(f);
    // an invalid radius: false, `distances` and `info` untouched
    const size_t before = dist.size();
    const bool refused = !compare_clouds(T, ref, cmp, -1.0, depth, dist, &s, min_points, reg_error) && dist.size() == before;
    std::cout << "@refused " << (refused ? 1 : 0) << " " << dist.size() << " " << (unsigned long long)s.m << std::endl;
    return 0;
}
