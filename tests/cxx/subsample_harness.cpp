// tests/cxx/subsample_harness.cpp -- drives subsample_cloud() of plade_amd/csrc/plade.h the way a user of the C++ API would.
// Usage: subsample_harness cloud.ply spacing seed out_rows.bin
// Writes the kept points (six floats each: x y z nx ny nz) and prints one "@subsample <n> <kept> <rounds>" line, then the same
// call in place (subset = *cloud) as "@in_place <0|1>" (1: the same points), then "@refused <0|1>" for a spacing of 0 and a
// negative one: 1 when the calls returned false and left their outputs untouched.
#include "plade.h"

#include <cstdio>
#include <cstring>
#include <iostream>

static std::vector<float> rows_of(const pcl::PointCloud<pcl::PointNormal> &c) {
    std::vector<float> r;
    for (const auto &p : c.points) {
        const float v[6] = {p.x, p.y, p.z, p.normal_x, p.normal_y, p.normal_z};
        r.insert(r.end(), v, v + 6);
    }
    return r;
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const double spacing = atof(argv[2]);
    const uint64_t seed = strtoull(argv[3], nullptr, 10);
    pcl::PointCloud<pcl::PointNormal>::Ptr cloud(new pcl::PointCloud<pcl::PointNormal>);
    if (!load_ply_cloud(argv[1], *cloud)) return 3;
    pcl::PointCloud<pcl::PointNormal> subset;
    CloudSubsample info;
    if (!subsample_cloud(cloud, subset, spacing, seed, &info)) return 5;
    std::cout << "@subsample " << info.n << " " << info.kept << " " << info.rounds << std::endl;
    const std::vector<float> rows = rows_of(subset);
    FILE *f = fopen(argv[4], "wb");
    if (!f) return 4;
    fwrite(rows.data(), 4, rows.size(), f);
    fclose(f);
    // bad input: false, the outputs untouched
    CloudSubsample kb;
    kb.kept = 77;
    pcl::PointCloud<pcl::PointNormal> keep_out;
    keep_out.points.resize(3);
    const bool refused = !subsample_cloud(cloud, keep_out, 0.0, seed, &kb) && keep_out.size() == 3 && kb.kept == 77 &&
                         !subsample_cloud(cloud, keep_out, -1.0, seed, &kb) && keep_out.size() == 3 && kb.kept == 77;
    // in place
    const bool ok = subsample_cloud(cloud, *cloud, spacing, seed);
    const std::vector<float> again = rows_of(*cloud);
    std::cout << "@in_place " << (ok && again.size() == rows.size() && memcmp(again.data(), rows.data(), rows.size() * 4) == 0 ? 1 : 0) << std::endl;
    std::cout << "@refused " << (refused ? 1 : 0) << std::endl;
    return 0;
}
