// tests/cxx/orient_harness.cpp -- drives orient_cloud_normals() of plade_amd/csrc/plade.h the way a user of the C++ API would.
// Usage: orient_harness cloud.ply radius mode inward rx ry rz out_rows.bin
// (rx ry rz: the viewpoint of mode 0, the direction of mode 1).  Writes the oriented points (six floats each: x y z nx ny nz) and
// prints one "@orient <n> <unoriented> <components> <flipped> <tree_edges> <tree_key_sum> <rounds>" line, then the same call with
// the default reference as "@default <flipped>", then in place (oriented = *cloud) as "@in_place <0|1>" (1: the same points),
// then "@refused <0|1>" for a radius of 0, a mode of 2 and a zero direction: 1 when the calls returned false and left their outputs
// untouched.
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
    if (argc != 9) return 2;
    const double radius = atof(argv[2]);
    const int mode = atoi(argv[3]);
    const bool inward = atoi(argv[4]) != 0;
    const float ref[3] = {(float)atof(argv[5]), (float)atof(argv[6]), (float)atof(argv[7])};
    pcl::PointCloud<pcl::PointNormal>::Ptr cloud(new pcl::PointCloud<pcl::PointNormal>);
    if (!load_ply_cloud(argv[1], *cloud)) return 3;
    pcl::PointCloud<pcl::PointNormal> oriented;
    NormalOrientation info;
    if (!orient_cloud_normals(cloud, oriented, radius, mode, inward, ref, &info)) return 5;
    std::cout << "@orient " << info.n << " " << info.unoriented << " " << info.components << " " << info.flipped << " " << info.tree_edges
              << " " << info.tree_key_sum << " " << info.rounds << std::endl;
    const std::vector<float> rows = rows_of(oriented);
    FILE *f = fopen(argv[8], "wb");
    if (!f) return 4;
    fwrite(rows.data(), 4, rows.size(), f);
    fclose(f);
    // the default reference: the origin (mode 0) or +z (mode 1)
    pcl::PointCloud<pcl::PointNormal> by_default;
    NormalOrientation di;
    if (!orient_cloud_normals(cloud, by_default, radius, mode, inward, nullptr, &di)) return 6;
    std::cout << "@default " << di.flipped << std::endl;
    // bad input: false, the outputs untouched
    NormalOrientation kb;
    kb.flipped = 77;
    pcl::PointCloud<pcl::PointNormal> keep_out;
    keep_out.points.resize(3);
    const float zero[3] = {0.f, 0.f, 0.f};
    const bool refused = !orient_cloud_normals(cloud, keep_out, 0.0, mode, inward, ref, &kb) && keep_out.size() == 3 && kb.flipped == 77 &&
                         !orient_cloud_normals(cloud, keep_out, radius, 2, inward, ref, &kb) && keep_out.size() == 3 && kb.flipped == 77 &&
                         !orient_cloud_normals(cloud, keep_out, radius, 1, inward, zero, &kb) && keep_out.size() == 3 && kb.flipped == 77;
    // in place
    const bool ok = orient_cloud_normals(cloud, *cloud, radius, mode, inward, ref);
    const std::vector<float> again = rows_of(*cloud);
    std::cout << "@in_place " << (ok && again.size() == rows.size() && memcmp(again.data(), rows.data(), rows.size() * 4) == 0 ? 1 : 0) << std::endl;
    std::cout << "@refused " << (refused ? 1 : 0) << std::endl;
    return 0;
}
