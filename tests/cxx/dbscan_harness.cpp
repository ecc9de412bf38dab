// tests/cxx/dbscan_harness.cpp -- drives cluster_cloud() of plade_amd/csrc/plade.h the way a user of the C++ API would.
// Usage: dbscan_harness cloud.ply radius min_points min_size keep_largest out_rows.bin out_labels.bin
// Writes the kept points (six floats each: x y z nx ny nz) and the labels (one int32 per input point) and prints one
// "@dbscan <n> <clusters> <core> <border> <noise> <kept_clusters> <kept> <largest>" line, then the call with the default
// min_points, min_size and keep_largest as "@default <clusters> <kept>", then in place (filtered = *cloud) as "@in_place <0|1>"
// (1: the same points), then "@refused <0|1>" for a radius of 0 and a min_points of 0: 1 when the calls returned false and left
// their outputs untouched.
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
    if (argc != 8) return 2;
    const double radius = atof(argv[2]);
    const int min_points = atoi(argv[3]), min_size = atoi(argv[4]), keep_largest = atoi(argv[5]);
    pcl::PointCloud<pcl::PointNormal>::Ptr cloud(new pcl::PointCloud<pcl::PointNormal>);
    if (!load_ply_cloud(argv[1], *cloud)) return 3;
    pcl::PointCloud<pcl::PointNormal> filtered;
    std::vector<int32_t> labels;
    CloudClusters info;
    if (!cluster_cloud(cloud, filtered, labels, radius, min_points, min_size, keep_largest, &info)) return 5;
    std::cout << "@dbscan " << info.n << " " << info.clusters << " " << info.core << " " << info.border << " " << info.noise << " "
              << info.kept_clusters << " " << info.kept << " " << info.largest << std::endl;
    const std::vector<float> rows = rows_of(filtered);
    FILE *f = fopen(argv[6], "wb");
    if (!f) return 4;
    fwrite(rows.data(), 4, rows.size(), f);
    fclose(f);
    f = fopen(argv[7], "wb");
    if (!f) return 4;
    fwrite(labels.data(), 4, labels.size(), f);
    fclose(f);
    // the defaults: min_points 4, every cluster kept
    pcl::PointCloud<pcl::PointNormal> by_default;
    std::vector<int32_t> dl;
    CloudClusters di;
    if (!cluster_cloud(cloud, by_default, dl, radius)) return 6;
    if (!cluster_cloud(cloud, by_default, dl, radius, 4, 1, 0, &di) || dl.size() != cloud->size() || by_default.size() != di.kept) return 6;
    std::cout << "@default " << di.clusters << " " << di.kept << std::endl;
    // bad input: false, the outputs untouched
    CloudClusters kb;
    kb.kept = 77;
    pcl::PointCloud<pcl::PointNormal> keep_out;
    keep_out.points.resize(3);
    std::vector<int32_t> keep_labels(5, 9);
    const bool refused = !cluster_cloud(cloud, keep_out, keep_labels, 0.0, min_points, min_size, keep_largest, &kb) && keep_out.size() == 3 &&
                         keep_labels == std::vector<int32_t>(5, 9) && kb.kept == 77 &&
                         !cluster_cloud(cloud, keep_out, keep_labels, radius, 0, min_size, keep_largest, &kb) && keep_out.size() == 3 &&
                         keep_labels == std::vector<int32_t>(5, 9) && kb.kept == 77;
    // in place
    std::vector<int32_t> again_labels;
    const bool ok = cluster_cloud(cloud, *cloud, again_labels, radius, min_points, min_size, keep_largest);
    const std::vector<float> again = rows_of(*cloud);
    std::cout << "@in_place "
              << (ok && again_labels == labels && again.size() == rows.size() && memcmp(again.data(), rows.data(), rows.size() * 4) == 0 ? 1 : 0)
              << std::endl;
    std::cout << "@refused " << (refused ? 1 : 0) << std::endl;
    return 0;
}
