// tests/cxx/corr_pose_harness.cpp -- drives estimate_pose_from_correspondences() and register_by_features() of
// plade_amd/csrc/plade.h the way a user of the C++ API would.
// Usage: corr_pose_harness source.ply target.ply radius inlier_dist out_corr.bin out_T.bin
// register_by_features on the two files' clouds, then describe_cloud + match_features + estimate_pose_from_correspondences on the same
// clouds; writes the correspondences of the one call (two int32 per pair) and the two matrices (16 floats each, row-major: the one
// call's, then the chained calls').  One "@pose" line per estimate; "@refused_pose <0|1>" for a list that names a point that does not
// exist and "@refused_register <0|1>" for an invalid radius, each 1 when the call returned false and left its outputs untouched.
#include "plade.h"

#include <cstdio>
#include <iostream>

static bool dump(const char *path, const void *data, size_t bytes) {
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    fwrite(data, 1, bytes, f);
    fclose(f);
    return true;
}

static void line(const PoseEstimate &p) {
    char b[300];
    snprintf(b, sizeof(b), "@pose %llu %u %u %u %u %u %d %.17g %.17g", (unsigned long long)p.correspondences, p.hypotheses, p.scored,
             p.best_hypothesis, p.best_count, p.inliers, p.refinements, p.rmse, p.fitness);
    std::cout << b << std::endl;
}

int main(int argc, char **argv) {
    if (argc != 7) return 2;
    const double radius = atof(argv[3]), dist = atof(argv[4]);
    pcl::PointCloud<pcl::PointNormal>::Ptr src(new pcl::PointCloud<pcl::PointNormal>), tgt(new pcl::PointCloud<pcl::PointNormal>);
    if (!load_ply_cloud(argv[1], *src) || !load_ply_cloud(argv[2], *tgt)) return 3;
    Eigen::Matrix4f T1, T2;
    PoseEstimate p1, p2;
    std::vector<std::pair<int, int>> corr1, corr2;
    if (!register_by_features(T1, tgt, src, radius, dist, &p1, &corr1)) return 5;
    line(p1);
    std::vector<float> fs, ft;
    if (!describe_cloud(src, radius, fs) || !describe_cloud(tgt, radius, ft) || !match_features(fs, ft, corr2)) return 6;
    if (!estimate_pose_from_correspondences(T2, tgt, src, corr2, dist, &p2)) return 7;
    line(p2);
    std::vector<int> flat;
    for (const auto &c : corr1) { flat.push_back(c.first); flat.push_back(c.second); }
    float T[32];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { T[4 * r + c] = T1(r, c); T[16 + 4 * r + c] = T2(r, c); }
    if (!dump(argv[5], flat.data(), flat.size() * sizeof(int)) || !dump(argv[6], T, sizeof(T))) return 4;
    // bad input: false, the outputs untouched
    Eigen::Matrix4f Tb;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) Tb(r, c) = 7.f;
    auto untouched = [&Tb] {
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) if (Tb(r, c) != 7.f) return false;
        return true;
    };
    PoseEstimate pb;
    pb.inliers = 77;
    std::vector<std::pair<int, int>> bad = corr2;
    bad[0].second = (int)tgt->size();
    const bool r1 = !estimate_pose_from_correspondences(Tb, tgt, src, bad, dist, &pb) && untouched() && pb.inliers == 77;
    std::cout << "@refused_pose " << (r1 ? 1 : 0) << std::endl;
    std::vector<std::pair<int, int>> keep(3, {5, 5});
    const bool r2 = !register_by_features(Tb, tgt, src, -1.0, dist, &pb, &keep) && untouched() && pb.inliers == 77 &&
                    keep.size() == 3 && keep[2].first == 5;
    std::cout << "@refused_register " << (r2 ? 1 : 0) << std::endl;
    return 0;
}
