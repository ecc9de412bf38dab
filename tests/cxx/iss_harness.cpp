// tests/cxx/iss_harness.cpp -- drives detect_keypoints() and register_by_keypoints() of plade_amd/csrc/plade.h the way a user of the
// C++ API would.
// Usage: iss_harness source.ply target.ply radius inlier_dist salient_radius non_max_radius out_key.bin out_corr.bin out_T.bin
// detect_keypoints on the source, then register_by_keypoints on the pair; writes the keypoints (one int32 each), the
// correspondences (two int32 per pair) and the matrix (16 floats, row-major).  One "@keypoints" line per summary, one "@pose" line;
// "@refused_detect <0|1>" for an invalid radius and for min_neighbours = 0, "@refused_register <0|1>" for an invalid inlier
// distance and for a salient radius of 0, each 1 when the calls returned false and left their outputs untouched.
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

static void line(const KeypointDetection &k) {
    char b[200];
    snprintf(b, sizeof(b), "@keypoints %llu %llu %llu %u", (unsigned long long)k.n, (unsigned long long)k.salient,
             (unsigned long long)k.keypoints, k.max_count);
    std::cout << b << std::endl;
}

int main(int argc, char **argv) {
    if (argc != 10) return 2;
    const double radius = atof(argv[3]), dist = atof(argv[4]), rs = atof(argv[5]), rn = atof(argv[6]);
    pcl::PointCloud<pcl::PointNormal>::Ptr src(new pcl::PointCloud<pcl::PointNormal>), tgt(new pcl::PointCloud<pcl::PointNormal>);
    if (!load_ply_cloud(argv[1], *src) || !load_ply_cloud(argv[2], *tgt)) return 3;
    std::vector<int> keys;
    KeypointDetection k1, k2;
    if (!detect_keypoints(src, rs, keys, &k1, rn)) return 5;
    line(k1);
    Eigen::Matrix4f T1;
    PoseEstimate p;
    std::vector<std::pair<int, int>> corr;
    if (!register_by_keypoints(T1, tgt, src, radius, dist, rs, &p, &k2, &corr, rn)) return 6;
    line(k2);
    char b[300];
    snprintf(b, sizeof(b), "@pose %llu %u %u %u %u %u %d %.17g %.17g", (unsigned long long)p.correspondences, p.hypotheses, p.scored,
             p.best_hypothesis, p.best_count, p.inliers, p.refinements, p.rmse, p.fitness);
    std::cout << b << std::endl;
    std::vector<int> flat;
    for (const auto &c : corr) { flat.push_back(c.first); flat.push_back(c.second); }
    float T[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T[4 * r + c] = T1(r, c);
    if (!dump(argv[7], keys.data(), keys.size() * sizeof(int)) || !dump(argv[8], flat.data(), flat.size() * sizeof(int)) ||
        !dump(argv[9], T, sizeof(T)))
        return 4;
    // bad input: false, the outputs untouched
    std::vector<int> keep_keys(3, 5);
    KeypointDetection kb;
    kb.keypoints = 77;
    const bool r1 = !detect_keypoints(src, -1.0, keep_keys, &kb, rn) && keep_keys.size() == 3 && keep_keys[2] == 5 && kb.keypoints == 77 &&
                    !detect_keypoints(src, rs, keep_keys, &kb, rn, 0) && keep_keys.size() == 3 && kb.keypoints == 77;
    std::cout << "@refused_detect " << (r1 ? 1 : 0) << std::endl;
    Eigen::Matrix4f Tb;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) Tb(r, c) = 7.f;
    auto untouched = [&Tb] {
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) if (Tb(r, c) != 7.f) return false;
        return true;
    };
    PoseEstimate pb;
    pb.inliers = 77;
    std::vector<std::pair<int, int>> keep(3, {5, 5});
    const bool r2 = !register_by_keypoints(Tb, tgt, src, radius, -1.0, rs, &pb, &kb, &keep, rn) && untouched() && pb.inliers == 77 &&
                    kb.keypoints == 77 && keep.size() == 3 && keep[2].first == 5 &&
                    !register_by_keypoints(Tb, tgt, src, radius, dist, 0.0, &pb, &kb, &keep, rn) && untouched() && pb.inliers == 77 &&
                    kb.keypoints == 77 && keep.size() == 3;
    std::cout << "@refused_register " << (r2 ? 1 : 0) << std::endl;
    return 0;
}
