// tests/cxx/fpfh_harness.cpp -- drives describe_cloud() and match_features() of plade_amd/csrc/plade.h the way a user of the C++ API
// would.
// Usage: fpfh_harness source.ply target.ply radius min_pairs mutual max_ratio out_source.bin out_target.bin out_corr.bin
// Describes the two files' clouds, matches source -> target and writes the descriptors (33 floats per point) and the correspondences
// (two int32 per pair).  One "@info" line per cloud with the summary; "@refused <0|1> <size of features afterwards> <info.n
// afterwards>" for a call with an invalid radius, "@refused_match <0|1> <size of correspondences afterwards>" for a table that is
// no multiple of 33 floats.
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

int main(int argc, char **argv) {
    if (argc != 10) return 2;
    const double radius = atof(argv[3]);
    const int min_pairs = atoi(argv[4]);
    const bool mutual = atoi(argv[5]) != 0;
    const float max_ratio = (float)atof(argv[6]);
    pcl::PointCloud<pcl::PointNormal>::Ptr src(new pcl::PointCloud<pcl::PointNormal>), tgt(new pcl::PointCloud<pcl::PointNormal>);
    if (!load_ply_cloud(argv[1], *src) || !load_ply_cloud(argv[2], *tgt)) return 3;
    std::vector<float> fs, ft;
    CloudDescription is, it;
    if (!describe_cloud(src, radius, fs, &is, min_pairs) || !describe_cloud(tgt, radius, ft, &it, min_pairs)) return 5;
    for (const CloudDescription *s : {&is, &it}) {
        char b[200];
        snprintf(b, sizeof(b), "@info %llu %llu %.17g %u", (unsigned long long)s->n, (unsigned long long)s->described, s->mean_pairs, s->max_pairs);
        std::cout << b << std::endl;
    }
    std::vector<std::pair<int, int>> corr;
    if (!match_features(fs, ft, corr, mutual, max_ratio)) return 6;
    std::vector<int> flat;
    for (const auto &c : corr) { flat.push_back(c.first); flat.push_back(c.second); }
    if (!dump(argv[7], fs.data(), fs.size() * sizeof(float)) || !dump(argv[8], ft.data(), ft.size() * sizeof(float)) ||
        !dump(argv[9], flat.data(), flat.size() * sizeof(int)))
        return 4;
    // an invalid radius: false, `features` and `info` untouched
    const size_t before = fs.size();
    const bool refused = !describe_cloud(src, -1.0, fs, &is, min_pairs) && fs.size() == before;
    std::cout << "@refused " << (refused ? 1 : 0) << " " << fs.size() << " " << (unsigned long long)is.n << std::endl;
    std::vector<float> odd(fs.begin(), fs.begin() + 40);
    const size_t pairs_before = corr.size();
    const bool refused_match = !match_features(odd, ft, corr, mutual, max_ratio) && corr.size() == pairs_before;
    std::cout << "@refused_match " << (refused_match ? 1 : 0) << " " << corr.size() << std::endl;
    return 0;
}
