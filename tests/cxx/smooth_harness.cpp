// tests/cxx/smooth_harness.cpp -- drives smooth_cloud() of plade_amd/csrc/plade.h the way a user of the C++ API would.
// Usage: smooth_harness cloud.ply radius min_neighbours out.bin
// Smooths the file's cloud three times -- the cloud's own normals kept, the fits' normals, and in place (`smoothed` = *cloud) --
// and writes the three results to out.bin as rows of six floats (x y z nx ny nz), one block of n rows after the other.  One
// "@info" line per call with the summary; "@refused <0|1> <size of smoothed afterwards>" for a call with an invalid radius.
#include "plade.h"

#include <cstdio>
#include <iostream>

static void put(FILE *f, const pcl::PointCloud<pcl::PointNormal> &c) {
    for (size_t i = 0; i < c.size(); ++i) {
        const pcl::PointNormal &p = c.at(i);
        const float row[6] = {p.x, p.y, p.z, p.normal_x, p.normal_y, p.normal_z};
        fwrite(row, sizeof(float), 6, f);
    }
}

static void show(const CloudSmoothing &s) {
    char b[200];
    snprintf(b, sizeof(b), "@info %llu %llu %.17g %.17g %u", (unsigned long long)s.n, (unsigned long long)s.fitted, s.rms, s.max, s.max_count);
    std::cout << b << std::endl;
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const double radius = atof(argv[2]);
    const int min_nb = atoi(argv[3]);
    pcl::PointCloud<pcl::PointNormal>::Ptr cloud(new pcl::PointCloud<pcl::PointNormal>);
    if (!load_ply_cloud(argv[1], *cloud)) return 3;
    FILE *f = fopen(argv[4], "wb");
    if (!f) return 4;
    pcl::PointCloud<pcl::PointNormal> own, fit;
    CloudSmoothing s;
    if (!smooth_cloud(cloud, own, radius, min_nb, false, &s)) return 5;
    show(s);
    put(f, own);
    if (!smooth_cloud(cloud, fit, radius, min_nb, true, &s)) return 6;
    show(s);
    put(f, fit);
    // an invalid radius: false, `smoothed` untouched
    const size_t before = fit.size();
    const bool refused = !smooth_cloud(cloud, fit, -1.0, min_nb, true, nullptr) && fit.size() == before;
    std::cout << "@refused " << (refused ? 1 : 0) << " " << fit.size() << std::endl;
    if (!smooth_cloud(cloud, *cloud, radius, min_nb, false, &s)) return 7;   // in place, the default normals
    show(s);
    put(f, *cloud);
    fclose(f);
    return 0;
}
