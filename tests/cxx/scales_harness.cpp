// tests/cxx/scales_harness.cpp -- drives multiscale_normals() of plade_amd/csrc/plade.h the way a user of the C++ API would.
// Usage: scales_harness cloud.ply mode min_neighbours out.bin radius...
// Estimates the file's normals three times -- toward the origin, along the cloud's own normals, and in place (`with_normals` =
// *cloud, toward the origin) -- and writes the three results to out.bin as rows of six floats (x y z nx ny nz), one block of n rows
// after the other.  One "@info" line per call with the summary; "@refused <0|1> <size of with_normals afterwards>" for a call with
// descending radii.
#include "plade.h"

#include <algorithm>
#include <cstdio>
#include <iostream>

static void put(FILE *f, const pcl::PointCloud<pcl::PointNormal> &c) {
    for (size_t i = 0; i < c.size(); ++i) {
        const pcl::PointNormal &p = c.at(i);
        const float row[6] = {p.x, p.y, p.z, p.normal_x, p.normal_y, p.normal_z};
        fwrite(row, sizeof(float), 6, f);
    }
}

static void show(const CloudScales &s) {
    std::cout << "@info " << s.queries << " " << s.fitted << " " << s.max_count;
    for (int t = 0; t < 8; ++t) std::cout << " " << s.chosen_hist[t];
    std::cout << std::endl;
}

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    const int mode = atoi(argv[2]), min_nb = atoi(argv[3]);
    std::vector<double> radii;
    for (int a = 5; a < argc; ++a) radii.push_back(atof(argv[a]));
    pcl::PointCloud<pcl::PointNormal>::Ptr cloud(new pcl::PointCloud<pcl::PointNormal>);
    if (!load_ply_cloud(argv[1], *cloud)) return 3;
    FILE *f = fopen(argv[4], "wb");
    if (!f) return 4;
    pcl::PointCloud<pcl::PointNormal> view, own;
    CloudScales s;
    if (!multiscale_normals(cloud, view, radii, mode, min_nb, false, &s)) return 5;
    show(s);
    put(f, view);
    if (!multiscale_normals(cloud, own, radii, mode, min_nb, true, &s)) return 6;
    show(s);
    put(f, own);
    // descending radii: false, `with_normals` untouched
    std::vector<double> down(radii);
    std::reverse(down.begin(), down.end());
    const size_t before = own.size();
    const bool refused = !multiscale_normals(cloud, own, down, mode, min_nb, true, nullptr) && own.size() == before;
    std::cout << "@refused " << (refused ? 1 : 0) << " " << own.size() << std::endl;
    if (!multiscale_normals(cloud, *cloud, radii, mode, min_nb, false, &s)) return 7;   // in place
    show(s);
    put(f, *cloud);
    fclose(f);
    return 0;
}
