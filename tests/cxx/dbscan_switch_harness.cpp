// tests/cxx/dbscan_switch_harness.cpp -- what plade_amd/csrc/cli_switches.h makes of values of PLADE_DBSCAN and PLADE_M3C2_CLUSTERS,
// in one process.  Reads "<variable>\t<text>" lines from stdin ("<variable>" alone: the variable is unset) and prints one
// "<on> <radius> <min_points> <min_size> <keep_largest>\t<warning>" line for each (the radius as %.17g, which reads back to the same
// double; the warning empty when the value was accepted).  tests/test_dbscan_host.py compares the lines with its table.
#include "cli_switches.h"

#include <cstdio>
#include <iostream>

using namespace cli_switches;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        const size_t tab = line.find('\t');
        const std::string var = line.substr(0, tab);
        const char *text = tab == std::string::npos ? nullptr : line.c_str() + tab + 1;
        Parsed<DbscanSwitch> p;
        if (var == "PLADE_DBSCAN") p = parse_dbscan(text);
        else if (var == "PLADE_M3C2_CLUSTERS") p = parse_m3c2_clusters(text);
        else return 2;
        const DbscanSwitch &s = p.value;
        printf("%d %.17g %d %d %d\t%s\n", (int)s.on, s.radius, s.min_points, s.min_size, s.keep_largest, p.warning.c_str());
    }
    return 0;
}
