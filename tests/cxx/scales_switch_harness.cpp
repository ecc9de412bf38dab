// tests/cxx/scales_switch_harness.cpp -- what plade_amd/csrc/cli_switches.h makes of values of PLADE_M3C2_NORMALS, in one process.
// Reads "<variable>\t<text>" lines from stdin ("<variable>" alone: the variable is unset) and prints one
// "<on> <scales> <mode> <radius as %a> ...\t<warning>" line for each (the radii: `scales` of them), the warning empty when the value
// was accepted.  tests/test_scales_switch_host.py holds the expected lines.
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
        if (var != "PLADE_M3C2_NORMALS") return 2;
        const Parsed<ScaleSwitch> p = parse_m3c2_normals(text);
        printf("%d %d %d", p.value.on ? 1 : 0, p.value.scales, p.value.mode);
        for (int t = 0; t < p.value.scales; ++t) printf(" %a", p.value.radii[t]);
        printf("\t%s\n", p.warning.c_str());
    }
    return 0;
}
