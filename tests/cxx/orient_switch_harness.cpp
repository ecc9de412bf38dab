// tests/cxx/orient_switch_harness.cpp -- what plade_amd/csrc/cli_switches.h makes of values of PLADE_CONSISTENT_NORMALS, in one
// process.  Reads "<variable>\t<text>" lines from stdin ("<variable>" alone: the variable is unset) and prints one
// "<radius as %a> <mode> <inward>\t<warning>" line for each, the warning empty when the value was accepted.
// tests/test_orient_host.py holds the expected lines.
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
        if (var != "PLADE_CONSISTENT_NORMALS") return 2;
        const Parsed<OrientSwitch> p = parse_consistent_normals(text);
        printf("%a %d %d\t%s\n", p.value.radius, p.value.mode, p.value.inward, p.warning.c_str());
    }
    return 0;
}
