// tests/cxx/subsample_switch_harness.cpp -- what plade_amd/csrc/cli_switches.h makes of values of PLADE_SUBSAMPLE and
// PLADE_M3C2_CORE, in one process.  Reads "<variable>\t<text>" lines from stdin ("<variable>" alone: the variable is unset) and
// prints one "<spacing as %a> <seed>\t<warning>" line for each, the warning empty when the value was accepted.
// tests/test_subsample_switches_host.py holds the expected lines.
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
        Parsed<SubsampleSwitch> p;
        if (var == "PLADE_SUBSAMPLE") p = parse_subsample(text);
        else if (var == "PLADE_M3C2_CORE") p = parse_m3c2_core(text);
        else return 2;
        printf("%a %llu\t%s\n", p.value.spacing, (unsigned long long)p.value.seed, p.warning.c_str());
    }
    return 0;
}
