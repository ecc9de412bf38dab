// tests/cxx/switch_harness.cpp -- what plade_amd/csrc/cli_switches.h makes of a list of values, in one process.
// Reads "<variable>\t<text>" lines from stdin ("<variable>" alone: the variable is unset) and prints one "<fields>\t<warning>"
// line for each: the fields of the parsed struct (reals as %a, integers and flags as %d, `on` first where there is one, then in
// the order of the value's grammar) and the warning, empty when the value was accepted.  tests/test_cli_switches_host.py
// compares the lines with tests/switch_cases.py.
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
        std::string warning;
        if (var == "PLADE_REFINE_GICP") { const auto p = parse_refine_gicp(text); warning = p.warning; printf("%d %a", (int)p.value.on, p.value.epsilon); }
        else if (var == "PLADE_EVALUATE") { const auto p = parse_evaluate(text); warning = p.warning; printf("%a", (double)p.value); }
        else if (var == "PLADE_M3C2") {
            const auto p = parse_m3c2(text); warning = p.warning;
            printf("%d %a %a %d %a", (int)p.value.on, p.value.radius, p.value.depth, p.value.min_points, p.value.reg_error);
        } else if (var == "PLADE_FPFH_MATCH") {
            const auto p = parse_fpfh_match(text); warning = p.warning;
            printf("%d %a %d %a", (int)p.value.on, p.value.radius, p.value.min_pairs, (double)p.value.max_ratio);
        } else if (var == "PLADE_FEATURE_REGISTER") {
            const auto p = parse_feature_register(text); warning = p.warning;
            printf("%d %a %a %d %d", (int)p.value.on, p.value.radius, p.value.inlier_dist, p.value.min_inliers, p.value.hypotheses);
        } else if (var == "PLADE_FEATURE_KEYPOINTS") {
            const auto p = parse_feature_keypoints(text); warning = p.warning;
            printf("%d %a %a %d", (int)p.value.on, p.value.salient_radius, p.value.non_max_radius, p.value.min_neighbours);
        } else if (var == "PLADE_REMOVE_OUTLIERS") { const auto p = parse_remove_outliers(text); warning = p.warning; printf("%d %a", p.value.k, p.value.alpha); }
        else if (var == "PLADE_KEEP_COMPONENTS") {
            const auto p = parse_keep_components(text); warning = p.warning;
            printf("%a %d %d", p.value.radius, p.value.min_size, p.value.keep_largest);
        } else if (var == "PLADE_SMOOTH") { const auto p = parse_smooth(text); warning = p.warning; printf("%a %d", p.value.radius, p.value.min_neighbours); }
        else if (var == "PLADE_MERGE") { const auto p = parse_merge(text); warning = p.warning; printf("%a", (double)p.value); }
        else return 2;
        printf("\t%s\n", warning.c_str());
    }
    return 0;
}
