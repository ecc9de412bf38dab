// plade_amd/csrc/cli_switches.h -- the list-valued environment switches of the C++ API / CLI: one parser, the field predicates
// and one pure function per switch.  Host only and included by plade_host.cpp alone; nothing here reads the environment or
// prints: plade_host.cpp holds one latch per switch (getenv once per process, the warning to std::cerr) and, in the comment
// block of that latch, the switch's documentation.
//
// A value is a comma-separated list of fields, read left to right.  A field is a real (strtod) or an integer (strtol, base 10)
// that its predicate accepts; what strtod / strtol accept is accepted (leading white space, "+5", hex floats, "inf" and "nan"
// -- the predicates then reject those two).  The first `required` fields must be there, the later ones keep their defaults
// when absent.  Reading stops at the first field that fails, and whatever is left behind the last field fails the whole
// value: "5.0" is no integer because of the ".0", a trailing comma is no empty field.  A value that fails gives the switch's
// "off" and one warning, `warning: NAME=<text><tail>`.
#pragma once

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>

namespace cli_switches {

// ---- the predicates of the real fields, each in the arithmetic of what consumes the value ----
// a search radius of the fp32 grid tools: its fp32 square is finite and not below FLT_MIN
inline bool radius_sq32(double r) {
    const float rf = (float)r;
    return std::isfinite(r) && rf > 0.f && std::isfinite(rf * rf) && rf * rf >= FLT_MIN;
}
// M3C2's radius: the square is taken in fp64
inline bool radius_sq64(double r) { return std::isfinite(r) && r > 0.0 && std::isfinite(r * r); }
inline bool positive(double v) { return std::isfinite(v) && v > 0.0; }
inline bool positive_f32(double v) { return positive((double)(float)v); }      // (a distance handed on as a float)
inline bool non_negative(double v) { return std::isfinite(v) && v >= 0.0; }    // (-0 passes)
inline bool non_negative_f32(double v) { return non_negative((double)(float)v); }
// >= 0 with a finite fp32 square: the components' radius (0 = off) and FPFH's max_ratio (0 = no ratio test)
inline bool non_negative_sq32(double v) { return non_negative(v) && std::isfinite((float)v * (float)v); }
// the smoothing radius: 0 = off, otherwise what plade_smooth_cloud accepts
inline bool smooth_radius(double r) {
    const float r2 = (float)r * (float)r;
    return non_negative(r) && std::isfinite(r2) && (r == 0.0 || r2 >= FLT_MIN);
}
// the spacing of a subsample and the radius of the consistent orientation: 0 = off, otherwise what plade_subsample_spacing and
// plade_orient_normals accept
inline bool spacing_or_off(double r) { return r == 0.0 || radius_sq32(r); }
// the RANSAC pose's inlier distance: its fp64 square is finite and > 0
inline bool inlier_dist(double v) { return positive(v) && std::isfinite(v * v) && v * v > 0.0; }
inline bool epsilon(double v) { return positive(v) && v <= 1.0; }

// ---- the parser ----
struct Field {
    bool (*real)(double);   // the predicate of a real field; nullptr: an integer in [lo, hi]
    long lo, hi;
};
constexpr Field real(bool (*predicate)(double)) { return {predicate, 0, 0}; }
constexpr Field integer(long lo, long hi = INT32_MAX) { return {nullptr, lo, hi}; }
struct Value { double r; long i; };   // of a field: r when it is a real, i when it is an integer
struct Spec { const char *name; const Field *fields; int n, required; const char *tail; };

// v: n values holding the defaults.  true: the fields that are there have replaced theirs; false: the value is rejected (v is
// then partly overwritten: take the switch's "off") and, when there was a text at all, `warning` says so
inline bool parse(const Spec &s, const char *text, Value *v, std::string &warning) {
    if (!text) return false;
    const char *p = text;
    char *end = nullptr;
    int count = 0;
    bool ok = true;
    while (ok && count < s.n) {
        const Field &f = s.fields[count];
        if (f.real) { v[count].r = strtod(p, &end); ok = end != p && f.real(v[count].r); }
        else { v[count].i = strtol(p, &end, 10); ok = end != p && v[count].i >= f.lo && v[count].i <= f.hi; }
        ++count;
        if (*end != ',') break;
        p = end + 1;
    }
    if (ok && count >= s.required && *end == '\0') return true;
    warning = std::string("warning: ") + s.name + "=" + text + s.tail;
    return false;
}

template <class S> struct Parsed { S value; std::string warning; };   // warning: empty when the value was accepted (or unset)

// ---- the switches (text: the variable's value, nullptr when it is unset) ----
struct GicpSwitch { bool on = false; double epsilon = 0.0; };
inline Parsed<GicpSwitch> parse_refine_gicp(const char *text) {
    static const Field f[] = {integer(0, 1), real(epsilon)};
    static const Spec spec = {"PLADE_REFINE_GICP", f, 2, 1, " is not 0, 1 or 1,<epsilon> with 0 < epsilon <= 1; no refinement"};
    Parsed<GicpSwitch> p;
    Value v[2] = {};
    if (parse(spec, text, v, p.warning)) { p.value.on = v[0].i == 1; p.value.epsilon = v[1].r; }
    return p;
}

inline Parsed<float> parse_evaluate(const char *text) {   // 0: off
    static const Field f[] = {real(positive_f32)};
    static const Spec spec = {"PLADE_EVALUATE", f, 1, 1, " is not a positive finite distance; no evaluation"};
    Parsed<float> p{0.f, {}};
    Value v[1] = {};
    if (parse(spec, text, v, p.warning)) p.value = (float)v[0].r;
    return p;
}

struct M3c2Switch { bool on = false; double radius = 0.0, depth = 0.0, reg_error = 0.0; int min_points = 4; };
inline Parsed<M3c2Switch> parse_m3c2(const char *text) {
    static const Field f[] = {real(radius_sq64), real(positive), integer(2), real(non_negative)};
    static const Spec spec = {"PLADE_M3C2", f, 4, 2,
                              " is not <radius>,<depth>[,<min_points>[,<reg_error>]] with radius > 0, depth > 0, min_points >= 2 and reg_error >= 0;"
                              " no comparison"};
    Parsed<M3c2Switch> p;
    Value v[4] = {{}, {}, {0.0, p.value.min_points}, {p.value.reg_error, 0}};
    if (parse(spec, text, v, p.warning)) {
        M3c2Switch &s = p.value;
        s.on = true; s.radius = v[0].r; s.depth = v[1].r; s.min_points = (int)v[2].i; s.reg_error = v[3].r;
    }
    return p;
}

struct FpfhSwitch { bool on = false; double radius = 0.0; int min_pairs = 5; float max_ratio = 0.f; };
inline Parsed<FpfhSwitch> parse_fpfh_match(const char *text) {
    static const Field f[] = {real(radius_sq32), integer(1), real(non_negative_sq32)};
    static const Spec spec = {"PLADE_FPFH_MATCH", f, 3, 1,
                              " is not <radius>[,<min_pairs>[,<max_ratio>]] with radius > 0, min_pairs >= 1 and max_ratio >= 0; no descriptors"};
    Parsed<FpfhSwitch> p;
    Value v[3] = {{}, {0.0, p.value.min_pairs}, {p.value.max_ratio, 0}};
    if (parse(spec, text, v, p.warning)) {
        FpfhSwitch &s = p.value;
        s.on = true; s.radius = v[0].r; s.min_pairs = (int)v[1].i; s.max_ratio = (float)v[2].r;
    }
    return p;
}

struct FeatureRegisterSwitch { bool on = false; double radius = 0.0, inlier_dist = 0.0; int min_inliers = 3, hypotheses = 65536; };
inline Parsed<FeatureRegisterSwitch> parse_feature_register(const char *text) {
    static const Field f[] = {real(radius_sq32), real(inlier_dist), integer(3), integer(1, 1L << 24)};
    static const Spec spec = {"PLADE_FEATURE_REGISTER", f, 4, 2,
                              " is not <radius>,<inlier_dist>[,<min_inliers>[,<hypotheses>]] with radius > 0, inlier_dist > 0, min_inliers >= 3"
                              " and 1 <= hypotheses <= 16777216; no feature registration"};
    Parsed<FeatureRegisterSwitch> p;
    Value v[4] = {{}, {}, {0.0, p.value.min_inliers}, {0.0, p.value.hypotheses}};
    if (parse(spec, text, v, p.warning)) {
        FeatureRegisterSwitch &s = p.value;
        s.on = true; s.radius = v[0].r; s.inlier_dist = v[1].r; s.min_inliers = (int)v[2].i; s.hypotheses = (int)v[3].i;
    }
    return p;
}

struct KeypointSwitch { bool on = false; double salient_radius = 0.0, non_max_radius = 0.0; int min_neighbours = 5; };
inline Parsed<KeypointSwitch> parse_feature_keypoints(const char *text) {
    static const Field f[] = {real(radius_sq32), real(radius_sq32), integer(1)};
    static const Spec spec = {"PLADE_FEATURE_KEYPOINTS", f, 3, 1,
                              " is not <salient_radius>[,<non_max_radius>[,<min_neighbours>]] with both radii > 0 and min_neighbours >= 1;"
                              " no keypoints"};
    Parsed<KeypointSwitch> p;
    Value v[3] = {{}, {p.value.non_max_radius, 0}, {0.0, p.value.min_neighbours}};
    if (parse(spec, text, v, p.warning)) {
        KeypointSwitch &s = p.value;
        s.on = true; s.salient_radius = v[0].r; s.non_max_radius = v[1].r; s.min_neighbours = (int)v[2].i;
    }
    return p;
}

struct OutlierSwitch { int k = 0; double alpha = 1.0; };
inline Parsed<OutlierSwitch> parse_remove_outliers(const char *text) {
    static const Field f[] = {integer(0, 64), real(non_negative)};
    static const Spec spec = {"PLADE_REMOVE_OUTLIERS", f, 2, 1, " is not <k>[,<alpha>] with k in [1, 64] and alpha >= 0; no outlier removal"};
    Parsed<OutlierSwitch> p;
    Value v[2] = {{}, {p.value.alpha, 0}};
    if (parse(spec, text, v, p.warning)) { p.value.k = (int)v[0].i; p.value.alpha = v[1].r; }
    return p;
}

struct ComponentSwitch { double radius = 0.0; int min_size = 1, keep_largest = 0; };
inline Parsed<ComponentSwitch> parse_keep_components(const char *text) {
    static const Field f[] = {real(non_negative_sq32), integer(1), integer(0)};
    static const Spec spec = {"PLADE_KEEP_COMPONENTS", f, 3, 1,
                              " is not <radius>[,<min_size>[,<keep_largest>]] with radius >= 0, min_size >= 1 and keep_largest >= 0; no component filter"};
    Parsed<ComponentSwitch> p;
    Value v[3] = {{}, {0.0, p.value.min_size}, {0.0, p.value.keep_largest}};
    if (parse(spec, text, v, p.warning)) { p.value.radius = v[0].r; p.value.min_size = (int)v[1].i; p.value.keep_largest = (int)v[2].i; }
    return p;
}

// <radius>,<min_points>[,<min_size>[,<keep_largest>]] of PLADE_DBSCAN and <radius>[,<min_points>[,<min_size>]] of PLADE_M3C2_CLUSTERS
struct DbscanSwitch { bool on = false; double radius = 0.0; int min_points = 4, min_size = 1, keep_largest = 0; };
inline Parsed<DbscanSwitch> parse_dbscan(const char *text) {
    static const Field f[] = {real(radius_sq32), integer(1), integer(1), integer(0)};
    static const Spec spec = {"PLADE_DBSCAN", f, 4, 2,
                              " is not <radius>,<min_points>[,<min_size>[,<keep_largest>]] with radius > 0 (its square not below FLT_MIN),"
                              " min_points >= 1, min_size >= 1 and keep_largest >= 0; no clustering"};
    Parsed<DbscanSwitch> p;
    Value v[4] = {{}, {0.0, p.value.min_points}, {0.0, p.value.min_size}, {0.0, p.value.keep_largest}};
    if (parse(spec, text, v, p.warning)) {
        DbscanSwitch &s = p.value;
        s.on = true; s.radius = v[0].r; s.min_points = (int)v[1].i; s.min_size = (int)v[2].i; s.keep_largest = (int)v[3].i;
    }
    return p;
}
inline Parsed<DbscanSwitch> parse_m3c2_clusters(const char *text) {
    static const Field f[] = {real(radius_sq32), integer(1), integer(1)};
    static const Spec spec = {"PLADE_M3C2_CLUSTERS", f, 3, 1,
                              " is not <radius>[,<min_points>[,<min_size>]] with radius > 0 (its square not below FLT_MIN), min_points >= 1"
                              " and min_size >= 1; no clusters of change"};
    Parsed<DbscanSwitch> p;
    Value v[3] = {{}, {0.0, p.value.min_points}, {0.0, p.value.min_size}};
    if (parse(spec, text, v, p.warning)) {
        DbscanSwitch &s = p.value;
        s.on = true; s.radius = v[0].r; s.min_points = (int)v[1].i; s.min_size = (int)v[2].i;
    }
    return p;
}

struct SmoothSwitch { double radius = 0.0; int min_neighbours = 6; };
inline Parsed<SmoothSwitch> parse_smooth(const char *text) {
    static const Field f[] = {real(smooth_radius), integer(3)};
    static const Spec spec = {"PLADE_SMOOTH", f, 2, 1,
                              " is not <radius>[,<min_neighbours>] with radius >= 0 (its square not below FLT_MIN) and min_neighbours >= 3; no smoothing"};
    Parsed<SmoothSwitch> p;
    Value v[2] = {{}, {0.0, p.value.min_neighbours}};
    if (parse(spec, text, v, p.warning)) { p.value.radius = v[0].r; p.value.min_neighbours = (int)v[1].i; }
    return p;
}

// <spacing>[,<seed>] of PLADE_SUBSAMPLE and PLADE_M3C2_CORE: spacing 0 = off
struct SubsampleSwitch { double spacing = 0.0; uint64_t seed = 0; };
inline Parsed<SubsampleSwitch> parse_spacing_seed(const Spec &spec, const char *text) {
    Parsed<SubsampleSwitch> p;
    Value v[2] = {};
    if (parse(spec, text, v, p.warning)) { p.value.spacing = v[0].r; p.value.seed = (uint64_t)v[1].i; }
    return p;
}
constexpr Field spacing_seed_fields[] = {real(spacing_or_off), integer(0, LONG_MAX)};
inline Parsed<SubsampleSwitch> parse_subsample(const char *text) {
    static const Spec spec = {"PLADE_SUBSAMPLE", spacing_seed_fields, 2, 1,
                              " is not <spacing>[,<seed>] with spacing >= 0 (its square not below FLT_MIN) and seed an integer >= 0; no subsampling"};
    return parse_spacing_seed(spec, text);
}
inline Parsed<SubsampleSwitch> parse_m3c2_core(const char *text) {
    static const Spec spec = {"PLADE_M3C2_CORE", spacing_seed_fields, 2, 1,
                              " is not <spacing>[,<seed>] with spacing >= 0 (its square not below FLT_MIN) and seed an integer >= 0;"
                              " the whole target as core points"};
    return parse_spacing_seed(spec, text);
}

// <r_min>,<r_max>[,<scales>[,<mode>]] of PLADE_M3C2_NORMALS: S radii r_min + (r_max - r_min) * s / (S - 1) in fp64, which
// plade_cloud_scale_features accepts only with strictly ascending fp32 squares; a value whose radii are not is rejected like one
// that does not parse
struct ScaleSwitch { bool on = false; int scales = 4, mode = 0; double radii[8] = {}; };
inline Parsed<ScaleSwitch> parse_m3c2_normals(const char *text) {
    static const Field f[] = {real(radius_sq32), real(radius_sq32), integer(2, 8), integer(0, 1)};
    static const Spec spec = {"PLADE_M3C2_NORMALS", f, 4, 2,
                              " is not <r_min>,<r_max>[,<scales>[,<mode>]] with 0 < r_min < r_max (the fp32 squares of the radii strictly"
                              " ascending), scales in [2, 8] and mode 0 or 1; the core points keep their normals"};
    Parsed<ScaleSwitch> p;
    Value v[4] = {{}, {}, {0.0, p.value.scales}, {0.0, p.value.mode}};
    if (!parse(spec, text, v, p.warning)) return p;
    ScaleSwitch s;
    s.on = true; s.scales = (int)v[2].i; s.mode = (int)v[3].i;
    for (int t = 0; t < s.scales; ++t) {
        s.radii[t] = v[0].r + (v[1].r - v[0].r) * t / (s.scales - 1);
        const float r = (float)s.radii[t], q = t ? (float)s.radii[t - 1] : 0.f;
        if (t && !(q * q < r * r)) {
            p.warning = std::string("warning: ") + spec.name + "=" + text + spec.tail;
            return p;
        }
    }
    p.value = s;
    return p;
}

// <radius>[,<mode>[,<inward>]] of PLADE_CONSISTENT_NORMALS: radius 0 = off; mode 0 = vote against the origin, 1 = extreme point along +z
struct OrientSwitch { double radius = 0.0; int mode = 0, inward = 0; };
inline Parsed<OrientSwitch> parse_consistent_normals(const char *text) {
    static const Field f[] = {real(spacing_or_off), integer(0, 1), integer(0, 1)};
    static const Spec spec = {"PLADE_CONSISTENT_NORMALS", f, 3, 1,
                              " is not <radius>[,<mode>[,<inward>]] with radius >= 0 (its square not below FLT_MIN), mode 0 or 1 and inward 0 or 1;"
                              " no orientation"};
    Parsed<OrientSwitch> p;
    Value v[3] = {};
    if (parse(spec, text, v, p.warning)) { p.value.radius = v[0].r; p.value.mode = (int)v[1].i; p.value.inward = (int)v[2].i; }
    return p;
}

inline Parsed<float> parse_merge(const char *text) {   // < 0: off
    static const Field f[] = {real(non_negative_f32)};
    static const Spec spec = {"PLADE_MERGE", f, 1, 1, " is not a finite leaf size >= 0; no merge"};
    Parsed<float> p{-1.f, {}};
    Value v[1] = {};
    if (parse(spec, text, v, p.warning)) p.value = (float)v[0].r;
    return p;
}

}  // namespace cli_switches
