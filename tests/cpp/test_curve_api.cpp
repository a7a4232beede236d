// Known answers of apply_curve / interpolate / quantile_mapping_curve / monotonize_curve through the C++ host mirror
// (gridpp_amd/host/gridpp.hpp), written as code for gridpp.h would call them.  The numbers are cases of
// tests/golden/curve_known_answers.json (named in the comments).  Built and run by tests/test_gpu_curve_cpp.py.
#include "gridpp.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace gridpp;

static int failures = 0;
static void expect(bool ok, const char* what) {
    if(!ok) { std::printf("FAIL: %s\n", what); failures++; }
}
static bool eq(float a, float b) { return (std::isnan(a) && std::isnan(b)) || a == b; }   // exact, as the reference's tests
static bool eq(const vec& a, const vec& b) {
    if(a.size() != b.size()) return false;
    for(size_t i = 0; i < a.size(); i++) if(!eq(a[i], b[i])) return false;
    return true;
}
static bool eq(const vec2& a, const vec2& b) {
    if(a.size() != b.size()) return false;
    for(size_t i = 0; i < a.size(); i++) if(!eq(a[i], b[i])) return false;
    return true;
}
static bool near(float a, float b, float tol) { return std::fabs(a - b) <= tol; }
template <class E, class F>
static bool throws(F f) {
    try { f(); } catch(const E&) { return true; } catch(...) { return false; }
    return false;
}

int main() {
    const float nan = std::nanf("");
    const vec x = {1, 2, 3}, y = {2, 5, 6};
    // apply_extrapolation_1d_* (tests/test_apply_curve.py:74-78), vector and scalar forms
    const Extrapolation policies[5] = {OneToOne, Zero, MeanSlope, NearestSlope, Unchanged};
    const vec expected[5] = {{1, 7}, {2, 6}, {0, 8}, {-1, 7}, {0, 4}};
    for(int p = 0; p < 5; p++) {
        expect(eq(apply_curve(vec{0, 4}, y, x, policies[p], policies[p]), expected[p]), "apply_extrapolation_1d");
        expect(eq(apply_curve(vec2{{0}, {4}}, y, x, policies[p], policies[p]), vec2{{expected[p][0]}, {expected[p][1]}}), "apply_extrapolation_2d");
        expect(eq(apply_curve(0.0f, y, x, policies[p], policies[p]), expected[p][0]) && eq(apply_curve(4.0f, y, x, policies[p], policies[p]), expected[p][1]),
               "apply_extrapolation, scalar form");
    }
    // apply_edge_* (:59-67)
    for(float val : {1.0f, 3.0f})
        for(Extrapolation p : {OneToOne, Zero, MeanSlope, NearestSlope})
            expect(eq(apply_curve(vec{val}, vec{2, 3, 4}, x, p, p), vec{val + 1}), "apply_edge");
    // apply_train_0 / _1, apply_negative (tests/test_quantile_mapping.py:13,23)
    expect(eq(apply_curve(vec{2, 3, 4}, vec{1, 2, 3}, vec{2, 3, 4}, OneToOne, OneToOne), vec{1, 2, 3}), "apply_train_0");
    expect(eq(apply_curve(vec{2, 3, 4}, vec{1, 1, 1}, vec{2, 3, 4}, OneToOne, OneToOne), vec{1, 1, 1}), "apply_train_1");
    // one curve per cell: the same curve in every cell reproduces the shared-curve answer; a second curve in one cell changes only that cell
    {
        vec3 cr(2, vec2(2, y)), cf(2, vec2(2, x));
        cr[1][0] = {10, 20, 30};
        const vec2 in = {{0, 1.5f}, {2.5f, 4}};
        expect(eq(apply_curve(in, cr, cf, MeanSlope, NearestSlope), vec2{{0, 3.5f}, {25, 7}}), "apply_curve, one curve per cell");
    }
    // apply_empty_fcst_1d / _2d (:52-57)
    expect(apply_curve(vec(), vec{1, 2}, vec{1, 2}, OneToOne, OneToOne).empty(), "apply_empty_fcst_1d");
    expect(eq(apply_curve(vec2{{}}, vec{1, 2}, vec{1, 2}, OneToOne, OneToOne), vec2{{}}), "apply_empty_fcst_2d");
    // apply_empty_curve_*, apply_invalid_curve_*, apply_invalid_policy, apply_3d_* (:9-47,106-112)
    expect(throws<std::invalid_argument>([&] { apply_curve(0.0f, vec(), vec(), OneToOne, OneToOne); }), "apply_empty_curve_scalar");
    expect(throws<std::invalid_argument>([&] { apply_curve(vec{0, 1}, vec{1, 2}, vec(), OneToOne, OneToOne); }), "apply_empty_curve_vector");
    expect(throws<std::invalid_argument>([&] { apply_curve(vec2{{0}, {1}}, vec{1, 2, 3}, vec{1, 2}, OneToOne, OneToOne); }), "apply_invalid_curve_grid");
    expect(throws<std::invalid_argument>([&] { apply_curve(3.0f, vec{3, 4, 5}, vec{0, 1, 2}, (Extrapolation)-1, (Extrapolation)-1); }), "apply_invalid_policy");
    expect(throws<std::invalid_argument>([&] { apply_curve(vec{1}, vec{3, 4, 5}, vec{0, 1, 2}, (Extrapolation)-1, OneToOne); }),
           "array form: unknown policy whatever the data");
    expect(throws<std::invalid_argument>([&] { apply_curve(vec2(2, vec(4, 0)), vec3(2, vec2(3, vec(4, 0))), vec3(2, vec2(3, vec(4, 0))), OneToOne, OneToOne); }),
           "apply_3d_fcst_shape");
    expect(throws<std::invalid_argument>([&] { apply_curve(vec2(2, vec(3, 0)), vec3(2, vec2(3, vec(3, 0))), vec3(2, vec2(3, vec(4, 0))), OneToOne, OneToOne); }),
           "apply_3d_curve_ref_shape");

    // interp_basic_*, interp_single_*, interp_empty_*, interp_nan, interp_duplicates_* (tests/test_interpolate.py)
    const vec ix = {0, 1, 2}, iy = {0, 2, 1};
    expect(eq(interpolate(0.0f, ix, iy), 0) && eq(interpolate(2.0f, ix, iy), 1) && eq(interpolate(1.0f, ix, iy), 2), "interp_basic, on the points");
    expect(near(interpolate(0.5f, ix, iy), 1, 1e-7f) && near(interpolate(0.9f, ix, iy), 1.8f, 1e-6f) && near(interpolate(1.5f, ix, iy), 1.5f, 1e-7f), "interp_basic, between");
    expect(eq(interpolate(-1.0f, ix, iy), 0) && eq(interpolate(3.0f, ix, iy), 1), "interp_basic, outside");
    expect(eq(interpolate(-1.0f, vec{0}, vec{0}), 0) && eq(interpolate(1.0f, vec{0}, vec{0}), 0), "interp_single");
    expect(std::isnan(interpolate(0.0f, vec(), vec())) && std::isnan(interpolate(nan, vec{0}, vec{0})), "interp_empty, interp_nan");
    const vec dx = {0, 0, 0.5f, 0.5f, 1, 1}, dy = {0, 0.1f, 0.4f, 0.6f, 0.9f, 1};
    expect(near(interpolate(1.0f, dx, dy), 0.9f, 1e-7f) && near(interpolate(0.0f, dx, dy), 0.1f, 1e-7f) && near(interpolate(0.5f, dx, dy), 0.5f, 1e-7f),
           "interp_duplicates_edge");
    expect(near(interpolate(0.499999f, dx, dy), 0.4f, 1e-5f) && near(interpolate(0.500001f, dx, dy), 0.6f, 1e-5f), "interp_duplicates_middle");
    expect(near(interpolate(0.0f, vec(6, 0), dy), 0.5f, 1e-5f), "interp_duplicates_all");
    {
        const vec got = interpolate(vec{0, 0.5f, 1, -1, 2, nan}, dx, dy);   // interp_vector and the scalar answers above through the kernel
        expect(got.size() == 6 && near(got[0], 0.1f, 1e-7f) && near(got[1], 0.5f, 1e-7f) && near(got[2], 0.9f, 1e-7f) && eq(got[3], 0) && eq(got[4], 1) &&
                   std::isnan(got[5]), "interpolate, vector form");
        expect(interpolate(vec(), dx, dy).empty(), "interp_empty_vector");
    }
    expect(throws<std::invalid_argument>([&] { interpolate(0.0f, vec{0, 1, 2}, vec{0, 1}); }), "interp_invalid_scalar");
    expect(throws<std::invalid_argument>([&] { interpolate(vec{0}, vec{0, 1, 2}, vec{0, 1}); }), "interp_invalid_vector");

    // qm_negative, qm_quantiles, qm_single_point, qm_empty, qm_dimension_mismatch, qm_invalid_quantile (tests/test_quantile_mapping.py)
    vec cf;
    expect(eq(quantile_mapping_curve(vec{1, 0, -1}, vec{2, 3, 4}, cf), vec{-1, 0, 1}) && eq(cf, vec{2, 3, 4}), "qm_negative");
    vec ref11(11), fcst11(11);
    for(int i = 0; i < 11; i++) { ref11[i] = (float)i; fcst11[i] = (float)(i + 2); }
    expect(eq(quantile_mapping_curve(ref11, fcst11, cf, vec{0.1f, 0.9f}), vec{1, 9}) && eq(cf, vec{3, 11}), "qm_quantiles");
    expect(eq(quantile_mapping_curve(vec{1}, vec{2}, cf), vec{1}) && eq(cf, vec{2}), "qm_single_point");
    expect(quantile_mapping_curve(vec(), vec(), cf, vec{0.1f, 0.9f}).empty() && cf.empty(), "qm_empty_quantiles");
    expect(throws<std::invalid_argument>([&] { quantile_mapping_curve(vec{1, 2}, vec{1, 2, 3}, cf); }), "qm_dimension_mismatch");
    expect(throws<std::invalid_argument>([&] { quantile_mapping_curve(ref11, fcst11, cf, vec{0.1f, -1}); }), "qm_invalid_quantile");

    // mono_* (tests/test_monotonize.py): monotonize_curve(y, x, curve_x) returns curve_y
    expect(eq(monotonize_curve(vec{0, 1, 2, 3}, vec{0, 1, 1, 3}, cf), vec{0, 3}) && eq(cf, vec{0, 3}), "mono_x_repeat");
    expect(eq(monotonize_curve(vec{0, 1, 2, 3}, vec{0, 0, 1, 3}, cf), vec{2, 3}) && eq(cf, vec{1, 3}), "mono_x_repeat_lower");
    expect(eq(monotonize_curve(vec{0, 1, 1, 2, 3}, vec{0, 3, 2, 1, 5}, cf), vec{0, 3}) && eq(cf, vec{0, 5}), "mono_knot");
    expect(eq(monotonize_curve(vec{0, 0, 1, 2, 3, 5, 3, 6, 7, 9}, vec{-8, -9, -7, -6, -3, -1, 0, 1, 2, 3}, cf), vec{1, 2, 3, 5, 3, 6, 7, 9}) &&
               eq(cf, vec{-7, -6, -3, -1, 0, 1, 2, 3}), "mono_lower_knot");
    expect(eq(monotonize_curve(vec{0, 1, 2, 3, 4, 5, 6, 7}, vec{0, 10, 20, 30, 25, 32, 31, 33}, cf), vec{0, 1, 2, 7}) && eq(cf, vec{0, 10, 20, 33}),
           "mono_two_knots_in_a_row");
    expect(eq(monotonize_curve(vec{0, nan, -1, 1, 2, 3, 4, 5, 6}, vec{0, nan, nan, 1, 2, 3, 4, 5, 6}, cf), vec{0, 1, 2, 3, 4, 5, 6}) &&
               eq(cf, vec{0, 1, 2, 3, 4, 5, 6}), "mono_with_missing_05");
    expect(throws<std::invalid_argument>([&] { monotonize_curve(vec(), vec(), cf); }), "mono_empty_0");
    expect(throws<std::invalid_argument>([&] { monotonize_curve(vec{1, 2, 3}, vec{1, 2}, cf); }), "mono_size_mismatch_0");

    if(failures == 0) std::printf("all checks passed\n");
    return failures ? 1 : 0;
}
