// Known answers of downscale_probability / mask_threshold_downscale_consensus / mask_threshold_downscale_quantile through the C++
// host mirror (gridpp_amd/host/gridpp.hpp), written as code for gridpp.h would call them.  The numbers are the cases of
// tests/golden/ensemble_downscaling_known_answers.json (named in the comments); smart has no known answer in the reference and is
// checked for its plain properties.  Built and run by tests/test_gpu_ensemble_downscaling_cpp.py.
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
static bool eq(const vec2& a, const vec2& b) {
    if(a.size() != b.size()) return false;
    for(size_t i = 0; i < a.size(); i++) {
        if(a[i].size() != b[i].size()) return false;
        for(size_t j = 0; j < a[i].size(); j++) if(!eq(a[i][j], b[i][j])) return false;
    }
    return true;
}
template <class E, class F>
static bool throws(F f) {
    try { f(); } catch(const E&) { return true; } catch(...) { return false; }
    return false;
}
// [E][Y][X] as the reference's tests write the cubes -> (Y, X, E)
static vec3 moveaxis(const vec3& a) {
    const size_t E = a.size(), Y = a[0].size(), X = a[0][0].size();
    vec3 o(Y, vec2(X, vec(E)));
    for(size_t e = 0; e < E; e++) for(size_t y = 0; y < Y; y++) for(size_t x = 0; x < X; x++) o[y][x][e] = a[e][y][x];
    return o;
}

int main() {
    const float nan = std::nanf("");
    const float t3 = 1.0f / 3, t23 = (float)(2. / 3);
    Grid grid1(vec2{{50, 50}, {30, 30}}, vec2{{10, 30}, {10, 30}});
    Grid grid2(vec2{{45, 45, 45}, {35, 35, 35}, {25, 25, 25}}, vec2{{5, 15, 25}, {5, 15, 25}, {5, 15, 25}});
    const vec3 values = moveaxis({{{-1, -1}, {-1, -1}}, {{0, 0}, {0, 0}}, {{1, 1}, {1, 1}}});
    const vec2 thresholds = {{-2, -0.5f, 0.5f}, {0, 1, -1}, {2, 0.5f, 0}};
    // probability_leq, probability_gt, probability_geq_nan_member, probability_lt_nan_cell
    expect(eq(downscale_probability(grid1, grid2, values, thresholds, Leq), vec2{{0, t3, t23}, {t23, 1, t3}, {1, t23, t23}}), "probability_leq");
    expect(eq(downscale_probability(grid1, grid2, values, thresholds, Gt), vec2{{1, t23, t3}, {t3, 0, t23}, {0, t3, t3}}), "probability_gt");
    vec3 v = values;
    v[1][1][0] = nan;
    expect(eq(downscale_probability(grid1, grid2, v, thresholds, Geq), vec2{{1, t23, t3}, {t23, t3, 1}, {0, t3, 1}}), "probability_geq_nan_member");
    v = values;
    v[0][0] = vec(3, nan);
    expect(eq(downscale_probability(grid1, grid2, v, thresholds, Lt), vec2{{nan, nan, t23}, {t3, t23, 0}, {1, t23, t3}}), "probability_lt_nan_cell");

    const vec3 vtrue = moveaxis({{{10, 5}, {3, 2}}, {{0, 1}, {4, 0}}, {{3, 0}, {0, 6}}});
    const vec3 vfalse(2, vec2(2, vec(3, 0)));
    const float a = 3 + 1.0f / 3, b = 2 + 1.0f / 3;
    // mask_leq_mean, mask_leq_sum, mask_gt_median, mask_lt_max, mask_geq_count_nan_threshold_value, mask_leq_quantile_025
    expect(eq(mask_threshold_downscale_consensus(grid1, grid2, vtrue, vfalse, values, thresholds, Leq, Mean), vec2{{0, a, 2}, {b, b, t23}, {b, b, t23}}),
           "mask_leq_mean");
    expect(eq(mask_threshold_downscale_consensus(grid1, grid2, vtrue, vfalse, values, thresholds, Leq, Sum), vec2{{0, 10, 6}, {7, 7, 2}, {7, 7, 2}}),
           "mask_leq_sum");
    expect(eq(mask_threshold_downscale_consensus(grid1, grid2, vtrue, vfalse, values, thresholds, Gt, Median), vec2{{3, 0, 0}, {0, 0, 0}, {0, 0, 0}}),
           "mask_gt_median");
    expect(eq(mask_threshold_downscale_consensus(grid1, grid2, vtrue, vfalse, values, thresholds, Lt, Max), vec2{{0, 10, 5}, {3, 4, 0}, {4, 4, 2}}),
           "mask_lt_max");
    vec3 tv = values;
    tv[0][1][0] = nan;
    expect(eq(mask_threshold_downscale_consensus(grid1, grid2, vtrue, vfalse, tv, thresholds, Geq, Count), vec2{{3, 3, 2}, {3, 3, 3}, {3, 3, 3}}),
           "mask_geq_count_nan_threshold_value");
    expect(eq(mask_threshold_downscale_quantile(grid1, grid2, vtrue, vfalse, values, thresholds, Leq, 0.25f), vec2{{0, 0, 0.5f}, {1.5f, 1.5f, 0}, {1.5f, 1.5f, 0}}),
           "mask_leq_quantile_025");

    // the checks the mirror adds, with the reference's exception types
    expect(throws<std::invalid_argument>([&] { downscale_probability(grid2, grid2, values, thresholds, Leq); }), "Grid size is not the same as values");
    expect(throws<std::invalid_argument>([&] { downscale_probability(grid1, grid2, values, vec2(2, vec(3, 0)), Leq); }), "threshold of the wrong size");
    expect(throws<std::invalid_argument>([&] { downscale_probability(grid1, grid2, values, thresholds, (ComparisonOperator)5); }), "Invalid comparison operator");
    expect(throws<std::invalid_argument>([&] { mask_threshold_downscale_consensus(grid1, grid2, vtrue, vec3(2, vec2(2, vec(2, 0))), values, thresholds, Leq, Mean); }),
           "cubes of different shape");
    expect(throws<std::invalid_argument>([&] { mask_threshold_downscale_quantile(grid1, grid2, vtrue, vfalse, values, thresholds, Leq, 1.5f); }),
           "quantile outside [0, 1]");
    expect(throws<std::runtime_error>([&] { mask_threshold_downscale_consensus(grid1, grid2, vtrue, vfalse, values, thresholds, Leq, Unknown); }),
           "Internal error. Cannot compute statistic");
    Grid cart(vec2{{0, 0}, {1000, 1000}}, vec2{{0, 1000}, {0, 1000}}, vec2(), vec2(), Cartesian);
    expect(throws<std::invalid_argument>([&] { downscale_probability(grid1, cart, values, vec2(2, vec(2, 0)), Leq); }), "Coordinate types must be the same");

    // smart: 3 x 3 Cartesian grid, 1 km spacing, onto itself; Barnes h = 1000 keeps every cell as a candidate
    vec2 y = {{0, 0, 0}, {1000, 1000, 1000}, {2000, 2000, 2000}}, x = {{0, 1000, 2000}, {0, 1000, 2000}, {0, 1000, 2000}};
    Grid sg(y, x, vec2(), vec2(), Cartesian);
    vec2 field = {{1, 2, 3}, {4, 5, 6}, {7, 8, 9}};
    BarnesStructure st(1000);
    expect(eq(smart(sg, sg, field, 1, st), field), "smart, num = 1: the cell itself");
    vec2 all = smart(sg, sg, field, 100, st);
    bool mean_ok = true;
    for(auto& r : all) for(float f : r) mean_ok = mean_ok && std::fabs(f - 5.0f) <= 1e-5f;
    expect(mean_ok, "smart, num > candidates: the mean of all cells");
    // num = 2 at the corner (0, 0): the two neighbours tie, the lower index (0, 1) is kept -> (1 + 2) / 2
    expect(eq(smart(sg, sg, field, 2, st)[0][0], 1.5f), "smart, tie -> lower index");
    vec2 none = smart(sg, sg, field, 0, st);
    expect(std::isnan(none[1][1]), "smart, num = 0 -> NaN");
    expect(throws<std::invalid_argument>([&] { smart(sg, sg, vec2(2, vec(3, 0)), 1, st); }), "smart: Grid size is not the same as values");

    if(failures == 0) std::printf("all checks passed\n");
    return failures ? 1 : 0;
}
