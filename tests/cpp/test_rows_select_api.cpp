// calc_statistic(vec2), calc_quantile(vec2, q) and calc_quantile(vec3, vec2) through the C++ host mirror (gridpp_amd/host/gridpp.hpp),
// written as code for gridpp.h would call them: known answers, the per-row agreement with the vec forms, ragged and empty rows, the
// default quantile and the exceptions of src/api/util.cpp:113-115,188-189.  Built and run by tests/test_gpu_rows_select_cpp.py.
#include "gridpp.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace gridpp;

static int failures = 0;
static void expect(bool ok, const char* what) {
    if(!ok) { std::printf("FAIL: %s\n", what); failures++; }
}
static bool eq(float a, float b) { return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, sizeof a) == 0; }   // bit for bit
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
template <class E, class F>
static bool throws(F f) {
    try { f(); } catch(const E&) { return true; } catch(...) { return false; }
    return false;
}

int main() {
    const float nan = std::nanf("");
    // ragged rows, one of them empty, one with a missing value
    const vec2 rows = {{1, 2, 3, 4}, {10}, {}, {5, nan, 1}, {-0.0f, 0.0f, -0.0f}};
    expect(eq(calc_statistic(rows, Mean), vec{2.5f, 10, nan, 3, 0}), "mean");
    expect(eq(calc_statistic(rows, Sum), vec{10, 10, nan, 6, 0}), "sum");
    expect(eq(calc_statistic(rows, Count), vec{4, 1, 0, 2, 3}), "count");
    expect(eq(calc_statistic(rows, Min), vec{1, 10, nan, 1, -0.0f}), "min: the first of equal values");
    expect(eq(calc_statistic(rows, Max), vec{4, 10, nan, 5, -0.0f}), "max: the first of equal values");
    expect(eq(calc_statistic(rows, Median), vec{2.5f, 10, nan, 3, -0.0f}), "median");
    expect(eq(calc_statistic(rows, Variance), vec{1.25f, 0, nan, 4, 0}), "variance");
    expect(eq(calc_quantile(rows, 0.5f), vec{2.5f, 10, nan, 3, -0.0f}), "quantile 0.5");
    expect(eq(calc_quantile(rows, 0.0f), vec{1, 10, nan, 1, -0.0f}), "quantile 0");
    expect(eq(calc_quantile(rows, 1.0f), vec{4, 10, nan, 5, -0.0f}), "quantile 1");
    expect(eq(calc_quantile(rows), vec(5, nan)), "quantile = MV (the default)");
    // every row agrees with the vec forms
    const Statistic stats[] = {Mean, Min, Median, Max, Std, Variance, Sum, Count};
    for(Statistic s : stats) {
        const vec got = calc_statistic(rows, s);
        for(size_t n = 0; n < rows.size(); n++) expect(eq(got[n], calc_statistic(rows[n], s)), "calc_statistic(vec2) row == calc_statistic(vec)");
    }
    for(float q : {0.0f, 0.1f, 0.25f, 0.5f, 0.9f, 1.0f}) {
        const vec got = calc_quantile(rows, q);
        for(size_t n = 0; n < rows.size(); n++) expect(eq(got[n], calc_quantile(rows[n], q)), "calc_quantile(vec2) row == calc_quantile(vec)");
    }
    // long rows (beyond the LDS tile) of different lengths
    vec2 longrows(3);
    for(int n = 0; n < 3; n++)
        for(int i = 0; i < 200 + 150 * n; i++) longrows[n].push_back((float)((i * 7919 + n * 31) % 1013) * 0.25f - 100.0f);
    for(float q : {0.3f, 0.5f, 0.99f}) {
        const vec got = calc_quantile(longrows, q);
        for(size_t n = 0; n < 3; n++) expect(eq(got[n], calc_quantile(longrows[n], q)), "long ragged rows");
    }
    expect(calc_statistic(vec2(), Mean).empty() && calc_quantile(vec2(), 0.5f).empty(), "no rows");
    expect(eq(calc_statistic(vec2(3), Mean), vec(3, nan)) && eq(calc_quantile(vec2(3), 0.5f), vec(3, nan)), "only empty rows");
    // a cube with one level per cell
    const vec3 cube = {{{1, 2, 3}, {4, nan, 6}}, {{9, 8, 7}, {nan, nan, nan}}};
    const vec2 levels = {{0.5f, 0.25f}, {1.0f, 0.5f}};
    const vec2 got = calc_quantile(cube, levels);
    expect(eq(got, vec2{{2, 4.5f}, {9, nan}}), "cube: known answers");
    for(size_t y = 0; y < 2; y++)
        for(size_t x = 0; x < 2; x++) expect(eq(got[y][x], calc_quantile(cube[y][x], levels[y][x])), "cube cell == calc_quantile(vec)");
    expect(eq(calc_quantile(cube, vec2{{nan, 0.5f}, {0.0f, 1.0f}}), vec2{{nan, 5}, {7, nan}}), "cube: a NaN level passes");
    // empty shapes (util.cpp:190-200)
    expect(calc_quantile(vec3(), vec2()).empty(), "cube: no y");
    expect(calc_quantile(vec3(2), vec2(2)).empty(), "cube: no x");
    expect(eq(calc_quantile(vec3(2, vec2(2)), vec2(2, vec(2, 0.5f))), vec2(2, vec(2, nan))), "cube: no members");
    // exceptions
    expect(throws<std::invalid_argument>([&] { calc_quantile(cube, vec2{{0.5f, 0.5f}}); }), "mismatch in y");
    expect(throws<std::invalid_argument>([&] { calc_quantile(cube, vec2{{0.5f}, {0.5f}}); }), "mismatch in x");
    expect(throws<std::invalid_argument>([&] { calc_quantile(cube, vec2{{0.5f, 1.5f}, {0.5f, 0.5f}}); }), "a level above 1");
    expect(throws<std::invalid_argument>([&] { calc_quantile(rows, 1.5f); }), "quantile above 1");
    expect(throws<std::invalid_argument>([&] { calc_quantile(rows, -0.1f); }), "quantile below 0");
    expect(throws<std::runtime_error>([&] { calc_statistic(rows, Quantile); }), "Quantile");
    expect(throws<std::runtime_error>([&] { calc_statistic(rows, RandomChoice); }), "RandomChoice");
    if(failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
