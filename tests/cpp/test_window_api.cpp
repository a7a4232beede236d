// Known answers of window through the C++ host mirror (gridpp_amd/host/gridpp.hpp), written as code for gridpp.h would call it.  The
// numbers are cases of tests/golden/window_known_answers.json (named in the comments).  Built and run by tests/test_gpu_window_cpp.py.
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

int main() {
    const float nan = std::nanf("");
    vec2 inputs(5, vec(5));
    for(int i = 0; i < 5; i++) for(int j = 0; j < 5; j++) inputs[i][j] = (float)(i + j);
    vec2 inputs_nan = inputs;
    inputs_nan[3][3] = nan;
    const vec2 small(2, vec(2, 1.0f));
    // sum, count, mean, min, max (tests/test_window.py:18-36)
    expect(eq(window(inputs, 3, Sum, false, false, false), vec2{{1, 3, 6, 9, 7}, {3, 6, 9, 12, 9}, {5, 9, 12, 15, 11}, {7, 12, 15, 18, 13}, {9, 15, 18, 21, 15}}), "sum");
    expect(eq(window(inputs, 3, Count, false, false, false), vec2(5, vec{2, 3, 3, 3, 2})), "count");
    expect(eq(window(inputs, 3, Mean, false, false, false),
              vec2{{0.5f, 1, 2, 3, 3.5f}, {1.5f, 2, 3, 4, 4.5f}, {2.5f, 3, 4, 5, 5.5f}, {3.5f, 4, 5, 6, 6.5f}, {4.5f, 5, 6, 7, 7.5f}}), "mean");
    expect(eq(window(inputs, 3, Min, false, false, false), vec2{{0, 0, 1, 2, 3}, {1, 1, 2, 3, 4}, {2, 2, 3, 4, 5}, {3, 3, 4, 5, 6}, {4, 4, 5, 6, 7}}), "min");
    expect(eq(window(inputs, 3, Max, false, false, false), vec2{{1, 2, 3, 4, 4}, {2, 3, 4, 5, 5}, {3, 4, 5, 6, 6}, {4, 5, 6, 7, 7}, {5, 6, 7, 8, 8}}), "max");
    // sum_before, count_before, sum_missing_edge, count_missing (:38-52)
    expect(eq(window(inputs, 3, Sum, true, false, false), vec2{{0, 1, 3, 6, 9}, {1, 3, 6, 9, 12}, {2, 5, 9, 12, 15}, {3, 7, 12, 15, 18}, {4, 9, 15, 18, 21}}), "sum_before");
    expect(eq(window(inputs, 3, Count, true, false, false), vec2(5, vec{1, 2, 3, 3, 3})), "count_before");
    expect(eq(window(inputs, 3, Sum, true, false, true),
              vec2{{nan, nan, 3, 6, 9}, {nan, nan, 6, 9, 12}, {nan, nan, 9, 12, 15}, {nan, nan, 12, 15, 18}, {nan, nan, 15, 18, 21}}), "sum_missing_edge");
    expect(eq(window(inputs, 3, Count, true, false, true), vec2(5, vec{1, 2, 3, 3, 3})), "count_missing");
    // count_nan (:54-64): Count ignores both flags
    vec2 all_nan(5, vec(5, nan));
    for(int keep = 0; keep < 2; keep++)
        for(int edges = 0; edges < 2; edges++) {
            expect(eq(window(inputs_nan, 3, Count, true, keep, edges), vec2{{1, 2, 3, 3, 3}, {1, 2, 3, 3, 3}, {1, 2, 3, 3, 3}, {1, 2, 3, 2, 2}, {1, 2, 3, 3, 3}}),
                   "count_nan_before");
            expect(eq(window(inputs_nan, 3, Count, false, keep, edges), vec2{{2, 3, 3, 3, 2}, {2, 3, 3, 3, 2}, {2, 3, 3, 3, 2}, {2, 3, 2, 2, 1}, {2, 3, 3, 3, 2}}),
                   "count_nan_centred");
            expect(eq(window(all_nan, 3, Count, false, keep, edges), vec2(5, vec(5, 0.0f))), "count_nan_all_missing");
        }
    // sum_keep_missing, edge_case, edge_case2 (:66-77)
    expect(eq(window(inputs_nan, 3, Sum, true, true, false), vec2{{0, 1, 3, 6, 9}, {1, 3, 6, 9, 12}, {2, 5, 9, 12, 15}, {3, 7, 12, nan, nan}, {4, 9, 15, 18, 21}}),
           "sum_keep_missing");
    expect(eq(window(small, 5, Sum, false, false, false), vec2{{2, 2}, {2, 2}}), "edge_case");
    expect(eq(window(small, 5, Sum, false, false, true), vec2{{nan, nan}, {nan, nan}}), "edge_case2");
    // before_*, centered_* (:79-105)
    const vec2 row = {{0, 1, 2, nan, 3, 4, 5}};
    expect(eq(window(row, 2, Sum, true, false, false), vec2{{0, 1, 3, 2, 3, 7, 9}}), "before_0");
    expect(eq(window(row, 2, Sum, true, true, false), vec2{{0, 1, 3, nan, nan, 7, 9}}), "before_keep");
    expect(eq(window(row, 2, Sum, true, false, true), vec2{{nan, 1, 3, 2, 3, 7, 9}}), "before_edges");
    expect(eq(window(row, 2, Sum, true, true, true), vec2{{nan, 1, 3, nan, nan, 7, 9}}), "before_keep_edges");
    expect(eq(window(row, 3, Sum, false, false, false), vec2{{1, 3, 3, 5, 7, 12, 9}}), "centered_0");
    expect(eq(window(row, 3, Sum, false, true, false), vec2{{1, 3, nan, nan, nan, 12, 9}}), "centered_keep");
    expect(eq(window(row, 3, Sum, false, false, true), vec2{{nan, 3, 3, 5, 7, 12, nan}}), "centered_edges");
    expect(eq(window(row, 3, Sum, false, true, true), vec2{{nan, 3, nan, nan, nan, 12, nan}}), "centered_keep_edges");
    // no_times, no_cases, no_anything (:107-120), with the defaults of include/gridpp.h:1611
    expect(eq(window(vec2(10), 3, Sum), vec2(10)), "no_times");
    expect(window(vec2(), 3, Sum).empty(), "no_cases / no_anything");
    // invalid_length (:122-126) and the odd-length rule (src/api/window.cpp:26-28), which comes after the empty shapes
    for(int length : {0, -1}) {
        expect(throws<std::invalid_argument>([&] { window(vec2(10, vec(3, 0.0f)), length, Sum); }), "invalid_length");
        expect(throws<std::invalid_argument>([&] { window(vec2(), length, Sum); }), "invalid_length, empty array");
    }
    expect(throws<std::invalid_argument>([&] { window(inputs, 4, Sum); }), "even length, centred");
    expect(eq(window(vec2(10), 4, Sum), vec2(10)), "even length, no times: the empty result comes first");
    expect(throws<std::runtime_error>([&] { window(inputs, 3, Quantile); }), "Quantile");
    expect(throws<std::runtime_error>([&] { window(inputs, 3, Unknown); }), "Unknown");
    // long_length, time_length_1 (:128-135)
    expect(eq(window(vec2{{0, 1, 2, 3}}, 1001, Sum, false, false, false), vec2{{6, 6, 6, 6}}), "long_length");
    expect(eq(window(vec2{{1}, {2}}, 1001, Sum, false, false, false), vec2{{1}, {2}}), "time_length_1");
    // the defaults: centred, missing values skipped, NaN at the edges
    expect(eq(window(row, 3, Max), vec2{{nan, 2, 2, 3, 4, 5, nan}}), "defaults");
    if(failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
