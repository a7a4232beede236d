// calc_score and neighbourhood_score through the C++ host mirror (gridpp_amd/host/gridpp.hpp), written as code for gridpp.h would call
// them.  The numbers are the known answers of tests/golden/score_known_answers.json (the reference's tests/test_metric_optimizer.py:29-46),
// the hand-worked guard rows of tests/score_ref.py and the 3 x 3 case of tests/test_score_restatement.py.  Built and run by
// tests/test_gpu_score_cpp.py.
#include "gridpp.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace gridpp;

static int failures = 0;
static void expect(bool ok, const char* what) {
    if(!ok) { std::printf("FAIL: %s\n", what); failures++; }
}
static bool eq(float a, float b) { return (std::isnan(a) && std::isnan(b)) || a == b; }
static bool near3(float a, float b) { return (std::isnan(a) && std::isnan(b)) || std::fabs(a - b) < 1.5e-3f; }   // assert_almost_equal(..., 3)
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
    static_assert(Ets == 0 && Ts == 1 && Kss == 20 && Pc == 30 && Bias == 40 && Hss == 50, "include/gridpp.h:103-110");
    // the 24 known answers, both vector overloads
    const vec obs = {1, 2, 3}, fcst = {2, 1, 3};
    const float thresholds[4] = {-1, 1.5f, 2.5f, 3};
    const Metric metrics[6] = {Bias, Pc, Ets, Kss, Hss, Ts};
    const float expected[6][4] = {{1, 1, 1, 1}, {1, 0.333f, 1, 1}, {nan, -0.2f, 1, nan}, {nan, -0.5f, 1, nan}, {nan, -0.5f, 1, nan}, {1, 0.333f, 1, nan}};
    for(int m = 0; m < 6; m++)
        for(int t = 0; t < 4; t++) {
            expect(near3(calc_score(obs, fcst, thresholds[t], metrics[m]), expected[m][t]), "known answer");
            expect(near3(calc_score(obs, fcst, thresholds[t], thresholds[t], metrics[m]), expected[m][t]), "known answer, both thresholds");
        }
    // fthreshold moves only the forecast's side: with fthreshold 5 nothing is forecast, a = b = 0
    expect(eq(calc_score(obs, fcst, 1.5f, 5.0f, Ts), 0.0f), "fthreshold");
    // tables: 3 1 2 4 by hand, and the guards
    expect(eq(calc_score(3, 1, 2, 4, Ets), 0.25f), "Ets");
    expect(eq(calc_score(3, 1, 2, 4, Ts), 0.5f), "Ts");
    expect(eq(calc_score(3, 1, 2, 4, Pc), 7.0f / 10.0f), "Pc");
    expect(eq(calc_score(3, 1, 2, 4, Kss), (float)(10.0 / 25.0)), "Kss");
    expect(eq(calc_score(3, 1, 2, 4, Bias), 1.0f - 1.0f / 3.0f), "Bias");
    expect(eq(calc_score(3, 1, 2, 4, Hss), (float)(20.0 / 50.0)), "Hss");
    expect(eq(calc_score(5, 0, 0, 7, Ets), 1.0f) && eq(calc_score(5, 0, 0, 0, Ets), nan) && eq(calc_score(0, 0, 0, 7, Ets), nan), "Ets guard");
    expect(eq(calc_score(0, 3, 0, 4, Kss), nan) && eq(calc_score(3, 0, 4, 0, Kss), nan) && eq(calc_score(0, 0, 0, 0, Hss), nan), "Kss / Hss guards");
    expect(eq(calc_score(0, 0, 0, 0, Bias), 1.0f) && eq(calc_score(4, 2, 2, 9, Bias), 1.0f), "Bias guard");
    expect(eq(calc_score(0, 0, 0, 0, Ts), nan) && eq(calc_score(0, 0, 0, 0, Pc), nan), "0 / 0");
    expect(throws<std::invalid_argument>([&] { calc_score(1, 1, 1, 1, (Metric)7); }), "unknown metric, table");
    expect(throws<std::invalid_argument>([&] { calc_score(obs, fcst, 1.5f, (Metric)7); }), "unknown metric, vectors");
    expect(throws<std::invalid_argument>([&] { calc_score(vec{1}, fcst, 1.5f, Pc); }), "ref shorter than fcst");
    expect(eq(calc_score(vec(), vec(), 0.5f, Bias), 1.0f) && eq(calc_score(vec(), vec(), 0.5f, Pc), nan), "empty vectors");
    // neighbourhood_score: 3 x 3 Cartesian grid, two observations, half width 1 (tests/test_score_restatement.py)
    vec2 lats(3, vec(3)), lons(3, vec(3));
    for(int y = 0; y < 3; y++) for(int x = 0; x < 3; x++) { lats[y][x] = 1000.0f * y; lons[y][x] = 1000.0f * x; }
    const vec2 zeros(3, vec(3, 0.0f));
    Grid grid(lats, lons, zeros, zeros, Cartesian);
    Points points(vec{100, 1900}, vec{-200, 2100}, vec{0, 0}, vec{0, 0}, Cartesian);
    const vec2 ones(3, vec(3, 1.0f));
    const vec ref = {1, 0};
    expect(eq(neighbourhood_score(grid, points, ones, ref, 1, Ts, 0.5f), vec2{{1, 1, nan}, {1, 0.5f, 0}, {nan, 0, 0}}), "neighbourhood_score Ts");
    expect(eq(neighbourhood_score(grid, points, ones, ref, 1, Pc, 0.5f), vec2{{1, 1, nan}, {1, 0.5f, 0}, {nan, 0, 0}}), "neighbourhood_score Pc");
    expect(eq(neighbourhood_score(grid, points, ones, ref, 1, Bias, 0.5f), vec2{{1, 1, 1}, {1, 0, 0}, {1, 0, 0}}), "neighbourhood_score Bias");
    expect(eq(neighbourhood_score(grid, points, ones, ref, 50, Bias, 0.5f), vec2(3, vec(3, 0.0f))), "a half width beyond the grid");
    // the checks in the reference's order
    const vec2 wrong(3, vec(4, 1.0f));
    auto message = [&](const vec2& f, const vec& r, int hw, Metric m) -> std::string {
        try { neighbourhood_score(grid, points, f, r, hw, m, 0.5f); } catch(const std::invalid_argument& e) { return e.what(); }
        return "";
    };
    expect(message(wrong, vec{1}, 0, (Metric)7) == "Grid size is not the same as forecast values", "check 1");
    expect(message(ones, vec{1}, 0, (Metric)7) == "half_width must be greater than 0", "check 2");
    expect(message(ones, vec{1}, 1, (Metric)7) == "Unknown metric", "check 3");
    expect(message(ones, vec{1}, 1, Ets) == "Points size is not the same as values", "check 4");
    expect(neighbourhood_score(Grid(), Points(), vec2(), vec(), 1, Ets, 0.5f).empty(), "empty grid");
    if(failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
