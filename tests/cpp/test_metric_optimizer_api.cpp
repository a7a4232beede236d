// get_optimal_threshold and metric_optimizer_curve through the C++ host mirror (gridpp_amd/host/gridpp_metric_optimizer.hpp), written as
// code for gridpp.h would call them: the reference's two known answers (tests/test_metric_optimizer.py there: a value in (2.4, 2.6), and
// a curve within 1.5 of the squared thresholds), the exact values DESIGN.md 4.13 defines for them, both exceptions, and the cases that
// return without device work.  tests/test_gpu_metric_optimizer_cpp.py builds and runs it.
#include "gridpp_metric_optimizer.hpp"
#include <cmath>
#include <cstdio>
#include <string>

using namespace gridpp;

static int failures = 0;
static void expect(bool ok, const char* what) {
    if(!ok) { std::printf("FAIL: %s\n", what); failures++; }
}
template <class F>
static std::string message_of(F f) {
    try { f(); } catch(const std::invalid_argument& e) { return e.what(); } catch(...) { return "another exception"; }
    return "no exception";
}

int main() {
    const vec obs = {0, 1, 1.4f, 1.6f, 2}, fcst = {1, 2, 2.4f, 2.6f, 3};
    const float x = get_optimal_threshold(obs, fcst, 1.5f, Bias);
    expect(x > 2.4f && x < 2.6f, "the reference's range");
    expect(x == 2.5f, "the midpoint of the plateau [2.4, 2.6)");

    vec ref(101), squares(101);
    for(int i = 0; i < 101; i++) { ref[i] = (float)(0.1 * i); squares[i] = (float)((0.1 * i) * (0.1 * i)); }
    const vec thresholds = {1, 2, 3, 4};
    for(Metric metric : {Pc, Bias}) {
        vec curve_fcst = {7, 7};
        const vec curve_ref = metric_optimizer_curve(ref, squares, thresholds, metric, curve_fcst);
        expect(curve_ref.size() == 4 && curve_fcst == thresholds, "every threshold has a valid optimum");
        for(size_t k = 0; k < curve_ref.size(); k++) {
            expect(std::fabs(curve_ref[k] - curve_fcst[k] * curve_fcst[k]) < 1.5f, "the reference's tolerance");
            expect(curve_ref[k] == get_optimal_threshold(ref, squares, thresholds[k], metric), "the curve holds the single results");
        }
    }
    // thresholds without a valid optimum are dropped, the order is kept
    vec kept;
    const vec some = metric_optimizer_curve(ref, squares, {3, 1000, 1, NAN, 2}, Pc, kept);
    expect(some.size() == 3 && kept == vec({3, 1, 2}) && some[0] > some[2] && some[2] > some[1], "dropped thresholds");

    // no device work
    vec out_fcst = {7};
    expect(metric_optimizer_curve(ref, squares, vec(), Pc, out_fcst).empty() && out_fcst.empty(), "no thresholds");
    expect(metric_optimizer_curve(vec(), vec(), thresholds, Pc, out_fcst).empty() && out_fcst.empty(), "no values");
    expect(std::isnan(get_optimal_threshold(vec(), vec(), 1.5f, Ets)), "empty vectors give MV");
    expect(std::isnan(get_optimal_threshold({2, 2, 2}, {1, 1, 1}, 1.5f, Ets)), "one plateau gives MV");

    expect(message_of([&] { get_optimal_threshold({1}, fcst, 1.5f, Bias); }) == "ref and fcst not the same size", "a short ref");
    expect(message_of([&] { vec o; metric_optimizer_curve({1}, fcst, thresholds, Bias, o); }) == "ref and fcst not the same size", "a short ref, curve");
    expect(message_of([&] { vec o; metric_optimizer_curve(vec(7, 1.0f), fcst, thresholds, Bias, o); }) == "ref and fcst not the same size", "a long ref, curve");
    expect(message_of([&] { get_optimal_threshold(obs, fcst, 1.5f, (Metric)7); }) == "Unknown metric", "an unknown metric");
    expect(message_of([&] { vec o; metric_optimizer_curve(obs, fcst, thresholds, (Metric)7, o); }) == "Unknown metric", "an unknown metric, curve");
    if(failures == 0) std::printf("all checks passed\n");
    return failures ? 1 : 0;
}
