// gamma_inv and the Gamma transform through the C++ host mirror (gridpp_amd/host/gridpp_gamma.hpp), written as code for gridpp.h would
// call them: the reference's known answers (tests/test_distribution.py:11-16, tests/test_transform.py:67-93 there), the constructor
// exceptions of transform.cpp:158-163, the messages of distribution.cpp:8-22, a Gamma used through a Transform reference, and the nested
// vector forms.  tests/test_gpu_gamma_cpp.py builds and runs it.
#include "gridpp_gamma.hpp"
#include <cmath>
#include <cstdio>
#include <string>

using namespace gridpp;

static int failures = 0;
static void expect(bool ok, const char* what) {
    if(!ok) { std::printf("FAIL: %s\n", what); failures++; }
}
static bool near(float got, double want, double decimals) { return std::fabs((double)got - want) < 1.5 * std::pow(10.0, -decimals); }
template <class F>
static std::string message_of(F f) {
    try { f(); } catch(const std::invalid_argument& e) { return e.what(); } catch(...) { return "another exception"; }
    return "no exception";
}

int main() {
    // tests/test_distribution.py:11-16
    const vec q = gamma_inv({0.5f, 0.5f, 0.5f}, {1, 2, 7.5f}, {2, 2, 1});
    expect(q.size() == 3 && near(q[0], 1.38629, 5) && near(q[1], 3.35669, 5) && near(q[2], 7.16943, 5), "gamma_inv known answers");
    expect(gamma_inv(vec(), vec(), vec()).empty(), "gamma_inv of nothing");
    const vec edge = gamma_inv({0, 1}, {1, 1}, {1, 1});
    expect(edge[0] == 0 && std::isinf(edge[1]) && edge[1] > 0, "levels 0 and 1");
    expect(message_of([] { gamma_inv({0.5f, -0.1f, 0.5f}, {1, 1, 1}, {1, 1, 1}); }) == "Invalid level '-0.1'. Levels must be on the interval [0, 1].", "level message");
    expect(message_of([] { gamma_inv({0.5f, 0.5f, 1.5f}, {1, 0, 1}, {1, 1, 1}); }) == "Invalid shape '0'. Shapes must be > 0.", "lowest index: the shape");
    expect(message_of([] { gamma_inv({0.5f}, {1}, {NAN}); }) == "Invalid scale 'nan'. Scale must be > 0.", "scale message");
    expect(message_of([] { gamma_inv({0.5f}, {1, 1}, {1, 1}); }) == "gamma_inv: levels, shape and scale must be of the same size", "unequal sizes");

    // tests/test_transform.py:67-93
    const Gamma gamma(1, 2, 0.01f);
    const Transform& t = gamma;
    expect(near(t.forward(0.0f), -2.5766933, 5) && near(t.forward(1.99f), 0.33747494, 5) && near(t.backward(0.3374749f), 1.99, 5), "scalar known answers");
    expect(std::isnan(t.forward(NAN)) && std::isnan(t.backward(NAN)), "NaN in, NaN out");
    const vec f = t.forward(vec{0.0f, 1.99f, NAN});
    expect(f.size() == 3 && near(f[0], -2.5766933, 5) && near(f[1], 0.33747494, 5) && std::isnan(f[2]), "vec forward");
    expect(f[0] == t.forward(0.0f) && f[1] == t.forward(1.99f), "kernel and host form agree on the known answers");
    const vec2 b2 = t.backward(vec2{{0.3374749f, 0.3374749f}, {}, {0.3374749f}});
    expect(b2.size() == 3 && b2[0].size() == 2 && b2[1].empty() && b2[2].size() == 1 && near(b2[0][1], 1.99, 5) && near(b2[2][0], 1.99, 5), "vec2 backward");
    const vec3 f3 = t.forward(vec3{{{1.99f}, {1.99f, 1.99f}}, {{}}});
    expect(f3.size() == 2 && f3[0].size() == 2 && f3[0][1].size() == 2 && f3[1][0].empty() && near(f3[0][1][1], 0.33747494, 5), "vec3 forward");
    Gamma(1, 2, 0);   // tolerance 0 is accepted
    expect(Gamma(1, 2).forward(0.0f) == gamma.forward(0.0f), "the default tolerance is 0.01");
    expect(gamma.forward(-1.0f) != gamma.forward(-1.0f) && gamma.forward(40.0f) == INFINITY && gamma.backward(6.0f) == INFINITY, "IEEE values at the edges");
    for(float bad : {-1.0f, 0.0f, NAN}) {
        expect(message_of([bad] { Gamma(bad, 1); }) == "Shape parameter must be > 0 in the gamma distribution", "shape exception");
        expect(message_of([bad] { Gamma(1, bad); }) == "Scale parameter must be > 0 in the gamma distribution", "scale exception");
    }
    for(float bad : {-1.0f, NAN}) expect(message_of([bad] { Gamma(1, 1, bad); }) == "Tolerance must be >= 0 in the gamma distribution", "tolerance exception");
    expect(Transform().forward(1.0f) == -1 && Transform().forward(vec{1, 2})[1] == -1 && Identity().forward(vec{3})[0] == 3, "the other transforms are unchanged");
    if(failures == 0) std::printf("all checks passed\n");
    return failures ? 1 : 0;
}
