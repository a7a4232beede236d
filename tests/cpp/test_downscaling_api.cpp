// Known answers of downscaling / simple_gradient / full_gradient through the C++ host mirror (gridpp_amd/host/gridpp.hpp),
// written as code for gridpp.h would call them (defaults included).  The numbers are cases of
// tests/golden/downscaling_known_answers.json (named in the comments).  Built and run by tests/test_gpu_downscaling_cpp.py.
#include "gridpp.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace gridpp;

static int failures = 0;
static void expect(bool ok, const char* what) {
    if(!ok) { std::printf("FAIL: %s\n", what); failures++; }
}
static bool eq(float a, float b) { return (std::isnan(a) && std::isnan(b)) || std::fabs(a - b) <= 1.5e-6f; }
static bool eq(const vec& a, const vec& b) { if(a.size() != b.size()) return false; for(size_t i = 0; i < a.size(); i++) if(!eq(a[i], b[i])) return false; return true; }
static bool eq(const vec2& a, const vec2& b) { if(a.size() != b.size()) return false; for(size_t i = 0; i < a.size(); i++) if(!eq(a[i], b[i])) return false; return true; }
static bool eq(const vec3& a, const vec3& b) { if(a.size() != b.size()) return false; for(size_t i = 0; i < a.size(); i++) if(!eq(a[i], b[i])) return false; return true; }
template <class F>
static bool throws_invalid(F f) {
    try { f(); } catch(const std::invalid_argument&) { return true; } catch(...) { return false; }
    return false;
}

int main() {
    // ---- full_gradient: the 2 x 2 grid of the full_* cases onto the 3 x 3 grid / its 9 points ----
    vec2 ilats = {{40, 40}, {50, 50}}, ilons = {{10, 20}, {10, 20}};
    vec2 olats = {{40, 40, 40}, {45, 45, 45}, {50, 50, 50}}, olons = {{10, 15, 20}, {10, 15, 20}, {10, 15, 20}};
    vec2 ielevs(2, vec(2, 0)), ilafs(2, vec(2, 0.5f));
    vec2 oelevs = {{0, 100, 0}, {0, 200, 0}, {0, 100, 0}}, olafs = {{0, 1, 0}, {0, 1, 0}, {0, 1, 0}};
    Grid igrid(ilats, ilons, ielevs, ilafs), ogrid(olats, olons, oelevs, olafs);
    Points opoints({10, 10, 10, 15, 15, 15, 20, 20, 20}, {40, 45, 50, 40, 45, 50, 40, 45, 50}, {0, 100, 0, 0, 200, 0, 0, 100, 0}, {0, 1, 0, 0, 1, 0, 0, 1, 0});
    vec2 iv(2, vec(2, 15)), eg(2, vec(2, -1.0f / 100)), lg(2, vec(2, 10)), zero(2, vec(2, 0));
    // full_grid_to_grid_all_2d, full_grid_to_point_all_1d
    expect(eq(full_gradient(igrid, ogrid, iv, eg, lg), vec2{{10, 19, 10}, {10, 18, 10}, {10, 19, 10}}), "full_grid_to_grid_all_2d");
    expect(eq(full_gradient(igrid, opoints, iv, eg, lg), vec{10, 19, 10, 10, 18, 10, 10, 19, 10}), "full_grid_to_point_all_1d");
    // full_grid_to_grid_elev_2d with the default laf_gradient (absent) and with a zero one
    expect(eq(full_gradient(igrid, ogrid, iv, eg), vec2{{15, 14, 15}, {15, 13, 15}, {15, 14, 15}}), "full gradient, default laf_gradient");
    expect(eq(full_gradient(igrid, ogrid, iv, eg, zero, Nearest), vec2{{15, 14, 15}, {15, 13, 15}, {15, 14, 15}}), "full_grid_to_grid_elev_2d");
    expect(eq(full_gradient(igrid, opoints, iv, zero, lg), vec{10, 20, 10, 10, 20, 10, 10, 20, 10}), "full_grid_to_point_laf_1d");
    // full_grid_to_grid_all_3d_varying and the same levels through the Points overload
    vec3 iv3(5, iv), eg3(5), lg3(5);
    vec3 want3(5);
    vec2 want2p(5);
    for(int i = 0; i < 5; i++) {
        eg3[i] = vec2(2, vec(2, -0.01f * (i + 1)));
        lg3[i] = vec2(2, vec(2, 10 * (1 - i / 5.0f)));
    }
    want3[0] = {{10, 19, 10}, {10, 18, 10}, {10, 19, 10}};
    want3[1] = {{11, 17, 11}, {11, 15, 11}, {11, 17, 11}};
    want3[2] = {{12, 15, 12}, {12, 12, 12}, {12, 15, 12}};
    want3[3] = {{13, 13, 13}, {13, 9, 13}, {13, 13, 13}};
    want3[4] = {{14, 11, 14}, {14, 6, 14}, {14, 11, 14}};
    expect(eq(full_gradient(igrid, ogrid, iv3, eg3, lg3), want3), "full_grid_to_grid_all_3d_varying");
    for(int i = 0; i < 5; i++) for(int y = 0; y < 3; y++) for(int x = 0; x < 3; x++) want2p[i].push_back(want3[i][y][x]);
    expect(eq(full_gradient(igrid, opoints, iv3, eg3, lg3, Nearest), want2p), "full gradient, Points, 3-D");
    // errors (gradient.cpp:10-20; the asserted overloads raise the same)
    expect(throws_invalid([&] { full_gradient(igrid, ogrid, vec2(2, vec(3, 15)), eg, lg); }), "Values is the wrong size");
    expect(throws_invalid([&] { full_gradient(igrid, ogrid, iv, vec2(1, vec(2, 0)), lg); }), "Elevation gradient is the wrong size");
    expect(throws_invalid([&] { full_gradient(igrid, opoints, iv3, eg3, vec3(2, lg)); }), "Laf gradient is the wrong size");
    expect(throws_invalid([&] { full_gradient(igrid, ogrid, iv, eg, lg, (Downscaler)5); }), "Invalid downscaler");

    // ---- simple_gradient: the 3 x 3 grid of the simple_* cases ----
    vec2 slats = {{0, 1, 2}, {0, 1, 2}, {0, 1, 2}}, slons = {{0, 0, 0}, {1, 1, 1}, {2, 2, 2}};
    vec2 selevs(3, vec(3, 0));
    selevs[0][0] = -10; selevs[1][1] = 10;
    Grid sgrid(slats, slons, selevs);
    Points spoints({-1, 0.9f}, {-1, 0.9f}, {-5, 5});
    vec2 sv(3, vec(3, 0));
    sv[0][0] = 4; sv[1][1] = 3;
    expect(eq(simple_gradient(sgrid, spoints, sv, 0), vec{4, 3}), "simple_point_to_point_0");
    expect(eq(simple_gradient(sgrid, spoints, sv, 1, Nearest), vec{9, -2}), "simple_point_to_point_1");
    expect(eq(simple_gradient(sgrid, spoints, vec3(2, sv), 1), vec2{{9, -2}, {9, -2}}), "simple_point_to_point_3d_1");
    vec2 g0lats = {{-0.1f, 0.1f, 1.1f}, {-0.1f, 0.1f, 1.1f}, {-0.1f, 0.1f, 1.1f}}, g0lons = {{-0.1f, -0.1f, -0.1f}, {0.1f, 0.1f, 0.1f}, {1.1f, 1.1f, 1.1f}};
    Grid g0(g0lats, g0lons, vec2{{0, 1, 2}, {3, 4, 5}, {6, 7, 8}});
    vec2 e1 = {{14, 15, 2}, {17, 18, 5}, {6, 7, 1}};
    expect(eq(simple_gradient(sgrid, g0, sv, 1), e1), "simple_grid_to_grid_1");
    expect(eq(simple_gradient(sgrid, g0, vec3(2, sv), 1), vec3{e1, e1}), "simple_3d");
    Points bare({-1, 0.9f}, {-1, 0.9f});
    vec2 s9 = {{0, 1, 2}, {3, 4, 5}, {6, 7, 8}};
    vec r = simple_gradient(sgrid, bare, s9, 0);
    expect(r.size() == 2 && std::isnan(r[0]) && std::isnan(r[1]), "simple_no_point_elev_0");
    expect(throws_invalid([&] { simple_gradient(sgrid, spoints, vec2(3, vec(2, 0)), 0); }), "simple_mismatch_points");

    // ---- downscaling ----
    vec2 dlats = {{30, 30, 30}, {40, 40, 40}, {50, 50, 50}}, dlons = {{0, 10, 20}, {0, 10, 20}, {0, 10, 20}};
    Grid dgrid(dlats, dlons), dgrid2(vec2{{30, 30}, {50, 50}}, vec2{{0, 20}, {0, 20}});
    vec3 d18(2, vec2(3, vec(3)));
    for(int k = 0; k < 18; k++) d18[k / 9][(k % 9) / 3][k % 3] = (float)k;
    expect(eq(downscaling(dgrid, dgrid2, d18, Nearest), vec3{{{0, 2}, {6, 8}}, {{9, 11}, {15, 17}}}), "downscaling_grid_to_grid_3d");
    expect(eq(downscaling(dgrid, dgrid2, d18[0], Bilinear), vec2{{0, 2}, {6, 8}}), "downscaling, Bilinear on the nodes");
    expect(throws_invalid([&] { downscaling(dgrid, dgrid2, vec2(3, vec(2, 0)), Nearest); }), "downscaling_mismatch_2d_grid");
    expect(throws_invalid([&] { downscaling(dgrid, dgrid2, d18[0], (Downscaler)2); }), "Invalid downscaler");

    if(failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
