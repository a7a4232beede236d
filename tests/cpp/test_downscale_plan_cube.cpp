// The cube-layout gradients and the planned ensemble downscalers of gridpp::DownscalingPlan (gridpp_amd/host/gridpp_downscale_plan.hpp)
// for a Grid and a Points output: every plane of simple_gradient_cube / full_gradient_cube equals the direct simple_gradient /
// full_gradient of gridpp.hpp on that member bit for bit (NaN matches NaN), with shared (vec2), per-member (vec3), mixed and absent
// gradients; downscale_probability and mask_threshold_downscale_* equal the direct functions.  The case comes from a fixed recurrence.
#include "gridpp_downscale_plan.hpp"
#include <cstdio>
#include <cstring>

using namespace gridpp;

static int failures = 0;
static void expect(bool ok, const char* what) {
    if(!ok) { std::printf("FAIL: %s\n", what); failures++; }
}
template <class E, class F>
static bool throws(F f) {
    try { f(); } catch(const E&) { return true; } catch(...) { return false; }
    return false;
}
static unsigned state = 4711u;
static float uniform() {   // [0, 1)
    state = state * 1664525u + 1013904223u;
    return (float)(state >> 8) / 16777216.0f;
}
static bool same(float a, float b) {
    if(std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    return std::memcmp(&a, &b, 4) == 0;
}
static bool same(const vec& a, const vec& b) {
    if(a.size() != b.size()) return false;
    for(size_t i = 0; i < a.size(); i++) if(!same(a[i], b[i])) return false;
    return true;
}
static bool same(const vec2& a, const vec2& b) {
    if(a.size() != b.size()) return false;
    for(size_t i = 0; i < a.size(); i++) if(!same(a[i], b[i])) return false;
    return true;
}
static vec2 field(int Y, int X, float lo, float hi, float missing) {
    vec2 f(Y, vec(X));
    for(auto& r : f) for(auto& v : r) { v = lo + (hi - lo) * uniform(); if(uniform() < missing) v = NAN; }
    return f;
}
static vec3 cube_of(int Y, int X, int E, float lo, float hi, float missing) {
    vec3 c(Y, vec2(X, vec(E)));
    for(auto& r : c) for(auto& m : r) for(auto& v : m) { v = lo + (hi - lo) * uniform(); if(uniform() < missing) v = NAN; }
    return c;
}
static vec2 member(const vec3& cube, int e) {   // plane e of (Y, X, E)
    vec2 f(cube.size(), vec(cube[0].size()));
    for(size_t y = 0; y < cube.size(); y++) for(size_t x = 0; x < cube[0].size(); x++) f[y][x] = cube[y][x][e];
    return f;
}
static vec column(const vec2& a, int e) {   // plane e of (N, E)
    vec m(a.size());
    for(size_t i = 0; i < a.size(); i++) m[i] = a[i][e];
    return m;
}

int main() {
    const int Y = 23, X = 29, OY = 31, OX = 37, N = 500, E = 6;
    vec2 lats(Y, vec(X)), lons(Y, vec(X)), olats(OY, vec(OX)), olons(OY, vec(OX));
    for(int y = 0; y < Y; y++) for(int x = 0; x < X; x++) { lats[y][x] = 60.0f + 0.05f * y + 0.002f * x; lons[y][x] = 10.0f + 0.08f * x - 0.003f * y; }
    const float lat0 = 59.95f, lat1 = 61.2f, lon0 = 9.85f, lon1 = 12.35f;   // a little beyond the input grid on every side
    for(int y = 0; y < OY; y++) for(int x = 0; x < OX; x++) { olats[y][x] = lat0 + (lat1 - lat0) * y / (OY - 1); olons[y][x] = lon0 + (lon1 - lon0) * x / (OX - 1); }
    vec plats(N), plons(N), pelevs(N), plafs(N);
    for(int i = 0; i < N; i++) { plats[i] = lat0 + (lat1 - lat0) * uniform(); plons[i] = lon0 + (lon1 - lon0) * uniform(); pelevs[i] = 1500 * uniform(); plafs[i] = uniform(); }
    const Grid igrid(lats, lons, field(Y, X, 0, 1500, 0.02f), field(Y, X, 0, 1, 0.02f));
    const Grid ogrid(olats, olons, field(OY, OX, 0, 1500, 0.02f), field(OY, OX, 0, 1, 0.02f));
    const Points opoints(plats, plons, pelevs, plafs);
    const vec3 cube = cube_of(Y, X, E, -5, 15, 0.05f), ecube = cube_of(Y, X, E, -0.01f, 0, 0.04f), lcube = cube_of(Y, X, E, 0, 3, 0.04f);
    const vec2 egrad = field(Y, X, -0.01f, 0, 0.04f), lgrad = field(Y, X, 0, 3, 0.04f);
    const vec2 threshold = field(OY, OX, 0, 10, 0.0f);

    for(Downscaler ds : {Nearest, Bilinear}) {
        const DownscalingPlan gplan(igrid, ogrid, ds), pplan(igrid, opoints, ds);
        // Grid -> Grid
        const vec3 gs = gplan.simple_gradient_cube(cube, -0.0065f);
        const vec3 gshared = gplan.full_gradient_cube(cube, egrad, lgrad), gmember = gplan.full_gradient_cube(cube, ecube, lcube);
        const vec3 gmixed = gplan.full_gradient_cube(cube, egrad, lcube), gelev = gplan.full_gradient_cube(cube, ecube, vec2());
        const vec3 gnone = gplan.full_gradient_cube(cube, vec2(), vec3());
        expect((int)gs.size() == OY && (int)gs[0].size() == OX && (int)gs[0][0].size() == E, "grid: the shape of simple_gradient_cube");
        for(int e = 0; e < E; e++) {
            const vec2 v = member(cube, e);
            expect(same(member(gs, e), simple_gradient(igrid, ogrid, v, -0.0065f, ds)), "grid: a member of simple_gradient_cube");
            expect(same(member(gshared, e), full_gradient(igrid, ogrid, v, egrad, lgrad, ds)), "grid: shared gradients");
            expect(same(member(gmember, e), full_gradient(igrid, ogrid, v, member(ecube, e), member(lcube, e), ds)), "grid: per-member gradients");
            expect(same(member(gmixed, e), full_gradient(igrid, ogrid, v, egrad, member(lcube, e), ds)), "grid: a shared and a per-member gradient");
            expect(same(member(gelev, e), full_gradient(igrid, ogrid, v, member(ecube, e), vec2(), ds)), "grid: the elevation gradient only");
            expect(same(member(gnone, e), full_gradient(igrid, ogrid, v, vec2(), vec2(), ds)), "grid: no gradient");
        }
        // Grid -> Points
        const vec2 ps = pplan.simple_gradient_cube_points(cube, 0.01f);
        const vec2 pshared = pplan.full_gradient_cube_points(cube, egrad, lgrad), pmember = pplan.full_gradient_cube_points(cube, ecube, lcube);
        expect((int)ps.size() == N && (int)ps[0].size() == E, "points: the shape of simple_gradient_cube_points");
        for(int e = 0; e < E; e++) {
            const vec2 v = member(cube, e);
            expect(same(column(ps, e), simple_gradient(igrid, opoints, v, 0.01f, ds)), "points: a member of simple_gradient_cube_points");
            expect(same(column(pshared, e), full_gradient(igrid, opoints, v, egrad, lgrad, ds)), "points: shared gradients");
            expect(same(column(pmember, e), full_gradient(igrid, opoints, v, member(ecube, e), member(lcube, e), ds)), "points: per-member gradients");
        }
        // the ensemble downscalers
        expect(same(gplan.downscale_probability(cube, threshold, Gt), downscale_probability(igrid, ogrid, cube, threshold, Gt)), "downscale_probability");
        expect(same(gplan.mask_threshold_downscale_consensus(cube, ecube, lcube, threshold, Leq, Mean),
                    mask_threshold_downscale_consensus(igrid, ogrid, cube, ecube, lcube, threshold, Leq, Mean)), "mask_threshold_downscale_consensus");
        expect(same(gplan.mask_threshold_downscale_quantile(cube, ecube, lcube, threshold, Lt, 0.3f),
                    mask_threshold_downscale_quantile(igrid, ogrid, cube, ecube, lcube, threshold, Lt, 0.3f)), "mask_threshold_downscale_quantile");
        // refusals
        expect(throws<std::invalid_argument>([&] { pplan.simple_gradient_cube(cube, 0); }), "a points plan refuses simple_gradient_cube");
        expect(throws<std::invalid_argument>([&] { gplan.full_gradient_cube_points(cube, egrad, lgrad); }), "a grid plan refuses full_gradient_cube_points");
        expect(throws<std::invalid_argument>([&] { pplan.downscale_probability(cube, threshold, Gt); }), "a points plan refuses downscale_probability");
        expect(throws<std::invalid_argument>([&] { gplan.simple_gradient_cube(cube_of(Y, X + 1, E, 0, 1, 0), 0); }), "a cube of another size is refused");
        expect(throws<std::invalid_argument>([&] { gplan.full_gradient_cube(cube, field(Y, X + 1, 0, 1, 0), lgrad); }), "an elevation gradient of another size is refused");
        expect(throws<std::invalid_argument>([&] { gplan.full_gradient_cube(cube, egrad, cube_of(Y, X, E + 1, 0, 1, 0)); }), "a laf gradient of another member count is refused");
        expect(throws<std::invalid_argument>([&] { gplan.downscale_probability(cube, field(OY, OX + 1, 0, 1, 0), Gt); }), "a threshold of another size is refused");
        expect(throws<std::invalid_argument>([&] { gplan.downscale_probability(cube, threshold, (ComparisonOperator)7); }), "an unknown operator is refused");
        expect(gplan.simple_gradient_cube(vec3(Y, vec2(X, vec())), 0).size() == (size_t)OY, "no members give an empty result");
    }
    // a Bilinear plan may span two coordinate types; the ensemble downscalers may not
    const DownscalingPlan across(igrid, Grid(olats, olons, vec2(), vec2(), Cartesian), Bilinear);
    expect(throws<std::invalid_argument>([&] { across.downscale_probability(cube, threshold, Gt); }), "coordinate types must be the same");
    if(failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
