// gridpp::DownscalingPlan through its own header (gridpp_amd/host/gridpp_downscale_plan.hpp): one Grid -> Grid and one Grid -> Points case,
// apply (one field and a stack of levels), apply_cube and the two gradients, each equal to the direct call of gridpp.hpp bit for bit
// (NaN matches NaN), for both downscalers.  The case is generated here from a fixed recurrence; some values are missing so that the
// Bilinear paths mix interpolated and nearest results.  The refusals of the header and its move semantics are checked as well.
#include "gridpp_downscale_plan.hpp"
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <utility>

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
static unsigned state = 12345u;
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
static bool same(const vec3& a, const vec3& b) {
    if(a.size() != b.size()) return false;
    for(size_t i = 0; i < a.size(); i++) if(!same(a[i], b[i])) return false;
    return true;
}
static vec2 field(int Y, int X, float lo, float hi, float missing) {
    vec2 f(Y, vec(X));
    for(auto& r : f) for(auto& v : r) { v = lo + (hi - lo) * uniform(); if(uniform() < missing) v = NAN; }
    return f;
}
static vec2 member(const vec3& cube, int e) {
    vec2 f(cube.size(), vec(cube[0].size()));
    for(size_t y = 0; y < cube.size(); y++) for(size_t x = 0; x < cube[0].size(); x++) f[y][x] = cube[y][x][e];
    return f;
}

int main() {
    const int Y = 23, X = 29, OY = 31, OX = 37, N = 500, T = 3, E = 5;
    vec2 lats(Y, vec(X)), lons(Y, vec(X)), olats(OY, vec(OX)), olons(OY, vec(OX));
    for(int y = 0; y < Y; y++) for(int x = 0; x < X; x++) { lats[y][x] = 60.0f + 0.05f * y + 0.002f * x; lons[y][x] = 10.0f + 0.08f * x - 0.003f * y; }
    const float lat0 = 59.95f, lat1 = 61.2f, lon0 = 9.85f, lon1 = 12.35f;   // a little beyond the input grid on every side
    for(int y = 0; y < OY; y++) for(int x = 0; x < OX; x++) { olats[y][x] = lat0 + (lat1 - lat0) * y / (OY - 1); olons[y][x] = lon0 + (lon1 - lon0) * x / (OX - 1); }
    vec plats(N), plons(N), pelevs(N), plafs(N);
    for(int i = 0; i < N; i++) { plats[i] = lat0 + (lat1 - lat0) * uniform(); plons[i] = lon0 + (lon1 - lon0) * uniform(); pelevs[i] = 1500 * uniform(); plafs[i] = uniform(); }
    const Grid igrid(lats, lons, field(Y, X, 0, 1500, 0.02f), field(Y, X, 0, 1, 0.02f));
    const Grid ogrid(olats, olons, field(OY, OX, 0, 1500, 0.02f), field(OY, OX, 0, 1, 0.02f));
    const Points opoints(plats, plons, pelevs, plafs);
    const vec2 values = field(Y, X, -5, 15, 0.04f), egrad = field(Y, X, -0.01f, 0, 0.04f), lgrad = field(Y, X, 0, 3, 0.04f);
    vec3 levels(T), elevels(T), llevels(T);
    for(int t = 0; t < T; t++) { levels[t] = field(Y, X, -5, 15, 0.04f); elevels[t] = field(Y, X, -0.01f, 0, 0.04f); llevels[t] = field(Y, X, 0, 3, 0.04f); }
    vec3 cube(Y, vec2(X, vec(E)));
    for(auto& r : cube) for(auto& c : r) for(auto& v : c) { v = 20 * uniform() - 5; if(uniform() < 0.05f) v = NAN; }

    for(Downscaler ds : {Nearest, Bilinear}) {
        const DownscalingPlan gplan(igrid, ogrid, ds), pplan(igrid, opoints, ds);
        expect(gplan.downscaler() == ds && gplan.distorted() == 0, "the accessors of a plan");
        expect(gplan.nbytes() >= (long long)OY * OX * (ds == Bilinear ? 16 : 4) && pplan.nbytes() >= (long long)N * (ds == Bilinear ? 16 : 4), "nbytes counts the records");
        // Grid -> Grid
        expect(same(gplan.apply(values), downscaling(igrid, ogrid, values, ds)), "grid: apply of a field");
        expect(same(gplan.apply(levels), downscaling(igrid, ogrid, levels, ds)), "grid: apply of levels");
        expect(same(gplan.simple_gradient(values, -0.0065f), simple_gradient(igrid, ogrid, values, -0.0065f, ds)), "grid: simple_gradient");
        expect(same(gplan.simple_gradient(levels, 0.01f), simple_gradient(igrid, ogrid, levels, 0.01f, ds)), "grid: simple_gradient of levels");
        expect(same(gplan.full_gradient(values, egrad, lgrad), full_gradient(igrid, ogrid, values, egrad, lgrad, ds)), "grid: full_gradient");
        expect(same(gplan.full_gradient(values, egrad), full_gradient(igrid, ogrid, values, egrad, vec2(), ds)), "grid: full_gradient without lafs");
        expect(same(gplan.full_gradient(levels, elevels, llevels), full_gradient(igrid, ogrid, levels, elevels, llevels, ds)), "grid: full_gradient of levels");
        const vec3 gcube = gplan.apply_cube(cube);
        expect((int)gcube.size() == OY && (int)gcube[0].size() == OX && (int)gcube[0][0].size() == E, "grid: the shape of apply_cube");
        for(int e = 0; e < E; e++) expect(same(member(gcube, e), downscaling(igrid, ogrid, member(cube, e), ds)), "grid: a member of apply_cube");
        // Grid -> Points
        expect(same(pplan.apply_points(values), downscaling(igrid, opoints, values, ds)), "points: apply of a field");
        expect(same(pplan.apply_points(levels), downscaling(igrid, opoints, levels, ds)), "points: apply of levels");
        expect(same(pplan.simple_gradient_points(values, -0.0065f), simple_gradient(igrid, opoints, values, -0.0065f, ds)), "points: simple_gradient");
        expect(same(pplan.simple_gradient_points(levels, 0.01f), simple_gradient(igrid, opoints, levels, 0.01f, ds)), "points: simple_gradient of levels");
        expect(same(pplan.full_gradient_points(values, egrad, lgrad), full_gradient(igrid, opoints, values, egrad, lgrad, ds)), "points: full_gradient");
        expect(same(pplan.full_gradient_points(levels, elevels, llevels), full_gradient(igrid, opoints, levels, elevels, llevels, ds)), "points: full_gradient of levels");
        const vec2 pcube = pplan.apply_cube_points(cube);
        expect((int)pcube.size() == N && (int)pcube[0].size() == E, "points: the shape of apply_cube");
        for(int e = 0; e < E; e++) {
            vec m(N);
            for(int i = 0; i < N; i++) m[i] = pcube[i][e];
            expect(same(m, downscaling(igrid, opoints, member(cube, e), ds)), "points: a member of apply_cube");
        }
        // a plan of one output kind refuses the methods of the other
        expect(throws<std::invalid_argument>([&] { gplan.apply_points(values); }), "a grid plan refuses apply_points");
        expect(throws<std::invalid_argument>([&] { pplan.apply(values); }), "a points plan refuses apply");
        expect(throws<std::invalid_argument>([&] { pplan.apply_cube(cube); }), "a points plan refuses apply_cube");
        // sizes
        expect(throws<std::invalid_argument>([&] { gplan.apply(field(Y, X + 1, 0, 1, 0)); }), "a field of another size is refused");
        expect(throws<std::invalid_argument>([&] { gplan.apply_cube(vec3(Y, vec2(X + 1, vec(E)))); }), "a cube of another size is refused");
        expect(throws<std::invalid_argument>([&] { gplan.full_gradient(values, field(Y, X + 1, 0, 1, 0), lgrad); }), "an elevation gradient of another size is refused");
        expect(throws<std::invalid_argument>([&] { gplan.full_gradient(values, egrad, field(Y + 1, X, 0, 1, 0)); }), "a laf gradient of another size is refused");
        expect(gplan.apply(vec3()).empty() && gplan.apply_cube(vec3(Y, vec2(X, vec()))).size() == (size_t)OY, "no levels and no members give empty results");
    }
    expect(throws<std::invalid_argument>([&] { DownscalingPlan(igrid, opoints, (Downscaler)7); }), "an unknown downscaler is refused");
    expect(throws<std::invalid_argument>([&] { DownscalingPlan(igrid, Points(plats, plons, vec(), vec(), Cartesian), Nearest); }), "Nearest refuses another coordinate type");

    // the plan outlives the sets it was built from; it moves, and the moved-to plan owns the records
    vec later;
    const vec want = downscaling(igrid, opoints, values, Bilinear);
    {
        Grid* g = new Grid(lats, lons);
        Points* p = new Points(plats, plons);
        DownscalingPlan first(*g, *p, Bilinear);
        delete g;
        delete p;
        DownscalingPlan second(std::move(first));
        DownscalingPlan third(igrid, ogrid, Nearest);
        third = std::move(second);
        later = third.apply_points(values);
    }
    expect(same(later, want), "a moved plan outlives the sets it was built from");
    expect(!std::is_copy_constructible<DownscalingPlan>::value && !std::is_copy_assignable<DownscalingPlan>::value, "a plan is not copyable");
    expect(std::is_nothrow_move_constructible<DownscalingPlan>::value, "a plan is movable");
    if(failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
