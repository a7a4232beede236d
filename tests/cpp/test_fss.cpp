// fractions_skill_score through the C++ header of its own (gridpp_amd/host/gridpp_fss.hpp), written as a program for it would call it: the two
// signatures taken by address with their exact types, the default operator, the hand-worked 3 x 3 answers, the shapes that need no device and
// the exceptions with their messages.  The case file holds a cube and a reference field as hex words; every result is printed as the hex words
// of its doubles, and tests/test_gpu_fss_cpp.py compares them bit for bit with the Python function.  Built and run by that file.
#include "gridpp_fss.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
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
static vec read_words(std::ifstream& in, size_t n) {
    vec v(n);
    for(size_t i = 0; i < n; i++) {
        std::string w;
        in >> w;
        const unsigned u = (unsigned)std::strtoul(w.c_str(), nullptr, 16);
        std::memcpy(&v[i], &u, sizeof u);
    }
    return v;
}
static void print(const std::string& name, const FssResult& r) {
    const dvec2* parts[3] = {&r.fss, &r.fbs, &r.fbs_worst};
    const char* names[3] = {"fss", "fbs", "worst"};
    for(int p = 0; p < 3; p++) {
        size_t n = 0;
        for(const auto& row : *parts[p]) n += row.size();
        std::printf("%s_%s %zu", name.c_str(), names[p], n);
        for(const auto& row : *parts[p])
            for(double x : row) { unsigned long long u; std::memcpy(&u, &x, sizeof u); std::printf(" %016llx", u); }
        std::printf("\n");
    }
    std::printf("%s_cells %zu", name.c_str(), r.cells.size());
    for(long long c : r.cells) std::printf(" %016llx", (unsigned long long)c);
    std::printf("\n");
}
static bool close(double got, double want) { return std::fabs(got - want) <= 4 * (std::nextafter(std::fabs(want), INFINITY) - std::fabs(want)); }

int main(int argc, char** argv) {
    // the two signatures, exactly
    FssResult (*f2)(const vec2&, const vec2&, const vec&, const ivec&, ComparisonOperator) = &fractions_skill_score;
    FssResult (*f3)(const vec3&, const vec2&, const vec&, const ivec&, ComparisonOperator) = &fractions_skill_score;
    const float nan = std::nanf("");

    // the hand-worked answers; the default operator is Gt
    vec2 f(3, vec(3, 0.0f)), r(3, vec(3, 0.0f));
    f[0][0] = 1; r[2][2] = 1;
    const FssResult a = fractions_skill_score(f, r, {0.5f}, {0, 1, 2});
    expect(a.fss.size() == 1 && a.fss[0].size() == 3 && a.cells == std::vector<long long>{9, 9, 9}, "3 x 3: shapes and cells");
    expect(a.fbs[0][0] == 2 && a.fbs_worst[0][0] == 2 && a.fss[0][0] == 0, "3 x 3: h = 0");
    expect(close(a.fbs[0][1], 17.0 / 72) && close(a.fbs_worst[0][1], 169.0 / 648) && std::fabs(a.fss[0][1] - 16.0 / 169) < 1e-14, "3 x 3: h = 1");
    expect(a.fbs[0][2] == 0 && close(a.fbs_worst[0][2], 2.0 / 9) && a.fss[0][2] == 1, "3 x 3: h = 2");
    const FssResult g = f2(f, r, {0.5f}, {0, 1, 2}, Gt), l = f2(f, r, {0.5f}, {0, 1, 2}, Leq);
    expect(g.fbs == a.fbs && g.fbs_worst == a.fbs_worst && g.cells == a.cells, "the default operator is Gt");
    expect(l.fbs[0][0] == 2 && l.fbs_worst[0][0] == 16, "Leq at h = 0: the complements");
    expect(std::isnan(f2(f, r, {5.0f}, {1}, Gt).fss[0][0]), "no event in either field: NaN");
    const vec3 cube(3, vec2(3, vec(4, 1.0f)));
    const FssResult c = f3(cube, r, {0.5f, INFINITY}, {1}, Gt);
    expect(c.fss.size() == 2 && c.cells == std::vector<long long>{9} && std::isnan(c.fss[1][0]) && c.fss[0][0] < 1, "a cube, an infinite threshold");

    // the shapes that need no device
    const FssResult none = f2(f, r, {}, {1, 2}, Gt), noh = f2(f, r, {0.5f}, {}, Gt), empty = f2(vec2(), vec2(), {0.5f}, {1, 2}, Gt);
    expect(none.fss.empty() && none.cells == std::vector<long long>{0, 0}, "no threshold");
    expect(noh.fss.size() == 1 && noh.fss[0].empty() && noh.cells.empty(), "no half width");
    expect(empty.fss.size() == 1 && std::isnan(empty.fss[0][0]) && std::isnan(empty.fss[0][1]) && empty.fbs[0][0] == 0 && empty.fbs_worst[0][1] == 0 &&
               empty.cells == std::vector<long long>{0, 0}, "an empty field");
    expect(std::isnan(f3(vec3(3, vec2(3, vec())), r, {0.5f}, {1}, Gt).fss[0][0]), "a cube without members");

    // exceptions
    expect(message_of([&] { f2(f, vec2(3, vec(4, 0.0f)), {0.5f}, {1}, Gt); }) == "fractions_skill_score: ref must have the shape (Y, X) of fcst", "ref of another shape");
    expect(message_of([&] { f3(cube, vec2(2, vec(3, 0.0f)), {0.5f}, {1}, Gt); }) == "fractions_skill_score: ref must have the shape (Y, X) of fcst", "cube: ref of another shape");
    expect(message_of([&] { f2(f, r, {0.5f, nan}, {-1}, (ComparisonOperator)5); }) == "fractions_skill_score: a threshold is NaN", "a NaN threshold comes first");
    expect(message_of([&] { f2(f, r, {0.5f}, {1, -1}, (ComparisonOperator)5); }) == "Half width must be > 0", "a negative half width");
    expect(message_of([&] { f2(f, r, {0.5f}, {1}, (ComparisonOperator)5); }) == "Invalid comparison operator", "the operator");

    // the case of the Python test
    if(argc > 1) {
        std::ifstream in(argv[1]);
        size_t Y, X, E;
        in >> Y >> X >> E;
        const vec cf = read_words(in, Y * X * E), rf = read_words(in, Y * X);
        expect((bool)in, "case file");
        vec3 cb(Y, vec2(X, vec(E)));
        vec2 first(Y, vec(X)), ref(Y, vec(X));
        for(size_t y = 0; y < Y; y++)
            for(size_t x = 0; x < X; x++) {
                for(size_t e = 0; e < E; e++) cb[y][x][e] = cf[(y * X + x) * E + e];
                first[y][x] = cb[y][x][0];
                ref[y][x] = rf[y * X + x];
            }
        const vec thr = {-0.2f, 0.4f, 1.0f};
        const ivec hws = {0, 2, 16, 40};
        print("field_gt", f2(first, ref, thr, hws, Gt));
        print("field_lt", f2(first, ref, thr, hws, Lt));
        print("cube_gt", f3(cb, ref, thr, hws, Gt));
        print("cube_geq", f3(cb, ref, thr, hws, Geq));
    }
    if(failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
