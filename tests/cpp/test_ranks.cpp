// calc_ranks, sort_rows, reorder_by_ranks and calc_crps through the C++ header of their own (gridpp_amd/host/gridpp_ranks.hpp), written as a
// program for it would call them: the twelve signatures taken by address with their exact types, known answers, a ragged vec2, the empty
// shapes and the exceptions with their messages.  The case file holds two cubes and a reference field as hex words; every result is printed
// the same way, and tests/test_gpu_ranks_cpp.py compares it bit for bit with the Python functions.  Built and run by that file.
#include "gridpp_ranks.hpp"
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
static bool eq(float a, float b) { return (std::isnan(a) && std::isnan(b)) || std::memcmp(&a, &b, sizeof a) == 0; }   // bit for bit
static bool eq(const vec& a, const vec& b) {
    if(a.size() != b.size()) return false;
    for(size_t i = 0; i < a.size(); i++) if(!eq(a[i], b[i])) return false;
    return true;
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
static vec3 cube_of(const vec& f, size_t Y, size_t X, size_t T) {
    vec3 c(Y, vec2(X, vec(T)));
    for(size_t y = 0; y < Y; y++)
        for(size_t x = 0; x < X; x++)
            for(size_t t = 0; t < T; t++) c[y][x][t] = f[(y * X + x) * T + t];
    return c;
}
static void print(const char* name, const vec& v) {
    std::printf("%s %zu", name, v.size());
    for(float x : v) { unsigned u; std::memcpy(&u, &x, sizeof u); std::printf(" %08x", u); }
    std::printf("\n");
}
static void print(const char* name, const ivec& v) {
    std::printf("%s %zu", name, v.size());
    for(int x : v) std::printf(" %08x", (unsigned)x);
    std::printf("\n");
}
template <class T> static std::vector<T> flat(const std::vector<std::vector<T>>& a) { std::vector<T> f; for(const auto& r : a) f.insert(f.end(), r.begin(), r.end()); return f; }
template <class T> static std::vector<T> flat(const std::vector<std::vector<std::vector<T>>>& a) { std::vector<T> f; for(const auto& p : a) for(const auto& r : p) f.insert(f.end(), r.begin(), r.end()); return f; }

int main(int argc, char** argv) {
    // the twelve signatures, exactly
    ivec (*r1)(const vec&) = &calc_ranks;
    ivec2 (*r2)(const vec2&) = &calc_ranks;
    ivec3 (*r3)(const vec3&) = &calc_ranks;
    vec (*s1)(const vec&) = &sort_rows;
    vec2 (*s2)(const vec2&) = &sort_rows;
    vec3 (*s3)(const vec3&) = &sort_rows;
    vec (*o1)(const vec&, const vec&) = &reorder_by_ranks;
    vec2 (*o2)(const vec2&, const vec2&) = &reorder_by_ranks;
    vec3 (*o3)(const vec3&, const vec3&) = &reorder_by_ranks;
    float (*c1)(const vec&, float) = &calc_crps;
    vec (*c2)(const vec2&, const vec&) = &calc_crps;
    vec2 (*c3)(const vec3&, const vec2&) = &calc_crps;
    const float nan = std::nanf(""), inf = INFINITY;

    // known answers: ties by position, the zeros of either sign, invalid values
    expect(r1({3, 1, nan, 1, inf, 0.0f, -0.0f}) == ivec{4, 2, -1, 3, -1, 0, 1}, "ranks: known answers");
    expect(eq(s1({3, 1, nan, 1, inf, 0.0f, -0.0f}), vec{0.0f, -0.0f, 1, 1, 3, nan, nan}), "sorted: known answers, the bits of the zeros kept");
    expect(eq(o1({10, nan, 30, 20}, {0.5f, 0.1f, 0.9f, 0.7f}), vec{20, 10, nan, 30}), "reorder: a rank beyond the valid values");
    expect(eq(o1({0.5f, 0.1f, 0.9f, 0.7f}, {10, nan, 30, 20}), vec{0.1f, nan, 0.7f, 0.5f}), "reorder: an invalid template value");
    expect(c1({5, nan}, 7) == 2.0f && c1({2, 2, 2}, 2) == 0.0f, "crps: N = 1 and y equal to every member");
    expect(std::isnan(c1({nan, inf}, 0)) && std::isnan(c1({1, 2}, nan)) && std::isnan(c1({1, 2}, inf)) && std::isnan(c1({}, 1)), "crps: NaN");
    expect(std::fabs(c1({1, 2, 3}, 2) - (2.0f / 3 - 4.0f / 9)) < 1e-7f, "crps: 1 2 3 against 2");
    expect(r1({}).empty() && s1({}).empty() && o1({}, {}).empty(), "vec: no values");
    // a ragged vec2: rows padded with NaN for the call, results at the rows' own lengths, an empty row
    const vec2 ragged = {{4, 2, 3, 1}, {10}, {}, {5, nan, 1}};
    const ivec2 rr = r2(ragged);
    const vec2 rs = s2(ragged), ro = o2(ragged, ragged);
    expect(rr.size() == 4 && rr[0] == ivec{3, 1, 2, 0} && rr[1] == ivec{0} && rr[2].empty() && rr[3] == ivec{1, -1, 0}, "ragged ranks");
    expect(rs.size() == 4 && eq(rs[0], vec{1, 2, 3, 4}) && eq(rs[1], vec{10}) && rs[2].empty() && eq(rs[3], vec{1, 5, nan}), "ragged sorted rows");
    for(size_t n = 0; n < ragged.size(); n++) {
        expect(rr[n] == r1(ragged[n]) && eq(rs[n], s1(ragged[n])), "ragged row == the vec form");
        expect(eq(ro[n], ragged[n]), "reorder by its own ranks is the identity");
    }
    expect(eq(c2(ragged, {2, 10, 0, 3}), vec{c1(ragged[0], 2), 0.0f, nan, c1(ragged[3], 3)}), "ragged crps");
    expect(r2(vec2()).empty() && s2(vec2()).empty() && o2(vec2(), vec2()).empty() && c2(vec2(), vec()).empty(), "vec2: no rows");
    expect(r3(vec3()).empty() && s3(vec3()).empty() && o3(vec3(), vec3()).empty() && c3(vec3(), vec2()).empty(), "vec3: no cells");
    // exceptions
    const vec3 a(2, vec2(3, vec(4, 1.0f))), b(2, vec2(3, vec(5, 2.0f))), c(2, vec2(2, vec(4, 1.0f))), d(3, vec2(3, vec(4, 1.0f)));
    const std::string same = "reorder_by_ranks: values and template must have the same shape";
    expect(message_of([&] { o1({1, 2}, {1, 2, 3}); }) == same, "vec: lengths differ");
    expect(message_of([&] { o2(ragged, {{4, 2, 3, 1}, {10}, {}, {5, 1}}); }) == same, "vec2: a row differs");
    expect(message_of([&] { o2(ragged, {{4, 2, 3, 1}}); }) == same, "vec2: rows differ");
    expect(message_of([&] { o3(a, b); }) == same && message_of([&] { o3(a, c); }) == same && message_of([&] { o3(a, d); }) == same, "vec3: shapes differ");
    const std::string shape = "calc_crps: ref must have the shape of ensemble without its last axis";
    expect(message_of([&] { c2(ragged, {1, 2, 3}); }) == shape, "crps vec2: ref of another length");
    expect(message_of([&] { c3(a, vec2(2, vec(2, 0.0f))); }) == shape && message_of([&] { c3(a, vec2(3, vec(3, 0.0f))); }) == shape, "crps vec3: ref of another shape");

    // the case of the Python test
    if(argc > 1) {
        std::ifstream in(argv[1]);
        size_t Y, X, E;
        in >> Y >> X >> E;
        const vec3 vals = cube_of(read_words(in, Y * X * E), Y, X, E), tmpl = cube_of(read_words(in, Y * X * E), Y, X, E);
        const vec reff = read_words(in, Y * X);
        expect((bool)in, "case file");
        vec2 ref2(Y, vec(X));
        for(size_t y = 0; y < Y; y++) for(size_t x = 0; x < X; x++) ref2[y][x] = reff[y * X + x];
        print("ranks_vec", r1(vals[0][0]));
        print("ranks_rows", flat(r2(vals[0])));
        print("ranks_cube", flat(r3(vals)));
        print("sorted_vec", s1(vals[0][0]));
        print("sorted_rows", flat(s2(vals[0])));
        print("sorted_cube", flat(s3(vals)));
        print("reorder_vec", o1(vals[0][0], tmpl[0][0]));
        print("reorder_rows", flat(o2(vals[0], tmpl[0])));
        print("reorder_cube", flat(o3(vals, tmpl)));
        print("crps_vec", vec{c1(vals[0][0], ref2[0][0])});
        print("crps_rows", c2(vals[0], ref2[0]));
        print("crps_cube", flat(c3(vals, ref2)));
        vec2 rag = vals[1];
        for(size_t x = 0; x < X; x++) rag[x].resize(E - x);
        print("ranks_ragged", flat(r2(rag)));
        print("sorted_ragged", flat(s2(rag)));
        print("crps_ragged", c2(rag, ref2[1]));
    }
    if(failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
