// calc_quantiles and quantile_mapping_curves through the C++ header of their own (gridpp_amd/host/gridpp_quantiles.hpp), written as a program
// for it would call them: the four signatures taken by address with their exact types, known answers, a ragged vec2, the empty shapes and
// the exceptions with their messages.  The case file holds cubes and levels as hex words; every result is printed the same way, and
// tests/test_gpu_quantiles_cpp.py compares it bit for bit with the Python functions.  Built and run by that file.
#include "gridpp_quantiles.hpp"
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
static vec flat(const vec2& a) { vec f; for(const auto& r : a) f.insert(f.end(), r.begin(), r.end()); return f; }
static vec flat(const vec3& a) { vec f; for(const auto& p : a) for(const auto& r : p) f.insert(f.end(), r.begin(), r.end()); return f; }

int main(int argc, char** argv) {
    // the four signatures, exactly
    vec (*f1)(const vec&, const vec&) = &calc_quantiles;
    vec2 (*f2)(const vec2&, const vec&) = &calc_quantiles;
    vec3 (*f3)(const vec3&, const vec&) = &calc_quantiles;
    vec3 (*f4)(const vec3&, const vec3&, vec3&, const vec&) = &quantile_mapping_curves;
    const float nan = std::nanf("");

    // known answers: interpolation between order statistics, positional Min / Max (the first of equal values), a NaN level, repeats
    expect(eq(f1({4, 1, nan, 3, 2, 5}, {0.5f, 0.0f, 1.0f, 0.25f, nan, 0.125f, 0.5f}), vec{3, 1, 5, 2, nan, 1.5f, 3}), "vec: known answers");
    expect(eq(f1({0.0f, -0.0f}, {0.0f, 0.5f, 1.0f}), vec{0.0f, 0.0f, 0.0f}), "vec: the first zero is Min and Max");   // (-0 + (0 - -0) / 2 = +0)
    expect(eq(f1({-0.0f, 0.0f, nan}, {0.0f, 0.5f, 1.0f}), vec{-0.0f, 0.0f, -0.0f}), "vec: the first zero is Min and Max (2)");
    expect(eq(f1({}, {0.5f, 0.1f}), vec{nan, nan}), "vec: no values");
    expect(f1({1, 2}, {}).empty(), "vec: no levels");
    // a ragged vec2: rows padded with NaN, an empty row
    const vec2 ragged = {{1, 2, 3, 4}, {10}, {}, {5, nan, 1}};
    const vec2 got = f2(ragged, {0.5f, 1.0f});
    expect(got.size() == 4 && eq(got[0], vec{2.5f, 4}) && eq(got[1], vec{10, 10}) && eq(got[2], vec{nan, nan}) && eq(got[3], vec{3, 5}), "ragged rows");
    for(size_t n = 0; n < ragged.size(); n++) {
        expect(eq(got[n], f1(ragged[n], {0.5f, 1.0f})), "ragged row == the vec form");
        expect(eq(got[n][0], calc_quantile(ragged[n], 0.5f)), "ragged row == calc_quantile");
    }
    expect(f2(vec2(), {0.5f}).empty(), "vec2: no rows");
    const vec2 nolevels = f2(ragged, {});
    expect(nolevels.size() == 4 && nolevels[0].empty(), "vec2: no levels");
    expect(f3(vec3(), {0.5f}).empty(), "vec3: no cells");
    // exceptions
    const vec3 a(2, vec2(3, vec(4, 1.0f))), b(2, vec2(3, vec(5, 2.0f))), c(2, vec2(2, vec(4, 1.0f))), d(3, vec2(3, vec(4, 1.0f)));
    vec3 o;
    const std::string range = "calc_quantiles: Quantiles must be between 0 and 1 inclusive";
    expect(message_of([&] { f1({1, 2}, {0.5f, 1.5f}); }) == range, "vec: a level above 1");
    expect(message_of([&] { f2(ragged, {-0.1f}); }) == range, "vec2: a level below 0");
    expect(message_of([&] { f3(a, {2.0f}); }) == range, "vec3: a level above 1");
    expect(message_of([&] { f1({}, {1.5f}); }) == range, "no values do not hide a bad level");
    const std::string dims = "quantile_mapping_curves: ref and fcst must have the same first two dimensions";
    expect(message_of([&] { f4(a, c, o, {0.5f}); }) == dims, "curves: X differs");
    expect(message_of([&] { f4(a, d, o, {}); }) == dims, "curves: Y differs (before the empty levels)");
    expect(message_of([&] { f4(a, b, o, {}); }) == "quantile_mapping_curves: empty quantiles: the sorted-rows form is not built", "curves: no levels");
    expect(message_of([&] { f4(a, b, o, {0.5f, nan}); }) == "Quantiles must be >= 0 and <= 1", "curves: a NaN level");
    expect(message_of([&] { f4(a, b, o, {1.5f}); }) == "Quantiles must be >= 0 and <= 1", "curves: a level above 1");
    const vec3 cr = f4(a, b, o, {0.0f, 0.5f, 1.0f});
    expect(cr.size() == 2 && cr[0].size() == 3 && eq(cr[1][2], vec{1, 1, 1}) && o.size() == 2 && o[0].size() == 3 && eq(o[1][2], vec{2, 2, 2}), "curves: constant cubes");

    // the case of the Python test
    if(argc > 1) {
        std::ifstream in(argv[1]);
        size_t Y, X, Tr, Tf, Q, K;
        in >> Y >> X >> Tr >> Tf >> Q >> K;
        const vec3 ref = cube_of(read_words(in, Y * X * Tr), Y, X, Tr), fcst = cube_of(read_words(in, Y * X * Tf), Y, X, Tf);
        const vec levels = read_words(in, Q), knots = read_words(in, K);   // (the knots of the curves hold no NaN)
        expect((bool)in, "case file");
        print("vec", f1(ref[0][0], levels));
        print("rows", flat(f2(ref[0], levels)));
        print("cube", flat(f3(ref, levels)));
        vec2 rag = ref[1];
        for(size_t x = 0; x < X; x++) rag[x].resize(Tr - x);
        print("ragged", flat(f2(rag, levels)));
        vec3 curve_fcst;
        print("curve_ref", flat(f4(ref, fcst, curve_fcst, knots)));
        print("curve_fcst", flat(curve_fcst));
    }
    if(failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
