// neighbourhood_quantiles_fast and neighbourhood_cdf through the C++ header of their own (gridpp_amd/host/gridpp_nbh_quantiles.hpp), written as a
// program for it would call them: the four signatures taken by address with their exact types, every level plane against neighbourhood_quantile_fast
// of gridpp.hpp, the empty shapes and the exceptions with their messages, and the device-pointer forms against the host forms.  The case file holds a
// cube, levels and thresholds as hex words; every result is printed the same way, and tests/test_gpu_nbh_quantiles_cpp.py compares it bit for bit
// with the Python functions.  Built and run by that file.
#include "gridpp_nbh_quantiles.hpp"
#include <algorithm>
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
static vec plane(const vec3& a, size_t j) { vec f; for(const auto& p : a) for(const auto& r : p) f.push_back(r[j]); return f; }
static void first_member(const vec3& a, vec2& out) {
    out.assign(a.size(), vec());
    for(size_t y = 0; y < a.size(); y++) for(const auto& c : a[y]) out[y].push_back(c[0]);
}
// a host array in HBM: the device forms take what hipMalloc gives (the three runtime calls declared here, so that the program needs no HIP headers)
extern "C" int hipMalloc(void**, size_t);
extern "C" int hipFree(void*);
extern "C" int hipMemcpy(void*, const void*, size_t, int);
static float* to_device(const vec& v) {
    void* p = nullptr;
    if(hipMalloc(&p, std::max<size_t>(v.size(), 1) * sizeof(float)) != 0) return nullptr;
    if(!v.empty() && hipMemcpy(p, v.data(), v.size() * sizeof(float), 1 /* hipMemcpyHostToDevice */) != 0) return nullptr;
    return static_cast<float*>(p);
}
static vec from_device(const float* p, size_t n) {
    vec v(n);
    if(n && hipMemcpy(v.data(), p, n * sizeof(float), 2 /* hipMemcpyDeviceToHost */) != 0) v.assign(n, -12345.0f);
    return v;
}

int main(int argc, char** argv) {
    // the four signatures, exactly
    vec3 (*f1)(const vec2&, const vec&, int, const vec&) = &neighbourhood_quantiles_fast;
    vec3 (*f2)(const vec3&, const vec&, int, const vec&) = &neighbourhood_quantiles_fast;
    vec3 (*f3)(const vec2&, const vec&, int) = &neighbourhood_cdf;
    vec3 (*f4)(const vec3&, const vec&, int) = &neighbourhood_cdf;
    void (*f5)(const float*, int, int, int, bool, const vec&, int, const float*, int, float*) = &neighbourhood_quantiles_fast_device;
    void (*f6)(const float*, int, int, int, bool, const float*, int, int, float*) = &neighbourhood_cdf_device;
    const float nan = std::nanf("");

    // known answers: one cell with three valid members of four -- fractions 0, 1/3, 2/3, 1 and their 4-fold float sums
    const vec3 one = {{{1, 2, 3, nan}}};
    const vec thr4 = {0, 1, 2.5f, 3};
    const vec3 c1 = f4(one, thr4, 0);
    expect(c1.size() == 1 && c1[0].size() == 1 && c1[0][0].size() == 4, "cdf: shape");
    if(c1.size() == 1 && c1[0].size() == 1 && c1[0][0].size() == 4) {
        const float third = 1.0f / 3.0f, s = ((third + third) + third) + third;
        expect(eq(c1[0][0][0], 0.0f) && eq(c1[0][0][1], s / 4) && eq(c1[0][0][3], 1.0f), "cdf: one cell");
        expect(std::fabs(c1[0][0][2] - 2.0f / 3.0f) < 1e-6f, "cdf: two thirds");
    }
    expect(eq(flat(f2(one, {0.0f, 1.0f, nan}, 0, thr4)), vec{0, 3, nan}), "levels: one cell");
    expect(eq(flat(f2(one, {0.5f}, 0, {})), vec{nan}), "levels: no thresholds");
    const vec3 none = f2(one, {}, 0, thr4);
    expect(none.size() == 1 && none[0].size() == 1 && none[0][0].empty(), "levels: no levels");
    const vec3 nothr = f4(one, {}, 0);
    expect(nothr.size() == 1 && nothr[0].size() == 1 && nothr[0][0].empty(), "cdf: no thresholds");
    expect(f1(vec2(), {0.5f}, 1, thr4).empty() && f2(vec3(), {0.5f}, 1, thr4).empty() && f3(vec2(), thr4, 1).empty() && f4(vec3(), thr4, 1).empty(), "empty fields");
    expect(f2(vec3(), {1.5f}, 1, thr4).empty(), "an empty field comes before the levels");
    // exceptions
    const std::string hw = "Half width must be > 0", range = "All quantiles must be >= 0 and <= 1";
    expect(message_of([&] { f2(one, {1.5f}, -1, thr4); }) == hw, "levels: halfwidth first");
    expect(message_of([&] { f1(vec2(), {0.5f}, -1, thr4); }) == hw, "levels: halfwidth before the empty field");
    expect(message_of([&] { f4(one, thr4, -1); }) == hw && message_of([&] { f3(vec2(), thr4, -3); }) == hw, "cdf: halfwidth");
    expect(message_of([&] { f2(one, {0.5f, 1.5f}, 0, thr4); }) == range, "levels: a level above 1");
    expect(message_of([&] { f1({{1, 2}}, {-0.25f}, 0, thr4); }) == range, "levels: a level below 0");
    expect(message_of([&] { f2(one, {2.0f}, 0, {}); }) == range, "levels: no thresholds do not hide a bad level");

    // the case of the Python test
    if(argc > 1) {
        std::ifstream in(argv[1]);
        size_t Y, X, E, Q, T;
        int halfwidth;
        in >> Y >> X >> E >> Q >> T >> halfwidth;
        const vec cube_flat = read_words(in, Y * X * E);
        const vec3 cube = cube_of(cube_flat, Y, X, E);
        const vec levels = read_words(in, Q), thr = read_words(in, T);
        expect((bool)in, "case file");
        const vec3 lv = f2(cube, levels, halfwidth, thr);
        print("levels3", flat(lv));
        for(size_t j = 0; j < Q; j++)
            expect(eq(plane(lv, j), flat(neighbourhood_quantile_fast(cube, levels[j], halfwidth, thr))), "a level plane == neighbourhood_quantile_fast of gridpp.hpp");
        print("cdf3", flat(f4(cube, thr, halfwidth)));
        vec2 field;
        first_member(cube, field);
        const vec3 lv2 = f1(field, levels, halfwidth, thr);
        print("levels2", flat(lv2));
        for(size_t j = 0; j < Q; j++)
            expect(eq(plane(lv2, j), flat(neighbourhood_quantile_fast(field, levels[j], halfwidth, thr))), "2-D: a level plane == neighbourhood_quantile_fast");
        print("cdf2", flat(f3(field, thr, halfwidth)));
        // the device-pointer forms
        float* d_cube = to_device(cube_flat); float* d_thr = to_device(thr);
        float* d_lv = to_device(vec(Y * X * Q)); float* d_cdf = to_device(vec(Y * X * T));
        expect(d_cube && d_thr && d_lv && d_cdf, "device allocations");
        if(d_cube && d_thr && d_lv && d_cdf) {
            f5(d_cube, (int)Y, (int)X, (int)E, true, levels, halfwidth, d_thr, (int)T, d_lv);
            f6(d_cube, (int)Y, (int)X, (int)E, true, d_thr, (int)T, halfwidth, d_cdf);
            print("levels3_device", from_device(d_lv, Y * X * Q));
            print("cdf3_device", from_device(d_cdf, Y * X * T));
            expect(message_of([&] { f5(d_cube, (int)Y, (int)X, (int)E, true, {1.5f}, halfwidth, d_thr, (int)T, d_lv); }) == range, "device form: a level above 1");
            expect(message_of([&] { f6(d_cube, (int)Y, (int)X, (int)E, true, d_thr, (int)T, -1, d_cdf); }) == hw, "device form: halfwidth");
        }
        hipFree(d_cube); hipFree(d_thr); hipFree(d_lv); hipFree(d_cdf);
    }
    if(failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
