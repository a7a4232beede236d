// neighbourhood_members and calc_gradient_members through the C++ header of their own (gridpp_amd/host/gridpp_members.hpp), written as a program
// for it would call them: the signatures taken by address with their exact types, known answers, the empty shapes and the exceptions with their
// messages, every plane against neighbourhood / calc_gradient of gridpp.hpp, and the device-pointer forms.  The case file holds a cube, a shared
// base and a base per member as hex words; every result is printed the same way, and tests/test_gpu_members_cpp.py compares it bit for bit with
// the Python functions.  Built and run by that file.
#include "gridpp_members.hpp"
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
static vec3 cube_of(const vec& f, size_t Y, size_t X, size_t E) {
    vec3 c(Y, vec2(X, vec(E)));
    for(size_t y = 0; y < Y; y++)
        for(size_t x = 0; x < X; x++)
            for(size_t e = 0; e < E; e++) c[y][x][e] = f[(y * X + x) * E + e];
    return c;
}
static vec2 field_of(const vec& f, size_t Y, size_t X) {
    vec2 c(Y, vec(X));
    for(size_t y = 0; y < Y; y++)
        for(size_t x = 0; x < X; x++) c[y][x] = f[y * X + x];
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
static vec2 member(const vec3& a, size_t j) {
    vec2 out(a.size());
    for(size_t y = 0; y < a.size(); y++) for(const auto& c : a[y]) out[y].push_back(c[j]);
    return out;
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
    // the signatures, exactly
    vec3 (*f1)(const vec3&, int, Statistic) = &neighbourhood_members;
    vec3 (*f2)(const vec2&, const vec3&, GradientType, int, int, float, float) = &calc_gradient_members;
    vec3 (*f3)(const vec3&, const vec3&, GradientType, int, int, float, float) = &calc_gradient_members;
    void (*f4)(const float*, int, int, int, int, Statistic, float*) = &neighbourhood_members_device;
    void (*f5)(const float*, int, const float*, int, int, int, GradientType, int, int, float, float, float*) = &calc_gradient_members_device;
    const float nan = std::nanf("");

    // known answers: a row of three cells with two members, one value missing
    const vec3 row = {{{1, 10}, {2, nan}, {6, 30}}};
    expect(eq(flat(f1(row, 1, Mean)), vec{1.5f, 10, 3, 20, 4, 30}), "Mean of a row");
    expect(eq(flat(f1(row, 1, Count)), vec{2, 1, 3, 2, 2, 1}), "Count of a row");
    expect(eq(flat(f1(row, 5, Max)), vec{6, 30, 6, 30, 6, 30}), "Max over the whole row");
    expect(eq(flat(f1(row, 0, Sum)), vec{1, 10, 2, nan, 6, 30}), "Sum at halfwidth 0");
    expect(eq(flat(f2({{0, 1, 2}}, row, MinMax, 1, 2, MV, 0)), vec{1, 0, 2.5f, 10, 4, 0}), "MinMax gradient of a row");
    expect(f1(vec3(), 1, Mean).empty() && f1(vec3(2, vec2()), 1, Max).empty(), "empty cubes");
    // exceptions
    const std::string hw = "Half width must be > 0", median = "neighbourhood_members does not compute the statistic Median: order statistics per member are not supported";
    expect(message_of([&] { f1(row, -1, Quantile); }) == hw && message_of([&] { f1(vec3(), -1, Mean); }) == hw, "halfwidth first");
    expect(message_of([&] { f1(row, 1, Quantile); }) == "Use neighbourhood_quantile for computing neighbourhood quantiles", "Quantile");
    expect(message_of([&] { f1(row, 1, Median); }) == median && message_of([&] { f1(vec3(), 1, Median); }) == median, "Median");
    expect(message_of([&] { f1(row, 1, RandomChoice); }).find("RandomChoice") != std::string::npos, "RandomChoice");
    expect(message_of([&] { f2({{0, 1, 2}}, row, MinMax, 0, -1, -1, 0); }) == "Halwidth cannot be <= 0; must be positive integer", "gradient: halfwidth first");
    expect(message_of([&] { f2({{0, 1, 2}}, row, MinMax, 1, -1, -1, 0); }) == "min_range must be >= 0", "gradient: min_range");
    expect(message_of([&] { f2({{0, 1, 2}}, row, MinMax, 1, -1, MV, 0); }) == "num_min must be >= 0", "gradient: num_min");
    expect(message_of([&] { f2(vec2(), row, MinMax, 1, 2, MV, 0); }) == "base input has no size", "gradient: no base");
    expect(message_of([&] { f2({{0, 1}}, row, MinMax, 1, 2, MV, 0); }) == "base is not the same size as values", "gradient: a narrower base");
    expect(message_of([&] { f3({{{1}, {2}, {6}}}, row, MinMax, 1, 2, MV, 0); }) == "base is not the same size as values", "gradient: a base with fewer members");
    expect(message_of([&] { f2({{0, 1, 2}}, row, (GradientType)5, 1, 2, MV, 0); }) == "unknown gradient type", "gradient: type");

    // the case of the Python test
    if(argc > 1) {
        std::ifstream in(argv[1]);
        size_t Y, X, E;
        int halfwidth;
        in >> Y >> X >> E >> halfwidth;
        const vec cube_flat = read_words(in, Y * X * E), shared_flat = read_words(in, Y * X), per_flat = read_words(in, Y * X * E);
        expect((bool)in, "case file");
        const vec3 cube = cube_of(cube_flat, Y, X, E), per = cube_of(per_flat, Y, X, E);
        const vec2 shared = field_of(shared_flat, Y, X);
        const Statistic stats[] = {Mean, Sum, Count, Min, Max, Std, Variance};
        const char* names[] = {"Mean", "Sum", "Count", "Min", "Max", "Std", "Variance"};
        float* d_cube = to_device(cube_flat); float* d_shared = to_device(shared_flat); float* d_per = to_device(per_flat); float* d_out = to_device(vec(Y * X * E));
        expect(d_cube && d_shared && d_per && d_out, "device allocations");
        const bool dev = d_cube && d_shared && d_per && d_out;
        for(int k = 0; k < 7; k++) {
            const vec3 r = f1(cube, halfwidth, stats[k]);
            print(names[k], flat(r));
            for(size_t e = 0; e < E; e++) expect(eq(plane(r, e), flat(neighbourhood(member(cube, e), halfwidth, stats[k]))), "a plane == neighbourhood of gridpp.hpp");
            if(dev) {
                f4(d_cube, (int)Y, (int)X, (int)E, halfwidth, stats[k], d_out);
                print((std::string(names[k]) + "_device").c_str(), from_device(d_out, Y * X * E));
            }
        }
        const GradientType types[] = {MinMax, LinearRegression};
        const char* tnames[] = {"MinMax", "LinearRegression"};
        for(int k = 0; k < 2; k++) {
            const vec3 gs = f2(shared, cube, types[k], halfwidth, 2, MV, 0), gp = f3(per, cube, types[k], halfwidth, 3, 1.0f, -0.5f);
            print((std::string(tnames[k]) + "_shared").c_str(), flat(gs));
            print((std::string(tnames[k]) + "_per").c_str(), flat(gp));
            for(size_t e = 0; e < E; e++) {
                expect(eq(plane(gs, e), flat(calc_gradient(shared, member(cube, e), types[k], halfwidth, 2, MV, 0))), "shared base: a plane == calc_gradient of gridpp.hpp");
                expect(eq(plane(gp, e), flat(calc_gradient(member(per, e), member(cube, e), types[k], halfwidth, 3, 1.0f, -0.5f))), "base per member: a plane == calc_gradient");
            }
            if(dev) {
                f5(d_shared, 1, d_cube, (int)Y, (int)X, (int)E, types[k], halfwidth, 2, MV, 0, d_out);
                print((std::string(tnames[k]) + "_shared_device").c_str(), from_device(d_out, Y * X * E));
                f5(d_per, (int)E, d_cube, (int)Y, (int)X, (int)E, types[k], halfwidth, 3, 1.0f, -0.5f, d_out);
                print((std::string(tnames[k]) + "_per_device").c_str(), from_device(d_out, Y * X * E));
            }
        }
        if(dev) {
            expect(message_of([&] { f4(d_cube, (int)Y, (int)X, (int)E, -1, Mean, d_out); }) == hw, "device form: halfwidth");
            expect(message_of([&] { f5(d_shared, 2, d_cube, (int)Y, (int)X, (int)E, MinMax, 1, 2, MV, 0, d_out); }) == "base is not the same size as values" || E == 2,
                   "device form: base_members");
        }
        hipFree(d_cube); hipFree(d_shared); hipFree(d_per); hipFree(d_out);
    }
    if(failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
