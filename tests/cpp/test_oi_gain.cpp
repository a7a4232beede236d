// gridpp::OiGain through its own header (gridpp_amd/host/gridpp_oi_gain.hpp), for a Grid and for a Points background.  The case comes as
// text (argv[1]: Y X S E, then lats, lons [Y*X], station lats, lons, ratios [S], the background stack [Y*X*E], pobs [S], pbackground [S*E],
// every float as the hexadecimal of its bits); the results go to stdout in the same form, for tests/test_gpu_oi_gain_cpp.py to compare
// with the Python binding's.  The Points background is the grid's points in row-major order.  The refusals of the header are checked here.
#include "gridpp_oi_gain.hpp"
#include <cstdio>
#include <cstdlib>
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
static float read_float(FILE* f) {
    unsigned u = 0;
    if(std::fscanf(f, "%x", &u) != 1) { std::printf("FAIL: short input\n"); std::exit(2); }
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}
static vec read_vec(FILE* f, int n) {
    vec v(n);
    for(int i = 0; i < n; i++) v[i] = read_float(f);
    return v;
}
static vec2 read_vec2(FILE* f, int y, int x) {
    vec2 v(y);
    for(int i = 0; i < y; i++) v[i] = read_vec(f, x);
    return v;
}
static void print(const char* name, const vec& a) {
    std::printf("%s %d", name, (int)a.size());
    for(float v : a) { unsigned u; std::memcpy(&u, &v, 4); std::printf(" %08x", u); }
    std::printf("\n");
}
static vec flat(const vec2& a) { vec o; for(const auto& r : a) o.insert(o.end(), r.begin(), r.end()); return o; }
static vec flat(const vec3& a) { vec o; for(const auto& r : a) for(const auto& c : r) o.insert(o.end(), c.begin(), c.end()); return o; }

int main(int argc, char** argv) {
    if(argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if(!f) return 2;
    int Y, X, S, E;
    if(std::fscanf(f, "%d %d %d %d", &Y, &X, &S, &E) != 4) return 2;
    const vec2 lats = read_vec2(f, Y, X), lons = read_vec2(f, Y, X);
    const vec plats = read_vec(f, S), plons = read_vec(f, S), ratios = read_vec(f, S);
    vec3 stack(Y);
    for(int y = 0; y < Y; y++) stack[y] = read_vec2(f, X, E);
    const vec pobs = read_vec(f, S);
    const vec2 pbackground = read_vec2(f, S, E);
    std::fclose(f);
    vec2 first(Y, vec(X));   // field 0 alone
    for(int y = 0; y < Y; y++) for(int x = 0; x < X; x++) first[y][x] = stack[y][x][0];
    vec pbg0(S);
    for(int s = 0; s < S; s++) pbg0[s] = pbackground[s][0];

    const Grid grid(lats, lons);
    const Points points(plats, plons);
    const BarnesStructure structure(12000);
    const OiGain gain(grid, points, ratios, structure, 12);
    print("grid_one", flat(gain.apply(first, pobs, pbg0)));
    print("grid_stack", flat(gain.apply(stack, pobs, pbackground)));
    print("grid_clamped", flat(gain.apply(stack, pobs, pbackground, false)));
    print("grid_variance", flat(gain.analysis_variance(vec2(Y, vec(X, 1.5f)))));
    expect(gain.max_points() == 12 && gain.largest_selection() <= 12 && gain.nbytes() >= (long long)Y * X * 12 * 12, "the accessors of a grid gain");
    const ivec counts = gain.counts();
    const ivec2 indices = gain.indices();
    const std::vector<std::vector<double> > weights = gain.weights();
    bool padded = (int)counts.size() == Y * X && (int)indices.size() == Y * X && (int)weights.size() == Y * X;
    for(size_t i = 0; padded && i < counts.size(); i++)
        for(int k = 0; k < 12; k++) padded = padded && ((k < counts[i]) == (indices[i][k] >= 0)) && (k < counts[i] || weights[i][k] == 0.0);
    expect(padded, "indices are -1 and weights 0 behind the selection");

    // the same points as a Points background
    const Points bpoints(flat(lats), flat(lons));
    vec2 rows((size_t)Y * X);
    for(int y = 0; y < Y; y++) for(int x = 0; x < X; x++) rows[(size_t)y * X + x] = stack[y][x];
    const OiGain pgain(bpoints, points, ratios, structure, 12);
    print("points_one", pgain.apply(flat(first), pobs, pbg0));
    print("points_stack", flat(pgain.apply(rows, pobs, pbackground)));
    print("points_variance", pgain.analysis_variance(vec((size_t)Y * X, 1.5f)));

    // a copy shares the gain; the original may go first
    vec later;
    {
        OiGain* temporary = new OiGain(bpoints, points, ratios, structure, 12);
        const OiGain copy = *temporary;
        delete temporary;
        later = copy.apply(flat(first), pobs, pbg0);
    }
    expect(later == pgain.apply(flat(first), pobs, pbg0), "a copy outlives the gain it was copied from");

    expect(throws<std::invalid_argument>([&] { OiGain(grid, Points(plats, plons, vec(), vec(), Cartesian), ratios, structure, 12); }), "points of another coordinate type are refused");
    expect(throws<std::invalid_argument>([&] { OiGain(grid, points, ratios, structure, 0); }), "max_points 0 is refused");
    expect(throws<std::invalid_argument>([&] { OiGain(grid, points, ratios, structure, OiGain::max_points_cap + 1); }), "max_points beyond the cap is refused");
    expect(throws<std::invalid_argument>([&] { OiGain(grid, points, vec(S - 1, 0.5f), structure, 12); }), "another number of ratios is refused");
    expect(throws<std::invalid_argument>([&] { OiGain(grid, points, ratios, structure, 12, ivec(S - 1, 1)); }), "another number of usable flags is refused");
    expect(throws<std::invalid_argument>([&] { gain.apply(flat(first), pobs, pbg0); }), "a grid gain refuses a flat field");
    expect(throws<std::invalid_argument>([&] { pgain.apply(stack, pobs, pbackground); }), "a points gain refuses a cube");
    expect(throws<std::invalid_argument>([&] { gain.apply(first, vec(S - 1), pbg0); }), "another number of observations is refused");
    vec2 narrow = pbackground;
    for(auto& r : narrow) r.pop_back();
    expect(throws<std::invalid_argument>([&] { gain.apply(stack, pobs, narrow); }), "another number of fields at the points is refused");
    vec bad = pbg0;
    bad[3] = NAN;
    expect(throws<std::invalid_argument>([&] { gain.apply(first, pobs, bad); }), "an invalid value at a usable station is refused");
    ivec usable(S, 1);
    usable[3] = 0;
    expect(!throws<std::invalid_argument>([&] { OiGain(grid, points, ratios, structure, 12, usable).apply(first, pobs, bad); }), "and accepted when the station is not usable");
    if(failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
