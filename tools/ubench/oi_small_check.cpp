// Host check of gridpp_amd/csrc/oi_small.h (tests/test_oi_union_selection_cases_oracle.py builds and runs it):
//   * every entry of the triangle-index table against the integer definition e = i (i + 1) / 2 + p, p <= i, and against the
//     square-root form the P build of k_oi_union used before;
//   * d_min_pos / d_min3_pos against fminf, bit for bit, on float32 operands without NaN and without a sign bit: +0, the smallest and
//     the largest subnormal, the smallest normal, ordinary values, neighbours one ulp apart, FLT_MAX, +inf, and 200 000 random patterns.
// build: g++ -O2 -std=c++17 -I gridpp_amd/csrc tools/ubench/oi_small_check.cpp -o oi_small_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "oi_small.h"

static constexpr TriTab TAB = make_tri_tab();
static_assert(TRI_N == 1953 && TAB.v[0] == 0 && TAB.v[1] == 0x100 && TAB.v[2] == 0x101 && TAB.v[819] == ((39 << 8) | 39) && TAB.v[TRI_N - 1] == ((61 << 8) | 61),
              "the table of the largest union, generated at compile time");

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

int main() {
    long bad_tab = 0, bad_min = 0, nmin = 0;
    int e = 0;
    for(int i = 0; i < TRI_ROWS; ++i)
        for(int p = 0; p <= i; ++p, ++e) {
            if(e != i * (i + 1) / 2 + p || TAB.v[e] != ((i << 8) | p)) bad_tab++;
            int j = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);   // the closed form it replaces
            if(j * (j + 1) / 2 > e) j--;
            if((j + 1) * (j + 2) / 2 <= e) j++;
            if(j != (TAB.v[e] >> 8) || e - j * (j + 1) / 2 != (TAB.v[e] & 255)) bad_tab++;
        }
    if(e != TRI_N) bad_tab++;

    std::vector<float> v = {0.0f, from_bits(1u), from_bits(2u), from_bits(0x007fffffu), from_bits(0x00800000u), from_bits(0x00800001u), 1e-30f, 0.5f,
                            from_bits(0x3f7fffffu), 1.0f, from_bits(0x3f800001u), 3.0f, 1e30f, from_bits(0x7f7fffffu), INFINITY};
    uint64_t s = 0x9e3779b97f4a7c15ull;
    for(int k = 0; k < 200000; ++k) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t u = (uint32_t)(s >> 33);          // 31 bits: no sign
        if((u & 0x7f800000u) == 0x7f800000u && (u & 0x007fffffu)) continue;   // a NaN pattern: outside the precondition
        v.push_back(from_bits(u));
    }
    const size_t n0 = 15;
    for(size_t a = 0; a < v.size(); ++a)
        for(size_t b = 0; b < (a < n0 ? v.size() : n0); ++b) {
            nmin++;
            if(bits(d_min_pos(v[a], v[b])) != bits(fminf(v[a], v[b])) || bits(d_min_pos(v[b], v[a])) != bits(fminf(v[b], v[a]))) bad_min++;
            const float c = v[(a * 7 + b * 13) % v.size()];
            if(bits(d_min3_pos(v[a], v[b], c)) != bits(fminf(fminf(v[a], v[b]), c))) bad_min++;
        }
    printf("table entries %d mismatches %ld; minima %ld mismatches %ld\n", e, bad_tab, nmin, bad_min);
    return bad_tab || bad_min ? 1 : 0;
}
