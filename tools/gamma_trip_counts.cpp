// Trip counts of gridpp_amd/csrc/gamma_fn.h on the seeded inputs of tools/bench_gamma.py: per value the calls of log_tail, the series terms
// plus continued-fraction steps, and the steps of the inverse; and per group of 64 consecutive values (a wave of k_gamma_inv /
// k_gamma_transform) the mean against the maximum, which is what the wave pays.  Host only, any C++17 compiler with the HIP headers on its include path:
//
//     g++ -O2 -std=c++17 -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include tools/gamma_trip_counts.cpp -o gamma_trip_counts
//     ./gamma_trip_counts inputs.bin      # written by tools/bench_gamma.py --dump-inputs inputs.bin
//
// inputs.bin: records of (int32 kind, int32 n, float32 p0, p1, p2, then the arrays): kind 0 = gamma_inv (levels, shape, scale follow),
// 1 = forward, 2 = backward (Gamma(p0, p1, p2), the values follow).
#include "../gridpp_amd/csrc/gamma_fn.h"
#include <algorithm>
#include <cstdio>
#include <vector>

namespace gm = gpp::gamma_fn;

int main(int argc, char** argv) {
    if(argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if(!f) return 2;
    int head[2];
    float p[3];
    while(std::fread(head, 4, 2, f) == 2 && std::fread(p, 4, 3, f) == 3) {
        const int kind = head[0], n = head[1];
        std::vector<float> a(n), b, c;
        if(std::fread(a.data(), 4, n, f) != (size_t)n) return 2;
        if(kind == 0) {
            b.resize(n), c.resize(n);
            if(std::fread(b.data(), 4, n, f) != (size_t)n || std::fread(c.data(), 4, n, f) != (size_t)n) return 2;
        }
        const gm::GammaParams g{p[0], p[1], p[2], std::lgamma((double)p[0])};
        double evals = 0, terms = 0, steps = 0, wave_max = 0;
        int most_terms = 0, most_steps = 0, most_series = 0, most_fraction = 0, wave_top = 0;
        for(int i = 0; i < n; i++) {
            gm::Work w;
            int code;
            if(kind == 0) gm::gamma_inv(a[i], b[i], c[i], &code, &w);
            else if(kind == 1) gm::transform_forward(a[i], g, &w);
            else gm::transform_backward(a[i], g, &w);
            evals += w.evaluations, terms += w.terms, steps += w.steps;
            most_terms = std::max(most_terms, w.terms), most_steps = std::max(most_steps, w.steps);
            most_series = std::max(most_series, w.most_series), most_fraction = std::max(most_fraction, w.most_fraction);
            wave_top = std::max(wave_top, w.terms);
            if(i % 64 == 63 || i == n - 1) { wave_max += wave_top; wave_top = 0; }
        }
        const double waves = (n + 63) / 64;
        std::printf("%s n=%d: per value %.2f log_tail calls, %.1f series terms + fraction steps, %.2f inverse steps; most %d terms, %d inverse steps, "
                    "longest series %d, longest fraction %d; per wave of 64 the slowest lane runs %.1f terms, the mean lane %.1f (%.2f x)\n",
                    kind == 0 ? "gamma_inv" : kind == 1 ? "forward" : "backward", n, evals / n, terms / n, steps / n, most_terms, most_steps, most_series, most_fraction,
                    wave_max / waves, terms / n, (wave_max / waves) / std::max(terms / n, 1e-9));
    }
    std::fclose(f);
    return 0;
}
