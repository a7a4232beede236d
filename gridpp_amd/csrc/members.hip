// Per-member window operations on (Y, X, E) cubes, no counterpart in the reference:
//   neighbourhood_members   plane e of the result = neighbourhood(input[..., e], halfwidth, statistic)
//   calc_gradient_members   plane e of the result = calc_gradient(base_e, values[..., e], ...)
//
// A cube is an image of Y rows by N = X * E floats whose horizontal window taps lie E apart.  The box statistics (Mean, Sum, Count, and through them
// Std and Variance) have two forms with the same sums; the five moments of the LinearRegression gradient take the second one:
//   fused    (halfwidth * E <= MEM_F_MAXH) k_mem_fused: a workgroup marches down a strip of MEM_F_T flattened columns, halo of halfwidth * E per side
//            included.  Every thread slides the column windows of MEM_F_NC columns down the rows in registers, the column sums of a row go through
//            LDS once, and the row window is 2 halfwidth + 1 taps E apart out of LDS.  No intermediate in HBM.
//   two-pass (every halfwidth, E and shape; GPP_MEMBERS_TWO_PASS forces it) over a band of rows: k_mem_cols slides the window down every flattened
// column j = x * E + e (vertical neighbours are one row pitch away: no halo, lanes along j coalesced whatever E is) and leaves the column sums (double) and the numbers of valid values (int) of the band in HBM; k_mem_rows
// slides along x through those, E apart, one thread per (row, segment of MEM_SEG cells, member) with the members on adjacent lanes, and finishes.
// Min / Max take the same two passes with direct window loops (exact selections).  The band keeps the intermediates small enough for the
// staging pool (and for the last-level cache) at every cube size; every index is a long and every launch a 1-D grid bounded by the band.
// Std / Variance and the LinearRegression gradient end in the kernels of the 2-D calls themselves (k_std_finish, k_gradient_regression,
// launched from their own translation units), so that their float expressions are the same instructions in both calls.
#include "common.h"
#include <algorithm>

#pragma clang fp contract(off)
using namespace gpp;

namespace gpp {
void std_finish_launch(const float* mean, const float* mean2, long n, int is_std, float* out);                       // neighbourhood.hip: k_std_finish
void gradient_regression_launch(const float* mX, const float* mY, const float* mXX, const float* mXY, const float* cnt, size_t n, int num_min,
                                float min_range, float default_gradient, float* out);                                 // gridops.hip: k_gradient_regression
}

namespace {

#define MEM_CS 32    // rows of a band that one thread of k_mem_cols slides down
#define MEM_SEG 32   // cells along x that one thread of k_mem_rows slides along
#define MEM_BAND_BYTES (192L << 20)   // intermediates of a band of the two-pass form in HBM: column sums (double), counts (int), the float planes of Std / Variance / the gradient
#define MEM_PLANE_BYTES (1L << 30)    // the float planes of a band of the fused form: its launches need some 1000 workgroups of 16 rows by up to 3072 columns to fill the chip
#define MEM_F_NC 12                   // fused form: columns per thread ...
#define MEM_F_T (256 * MEM_F_NC)      // ... of a strip of 3072 columns, halo included: 2 x 3072 x (8 + 2) B = 60 KiB of LDS, two workgroups per CU
#define MEM_F_MAXH 1024               // the halo halfwidth * E the fused form takes: at least MEM_F_T - 2 * 1024 = 1024 output columns per strip

// What a pass sums: the values themselves, their float squares (Std / Variance), or one of the five moment fields of calc_gradient.cpp:79-98
// formed on the fly from base and values (an invalid base or value makes all five invalid; the mask is 1 / 0).
enum { SRC_VALUE = 0, SRC_SQUARE, SRC_B, SRC_V, SRC_BB, SRC_BV, SRC_OK };
struct Source {
    const float* values;   // [Y][X][E]
    const float* base;     // [Y][X] (base_e == 0) or [Y][X][E]; moments only
    int X, E, base_e;
};
// element (row, flattened column j) of the source; x = j / E (a thread works it out once per column)
template <int SRC>
__device__ __forceinline__ float source_at(const Source& s, long row, long j, int x) {
    const long i = row * ((long)s.X * s.E) + j;
    const float v = s.values[i];
    if(SRC == SRC_VALUE) return v;
    if(SRC == SRC_SQUARE) return v * v;
    const float b = s.base[s.base_e ? i : row * s.X + x];
    const bool good = dev_valid(b) && dev_valid(v);
    if(SRC == SRC_OK) return good ? 1.0f : 0.0f;
    if(!good) return NAN;
    return SRC == SRC_B ? b : SRC == SRC_V ? v : SRC == SRC_BB ? b * b : b * v;
}

// Column pass: the band rows [ya, yb) of a [Y][N] image.  One thread per (strip of MEM_CS rows, flattened column); cs / cc are [yb - ya][N].
template <int SRC>
__global__ __launch_bounds__(256) void k_mem_cols(Source src, int Y, long N, int hw, int ya, int yb, double* __restrict__ cs, int* __restrict__ cc) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long nstrip = (yb - ya + MEM_CS - 1) / MEM_CS;
    if(t >= nstrip * N) return;
    const long strip = t / N, j = t - strip * N;
    const int y0 = ya + (int)strip * MEM_CS, y1 = min(yb, y0 + MEM_CS);
    const long lo = max(0L, (long)y0 - hw), hi = min((long)Y - 1, (long)y0 + hw);
    const int x = (int)(j / src.E);
    double s = 0; int c = 0;
    for(long yy = lo; yy <= hi; yy++) { const float v = source_at<SRC>(src, yy, j, x); if(dev_valid(v)) { s += (double)v; c++; } }
    for(int y = y0; y < y1; y++) {
        if(y > y0) {
            const long add = (long)y + hw, sub = (long)y - hw - 1;
            if(add <= (long)Y - 1) { const float v = source_at<SRC>(src, add, j, x); if(dev_valid(v)) { s += (double)v; c++; } }
            if(sub >= 0) { const float v = source_at<SRC>(src, sub, j, x); if(dev_valid(v)) { s -= (double)v; c--; } }
        }
        const long o = (long)(y - ya) * N + j;
        cs[o] = s; cc[o] = c;
    }
}
// Row pass + finish: one thread per (band row, segment of MEM_SEG cells, member), members fastest; out is the band's [rows][X][E].
// Mean is the double sum over the count rounded once to float (neighbourhood.cpp:132-142).
__global__ __launch_bounds__(256) void k_mem_rows(const double* __restrict__ cs, const int* __restrict__ cc, long rows, int X, int E, int hw, int statistic,
                                                  float* __restrict__ out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long nseg = ((long)X + MEM_SEG - 1) / MEM_SEG, per_row = nseg * E;
    if(t >= rows * per_row) return;
    const long r = t / per_row, q = t - r * per_row;
    const long g = q / E; const int e = (int)(q - g * E);
    const long row = r * (long)X * E + e;
    const int x0 = (int)(g * MEM_SEG), x1 = min(X, x0 + MEM_SEG);
    const long lo = max(0L, (long)x0 - hw), hi = min((long)X - 1, (long)x0 + hw);
    double s = 0; int c = 0;
    for(long k = lo; k <= hi; k++) { s += cs[row + k * E]; c += cc[row + k * E]; }
    for(int x = x0; x < x1; x++) {
        if(x > x0) {
            const long add = (long)x + hw, sub = (long)x - hw - 1;
            if(add <= (long)X - 1) { s += cs[row + add * E]; c += cc[row + add * E]; }
            if(sub >= 0) { s -= cs[row + sub * E]; c -= cc[row + sub * E]; }
        }
        float o = NAN;
        if(statistic == GPP_COUNT) o = (float)c;
        else if(c > 0) o = (statistic == GPP_MEAN) ? (float)(s / (double)c) : (float)s;
        out[row + (long)x * E] = o;
    }
}
// Fused form.  Workgroup b: strip b % nstrip of W = MEM_F_T - 2 H output columns (H = hw * E), rows [y0, y1) = segment b / nstrip of SH rows of the band [ya, yb).
// Thread t owns the columns j0 - H + t + 256 i: their window sums over the rows slide down in registers (a column or row outside the image adds nothing, so the
// taps need no bounds), go to LDS (two buffers: one barrier per row), and output column oc sums the LDS entries oc, oc + E, ..., oc + 2 H.  The values of the
// next row are asked for before the taps of this one.  out is the band's [yb - ya][N].
template <int SRC>
__global__ __launch_bounds__(256) void k_mem_fused(Source src, int Y, long N, int hw, int statistic, int ya, int yb, int SH, float* __restrict__ out) {
    __shared__ double ls[2][MEM_F_T];
    __shared__ unsigned short lc[2][MEM_F_T];   // (a count is at most 2 hw + 1 <= 2 MEM_F_MAXH + 1)
    const int E = src.E, H = hw * E, W = MEM_F_T - 2 * H, tid = threadIdx.x;
    const long nstrip = (N + W - 1) / W, strip = blockIdx.x % nstrip;
    const int seg = (int)(blockIdx.x / nstrip);
    const int y0 = ya + seg * SH, y1 = min(yb, y0 + SH);
    const long j0 = strip * W, jl = j0 - H + tid;
    double s[MEM_F_NC]; int c[MEM_F_NC], xc[MEM_F_NC]; float va[MEM_F_NC], vs[MEM_F_NC];
#pragma unroll
    for(int i = 0; i < MEM_F_NC; i++) { s[i] = 0; c[i] = 0; const long j = jl + 256 * i; xc[i] = (j >= 0 && j < N) ? (int)(j / E) : -1; }   // -1: outside the image
    auto ld = [&](long row, int i) -> float { return (row >= 0 && row < Y && xc[i] >= 0) ? source_at<SRC>(src, row, jl + 256 * i, xc[i]) : NAN; };
    const long lo = max(0L, (long)y0 - hw), hi = min((long)Y - 1, (long)y0 + hw);
    for(long yy = lo; yy <= hi; yy++) {
#pragma unroll
        for(int i = 0; i < MEM_F_NC; i++) { const float v = ld(yy, i); if(dev_valid(v)) { s[i] += (double)v; c[i]++; } }
    }
#pragma unroll
    for(int i = 0; i < MEM_F_NC; i++) { va[i] = ld((long)y0 + 1 + hw, i); vs[i] = ld((long)y0 - hw, i); }   // row y0 + 1 enters / leaves
    for(int y = y0; y < y1; y++) {
        const int b = (y - y0) & 1;
#pragma unroll
        for(int i = 0; i < MEM_F_NC; i++) { ls[b][tid + 256 * i] = s[i]; lc[b][tid + 256 * i] = (unsigned short)c[i]; }
        lds_barrier();   // (__syncthreads would also wait for the global loads of the next row, which are meant to stay in flight)
        if(y + 1 < y1) {
#pragma unroll
            for(int i = 0; i < MEM_F_NC; i++) {
                if(dev_valid(va[i])) { s[i] += (double)va[i]; c[i]++; }
                if(dev_valid(vs[i])) { s[i] -= (double)vs[i]; c[i]--; }
            }
            if(y + 2 < y1) {
#pragma unroll
                for(int i = 0; i < MEM_F_NC; i++) { va[i] = ld((long)y + 2 + hw, i); vs[i] = ld((long)y + 1 - hw, i); }
            }
        }
#pragma unroll
        for(int i = 0; i < MEM_F_NC; i++) {
            const int oc = tid + 256 * i;
            const long j = j0 + oc;
            if(oc < W && j < N) {
                double sum = 0; int cnt = 0;
                for(int k = 0; k <= 2 * hw; k++) { sum += ls[b][oc + k * E]; cnt += lc[b][oc + k * E]; }
                float o = NAN;
                if(statistic == GPP_COUNT) o = (float)cnt;
                else if(cnt > 0) o = (statistic == GPP_MEAN) ? (float)(sum / (double)cnt) : (float)sum;
                out[(long)(y - ya) * N + j] = o;
            }
        }
    }
}
// Min / Max: the column window of the band rows [ya, yb) into tmp [yb - ya][N], then the row window out of it.  Selections over valid
// values; NaN where there is none (an intermediate is a valid value or NaN).
__global__ __launch_bounds__(256) void k_mem_minmax_cols(const float* __restrict__ in, int Y, long N, int hw, int is_max, int ya, int yb, float* __restrict__ tmp) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if(t >= (long)(yb - ya) * N) return;
    const long r = t / N, j = t - r * N;
    const long y = ya + r, lo = max(0L, y - hw), hi = min((long)Y - 1, y + hw);
    float m = NAN;
    for(long k = lo; k <= hi; k++) { const float v = in[k * N + j]; if(dev_valid(v) && (!dev_valid(m) || (is_max ? v > m : v < m))) m = v; }
    tmp[t] = m;
}
__global__ __launch_bounds__(256) void k_mem_minmax_rows(const float* __restrict__ tmp, long rows, int X, int E, int hw, int is_max, float* __restrict__ out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long N = (long)X * E;
    if(t >= rows * N) return;
    const long r = t / N, j = t - r * N;
    const long x = j / E; const int e = (int)(j - x * E);
    const long lo = max(0L, x - hw), hi = min((long)X - 1, x + hw);
    const float* row = tmp + r * N + e;
    float m = NAN;
    for(long k = lo; k <= hi; k++) { const float v = row[k * E]; if(dev_valid(v) && (!dev_valid(m) || (is_max ? v > m : v < m))) m = v; }
    out[t] = m;
}
// calc_gradient.cpp:26-74 (MinMax) for one (cell, member): the reference's walk in row-major order, strict > / <, validity of base and value
// together.  Members on adjacent lanes: a shared base is a broadcast load, the values a coalesced one.
__global__ __launch_bounds__(256) void k_mem_gradient_minmax(const float* __restrict__ base, int base_e, const float* __restrict__ values, int nY, int nX, int E,
                                                             int halfwidth, int num_min, float min_range, float default_gradient, float* __restrict__ out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if(t >= (long)nY * nX * E) return;
    const long c = t / E; const int e = (int)(t - c * E);
    const long y = c / nX, x = c - y * nX;
    float cmax = NAN, cmin = NAN;
    long imax = 0, imin = 0;
    int count = 0;
    const long ylo = max(0L, y - halfwidth), yhi = min((long)nY - 1, y + halfwidth), xlo = max(0L, x - halfwidth), xhi = min((long)nX - 1, x + halfwidth);
    for(long yy = ylo; yy <= yhi; ++yy)
        for(long xx = xlo; xx <= xhi; ++xx) {
            const long n = yy * nX + xx;
            const float b = base[base_e ? n * E + e : n];
            if(!dev_valid(b) || !dev_valid(values[n * E + e])) continue;
            if(!dev_valid(cmax) || b > cmax) { cmax = b; imax = n; }
            if(!dev_valid(cmin) || b < cmin) { cmin = b; imin = n; }
            count++;
        }
    float r = default_gradient;
    if(!(count < num_min || !dev_valid(cmax) || !dev_valid(cmin) || fabsf(cmax - cmin) <= min_range)) r = (values[imax * E + e] - values[imin * E + e]) / (cmax - cmin);
    out[t] = r;
}


// The fused form takes this call (the halo fits its strip); GPP_MEMBERS_TWO_PASS forces the two-pass form (tests, A/B timings)
bool fused_form(int hw, int E) { return (long)hw * E <= MEM_F_MAXH && !path_env("GPP_MEMBERS_TWO_PASS"); }
// Rows per band: the intermediates of a band (`bytes` per element) stay within MEM_BAND_BYTES (whole strips of MEM_CS rows where more than one fits; at
// least one row); a call without intermediates takes the cube in one band.  GPP_MEMBERS_BAND_ROWS sets it (tests: several bands on a small cube; A/B timings).
int band_rows(int Y, long N, int bytes, long budget = MEM_BAND_BYTES) {
    long rows = bytes ? std::max(1L, budget / bytes / std::max(1L, N)) : Y;
    if(bytes && rows > MEM_CS) rows -= rows % MEM_CS;
    if(const char* v = path_env("GPP_MEMBERS_BAND_ROWS")) rows = std::max(1, atoi(v));
    return (int)std::min<long>(rows, Y);
}

typedef void (*ColsKernel)(Source, int, long, int, int, int, double*, int*);
ColsKernel cols_kernel(int src) {
    static const ColsKernel forms[] = {k_mem_cols<SRC_VALUE>, k_mem_cols<SRC_SQUARE>, k_mem_cols<SRC_B>, k_mem_cols<SRC_V>, k_mem_cols<SRC_BB>, k_mem_cols<SRC_BV>,
                                       k_mem_cols<SRC_OK>};
    return forms[src];
}
typedef void (*FusedKernel)(Source, int, long, int, int, int, int, int, float*);
FusedKernel fused_kernel(int src) {
    static const FusedKernel forms[] = {k_mem_fused<SRC_VALUE>, k_mem_fused<SRC_SQUARE>};   // (the gradient's moments lost in this form: DESIGN.md 4.21)
    return forms[src];
}

// The workspaces of one call: borrowed from the staging pool (gpp_release_workspaces() empties it), nothing is kept between calls.
struct MemBuffers {
    Staged<double> cs; Staged<int> cc; Staged<float> f;
};
// Mean / Sum / Count of source `src` over the band rows [ya, yb): d_out is the band's [yb - ya][X][E]
void box_band(MemBuffers& w, const Source& s, int src, bool fused, int Y, int X, int hw, int statistic, int ya, int yb, float* d_out) {
    const long N = (long)X * s.E, rows = yb - ya, nstrip = (rows + MEM_CS - 1) / MEM_CS;
    if(fused) {
        const long W = MEM_F_T - 2L * hw * s.E, strips = (N + W - 1) / W;
        int SH = 64;   // rows a workgroup marches down: shorter where the launch would not fill the chip (its first window costs 2 hw + 1 rows)
        while(SH > 16 && strips * ((rows + SH - 1) / SH) < 1024) SH >>= 1;
        if(const char* v = path_env("GPP_MEMBERS_SEG_ROWS")) SH = std::max(1, atoi(v));   // (tests: the long segments of a large cube on a small one; A/B timings)
        launch(fused_kernel(src), (unsigned)(strips * ((rows + SH - 1) / SH)), 256, 0, s, Y, N, hw, statistic, ya, yb, SH, d_out);
        return;
    }
    launch(cols_kernel(src), blocks_of(nstrip * N), 256, 0, s, Y, N, hw, ya, yb, w.cs.p, w.cc.p);
    const long nseg = ((long)X + MEM_SEG - 1) / MEM_SEG;
    launch(k_mem_rows, blocks_of(rows * nseg * s.E), 256, 0, (const double*)w.cs.p, (const int*)w.cc.p, rows, X, s.E, hw, statistic, d_out);
}

void members_neighbourhood(const float* d_in, int Y, int X, int E, int hw, int statistic, float* d_out) {
    const long N = (long)X * E;
    const bool minmax = statistic == GPP_MIN || statistic == GPP_MAX, moments = statistic == GPP_STD || statistic == GPP_VARIANCE;
    const bool fused = !minmax && fused_form(hw, E), two_pass = !minmax && !fused;
    const int B = band_rows(Y, N, minmax ? 4 : (two_pass ? 12 : 0) + (moments ? 8 : 0), minmax || two_pass ? MEM_BAND_BYTES : MEM_PLANE_BYTES);
    const size_t bn = (size_t)B * N;
    MemBuffers w;
    const Source s{d_in, nullptr, X, E, 0};
    if(minmax) w.f.get(bn);
    if(two_pass) { w.cs.get(bn); w.cc.get(bn); }
    if(moments) w.f.get(2 * bn);
    for(int ya = 0; ya < Y; ya += B) {
        const int yb = std::min(Y, ya + B);
        const long n = (long)(yb - ya) * N;
        float* o = d_out + (long)ya * N;
        if(minmax) {
            launch(k_mem_minmax_cols, blocks_of(n), 256, 0, d_in, Y, N, hw, statistic == GPP_MAX, ya, yb, w.f.p);
            launch(k_mem_minmax_rows, blocks_of(n), 256, 0, (const float*)w.f.p, (long)(yb - ya), X, E, hw, statistic == GPP_MAX, o);
        }
        else if(moments) {   // neighbourhood.cpp:205-233: the float means of the values and of their float squares, then k_std_finish
            float *mean = w.f.p, *mean2 = w.f.p + bn;
            box_band(w, s, SRC_VALUE, fused, Y, X, hw, GPP_MEAN, ya, yb, mean);
            box_band(w, s, SRC_SQUARE, fused, Y, X, hw, GPP_MEAN, ya, yb, mean2);
            std_finish_launch(mean, mean2, n, statistic == GPP_STD, o);
        }
        else box_band(w, s, SRC_VALUE, fused, Y, X, hw, statistic, ya, yb, o);
    }
}

void members_gradient(const float* d_base, int base_e, const float* d_values, int Y, int X, int E, int type, int hw, int num_min, float min_range,
                      float default_gradient, float* d_out) {
    const long N = (long)X * E;
    if(type == GPP_GRADIENT_MINMAX) {
        launch(k_mem_gradient_minmax, blocks_of((long)Y * N), 256, 0, d_base, base_e, d_values, Y, X, E, hw, num_min, min_range, default_gradient, d_out);
        return;
    }
    // calc_gradient.cpp:79-124: box means of the four moment fields, the box sum of the mask, k_gradient_regression
    const int B = band_rows(Y, N, 12 + 20);   // (the two-pass form at every halfwidth)
    const size_t bn = (size_t)B * N;
    MemBuffers w;
    w.cs.get(bn); w.cc.get(bn); w.f.get(5 * bn);
    const Source s{d_values, d_base, X, E, base_e};
    for(int ya = 0; ya < Y; ya += B) {
        const int yb = std::min(Y, ya + B);
        const long n = (long)(yb - ya) * N;
        float* m[5];
        for(int k = 0; k < 5; k++) {
            m[k] = w.f.p + k * bn;
            box_band(w, s, SRC_B + k, false, Y, X, hw, k == 4 ? GPP_SUM : GPP_MEAN, ya, yb, m[k]);
        }
        gradient_regression_launch(m[0], m[1], m[2], m[3], m[4], (size_t)n, num_min, min_range, default_gradient, d_out + (long)ya * N);
    }
}

}   // namespace

extern "C" int gpp_neighbourhood_members(const float* input, int ny, int nx, int ne, int halfwidth, int statistic, float* out, int mem) {
    GPP_TRY
    if(halfwidth < 0) invalid("Half width must be > 0");
    if(statistic == GPP_QUANTILE) invalid("Use neighbourhood_quantile for computing neighbourhood quantiles");
    if(statistic == GPP_MEDIAN) invalid("neighbourhood_members does not compute the statistic Median: order statistics per member are not supported");
    if(statistic == GPP_RANDOMCHOICE) invalid("neighbourhood_members does not compute the statistic RandomChoice: order statistics per member are not supported");
    switch(statistic) {
        case GPP_MEAN: case GPP_MIN: case GPP_MAX: case GPP_STD: case GPP_VARIANCE: case GPP_SUM: case GPP_COUNT: break;
        default: invalid("neighbourhood_members: unknown statistic");
    }
    if(ny < 0 || nx < 0 || ne < 0) invalid("negative size");
    if(ny == 0 || nx == 0 || ne == 0) return GPP_OK;
    if(!input || !out) invalid("input / out is NULL");
    ensure_device();
    const size_t n = (size_t)ny * nx * ne;
    InField in; OutField o;
    in.bind(input, n, mem);
    o.bind(out, n, mem);
    members_neighbourhood(in.d, ny, nx, ne, halfwidth, statistic, o.d);
    return finish_call(o);
    GPP_CATCH
}

extern "C" int gpp_calc_gradient_members(const float* base, int base_members, const float* values, int ny, int nx, int ne, int gradient_type, int halfwidth,
                                         int num_min, float min_range, float default_gradient, float* out, int mem) {
    GPP_TRY
    if(halfwidth <= 0) invalid("Halwidth cannot be <= 0; must be positive integer");   // calc_gradient.cpp:10-17
    if(is_valid(min_range) && min_range < 0) invalid("min_range must be >= 0");
    if(num_min < 0) invalid("num_min must be >= 0");
    if(ny <= 0) invalid("base input has no size");
    if(nx < 0 || ne < 0) invalid("negative size");
    if(base_members != 1 && base_members != ne) invalid("base is not the same size as values");
    if(gradient_type != GPP_GRADIENT_MINMAX && gradient_type != GPP_GRADIENT_LINEAR_REGRESSION) invalid("unknown gradient type");
    const size_t n = (size_t)ny * nx * ne;
    if(n == 0) return GPP_OK;
    if(!base || !values || !out) invalid("base / values / out is NULL");
    ensure_device();
    InField b, v; OutField o;
    b.bind(base, (size_t)ny * nx * base_members, mem);
    v.bind(values, n, mem);
    o.bind(out, n, mem);
    members_gradient(b.d, base_members == ne ? 1 : 0, v.d, ny, nx, ne, gradient_type, halfwidth, num_min, min_range, default_gradient, o.d);
    return finish_call(o);
    GPP_CATCH
}
