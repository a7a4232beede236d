// gridpp::calc_score and gridpp::neighbourhood_score (src/api/metric_optimizer.cpp:185-244, src/api/neighbourhood_score.cpp:6-60) for gfx950.
//
// neighbourhood_score in the reference: gridding_nearest of the observations, four float planes a / b / c / d of zeros and ones, four
// neighbourhood(..., Mean) calls (a double summed-area table each) and calc_score per cell.  The planes hold only 0 and 1 and a cell is in
// at most one of them, so the four box sums are exact small integers whatever the order of the additions: here a cell is ONE byte (0: not
// counted, 1..4: a..d) and one pass forms all four sums.  mean = (float)((double)n / area) with `area` the cells of the clipped window is
// what neighbourhood.cpp:132-141 computes (the planes have no missing values, so its count is the area), hence the same bits.
//
//   k_score_classify    one thread per cell: the gridded reference (gpp_gridding_nearest_device, radius.hip) and fcst -> the byte.
//   k_score_march       half widths up to GPP_SCORE_FUSED_MAXHW, row pass and column pass in one kernel in the shape of k_box_march
//                       (neighbourhood.hip).  A workgroup marches down a strip of SC_W output columns in chunks of SC_C rows.  The
//                       (SC_W + 2 hw) bytes of every new row go through LDS once (the next chunk's are asked for before the sums of this one
//                       are formed); their row-window counts, four 16-bit lanes in one 64-bit word, go into a ring of SC_RING rows; the
//                       outputs whose 2 hw + 1 rows are in the ring are column sums of ring words, again packed.  The finish step unpacks,
//                       forms the area in closed form and evaluates the score (score.h).  No plane of a, b, c or d exists anywhere.
//                       LDS: the chunk's rows have a pitch of 25 words and the ring's rows one of 65 double words, and in the row pass
//                       the 32 lanes of a half wavefront hold 32 rows of one eight-column segment: their byte reads fall into 32
//                       different banks and the 8-byte ring writes of 16 lanes cover all 32 once.  The column pass reads the ring along
//                       a row: consecutive words.  36 480 bytes per workgroup, four workgroups per CU.  GPP_SCORE_FILL (a path override)
//                       replaces the 1024 workgroups the launch aims for: with 1 a workgroup marches down all rows of its strip, as it
//                       does on fields of millions of cells, and the tests reach the wrapping ring on small grids.
//   k_score_rows /      the general path, any half width (the host clamps it to the longer side of the field, which changes no window):
//   k_score_cols        a separable pair with 32-bit counters, four per cell in a workspace plane, sliding along runs of SC_RUN cells;
//                       the column kernel ends in the same finish step.  GPP_SCORE_GENERAL (a path override) forces it.
//   k_score_counts      the vector calc_score: four 64-bit counters in one pass, per-wave shuffles, then one atomic per counter and
//                       workgroup on ordinary global memory.
//
// Packing bound: a lane of a ring word holds at most 2 hw + 1 and a lane of a column sum at most (2 hw + 1)^2, which must stay below
// 65536: hw <= 127.  GPP_SCORE_FUSED_MAXHW = 16 is set by the ring (SC_C + 2 hw <= SC_RING), far inside that bound; a window of 65535 or
// more counted cells can therefore only occur on the general path, whose counters are 32 bits wide (a field has fewer than 2^31 cells).
#include "common.h"
#include "march_geom.h"
#include "score.h"
#include <algorithm>
#include <cstdint>

#pragma clang fp contract(off)

using namespace gpp;

static_assert(GPP_METRIC_ETS == GPP_SCORE_ETS && GPP_METRIC_TS == GPP_SCORE_TS && GPP_METRIC_KSS == GPP_SCORE_KSS && GPP_METRIC_PC == GPP_SCORE_PC &&
              GPP_METRIC_BIAS == GPP_SCORE_BIAS && GPP_METRIC_HSS == GPP_SCORE_HSS, "score.h and gridpp_hip.h name the same metrics");

namespace {

constexpr int SC_W = GPP_SCORE_TILE_COLS;                         // output columns of a strip
constexpr int SC_C = GPP_SCORE_TILE_ROWS;                         // rows of a chunk
constexpr int SC_RING = 64;                         // rows of row-window counts kept
constexpr int SC_MAXHW = GPP_SCORE_FUSED_MAXHW;
constexpr int SC_WT = SC_W + 2 * SC_MAXHW;          // bytes of a chunk row: the strip and both halos
constexpr int SC_P = SC_WT + 4;                     // their pitch in LDS: 25 words, so the 32 rows that a half wavefront reads lie in 32 banks
constexpr int SC_RP = SC_W + 1;                     // pitch of a ring row in 8-byte words: 16 rows written together lie in 32 different banks
constexpr int SC_THREADS = 256;
constexpr int SC_PRE = SC_C * SC_WT / SC_THREADS;   // bytes of a chunk that one thread moves
constexpr int SC_RUN = 32;                          // outputs per thread of the general path's sliding sums
static_assert(SC_C + 2 * SC_MAXHW <= SC_RING && (SC_RING & (SC_RING - 1)) == 0, "the ring holds every row that a pending output needs");
static_assert((2 * SC_MAXHW + 1) * (2 * SC_MAXHW + 1) < 65536, "16-bit lanes hold the counts of a window");
static_assert(SC_C * SC_WT % SC_THREADS == 0 && SC_THREADS == 8 * SC_C && SC_THREADS == 4 * SC_W && SC_W == 64 && SC_C == 32, "thread layout");
static_assert((SC_P / 4) % 2 == 1 && SC_P % 4 == 0 && SC_RP % 2 == 1, "odd pitches");

__global__ __launch_bounds__(256) void k_score_classify(const float* __restrict__ ref_grid, const float* __restrict__ fcst, size_t n, float threshold,
                                                        unsigned char* __restrict__ cat) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) return;
    const float r = ref_grid[i], f = fcst[i];
    unsigned char k = 0;
    if(dev_valid(r) && dev_valid(f))                                           // neighbourhood_score.cpp:31-41
        k = f > threshold ? (r > threshold ? 1 : 2) : (r > threshold ? 3 : 4);
    cat[i] = k;
}

// one count in the 16-bit lane of the category (nothing for 0)
__device__ __forceinline__ unsigned long long lane_of(unsigned k) { return k ? 1ull << (16 * (k - 1)) : 0ull; }

// the score of the cell (y, x) from the numbers of a / b / c / d cells in its clipped window
__device__ __forceinline__ float finish(unsigned na, unsigned nb, unsigned nc, unsigned nd, int y, int x, int Y, int X, int hw, int metric) {
    const int area = (min(y + hw, Y - 1) - max(y - hw, 0) + 1) * (min(x + hw, X - 1) - max(x - hw, 0) + 1);
    const double A = (double)area;
    const float a = (float)((double)na / A), b = (float)((double)nb / A), c = (float)((double)nc / A), d = (float)((double)nd / A);
    return gpp_score_value(a, b, c, d, metric);
}

// blockIdx.x: the strip, blockIdx.y: the segment of SH rows (a multiple of SC_C).  1 <= hw <= SC_MAXHW.
__global__ __launch_bounds__(SC_THREADS) void k_score_march(const unsigned char* __restrict__ cat, int Y, int X, int hw, int metric, int SH,
                                                            float* __restrict__ out) {
    __shared__ unsigned char tin[SC_C * SC_P];              // the rows of the chunk, column x0 - hw first; 0 outside the field
    __shared__ unsigned long long ring[SC_RING * SC_RP];    // packed row-window counts of the strip's columns; slot of row y: (y - yl0) % SC_RING
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SC_W;
    const int ya = blockIdx.y * SH, yb = min(Y, ya + SH);
    const int yl0 = ya - hw;                                // first row the segment loads
    const int nchunk = (yb - 1 + hw - yl0) / SC_C + 1;
    const int Wt = SC_W + 2 * hw;
    unsigned char pre[SC_PRE];
    auto fetch = [&](const int k) {
#pragma unroll
        for(int j = 0; j < SC_PRE; j++) {
            const int i = tid + SC_THREADS * j, r = i / SC_WT, t = i - r * SC_WT;
            const int y = yl0 + k * SC_C + r, x = x0 - hw + t;
            pre[j] = (t < Wt && y >= 0 && y < Y && x >= 0 && x < X) ? cat[(size_t)y * X + x] : (unsigned char)0;
        }
    };
    fetch(0);
    int ynext = ya;
    for(int k = 0; k < nchunk; k++) {
#pragma unroll
        for(int j = 0; j < SC_PRE; j++) {
            const int i = tid + SC_THREADS * j, r = i / SC_WT;
            tin[r * SC_P + (i - r * SC_WT)] = pre[j];
        }
        __syncthreads();   // the chunk is in LDS; every thread has left the column pass of the chunk before
        if(k + 1 < nchunk) fetch(k + 1);
        {   // row pass: thread (r, sg) slides along the eight columns of segment sg of row r; the lanes of a half wavefront hold 32 rows of one segment
            const int r = tid & (SC_C - 1), sg = tid / SC_C;
            const unsigned char* const row = tin + r * SC_P + 8 * sg;   // the window of column 8 sg + j is row[j .. j + 2 hw]
            unsigned long long* const rs = ring + ((k * SC_C + r) & (SC_RING - 1)) * SC_RP + 8 * sg;
            unsigned long long s = 0;
            for(int q = 0; q <= 2 * hw; q++) s += lane_of(row[q]);
            rs[0] = s;
#pragma unroll
            for(int j = 1; j < 8; j++) {
                s += lane_of(row[j + 2 * hw]) - lane_of(row[j - 1]);
                rs[j] = s;
            }
        }
        __syncthreads();   // the ring holds the rows up to ytop
        const int ytop = yl0 + (k + 1) * SC_C - 1;
        const int ylim = max(ynext, min(yb, ytop - hw + 1));   // outputs [ynext, ylim) have their 2 hw + 1 rows in the ring: at most SC_C of them
        {   // column pass: thread (c, g) slides down eight rows of column c
            const int c = tid & (SC_W - 1), x = x0 + c;
            const int y8 = ynext + 8 * (tid / SC_W);
            if(y8 < ylim && x < X) {
                const unsigned long long* const rc = ring + c;
                unsigned long long v = 0;
                for(int q = -hw; q <= hw; q++) v += rc[((y8 + q - yl0) & (SC_RING - 1)) * SC_RP];
                for(int j = 0; j < 8; j++) {
                    const int y = y8 + j;
                    if(y >= ylim) break;
                    if(j) v += rc[((y + hw - yl0) & (SC_RING - 1)) * SC_RP] - rc[((y - hw - 1 - yl0) & (SC_RING - 1)) * SC_RP];
                    out[(size_t)y * X + x] = finish((unsigned)(v & 0xffff), (unsigned)((v >> 16) & 0xffff), (unsigned)((v >> 32) & 0xffff),
                                                    (unsigned)(v >> 48), y, x, Y, X, hw, metric);
                }
            }
        }
        ynext = ylim;
    }
}

struct Counts4 { unsigned a, b, c, d; };
__device__ __forceinline__ void count_in(Counts4& s, unsigned k) { s.a += k == 1; s.b += k == 2; s.c += k == 3; s.d += k == 4; }
__device__ __forceinline__ void count_out(Counts4& s, unsigned k) { s.a -= k == 1; s.b -= k == 2; s.c -= k == 3; s.d -= k == 4; }

// general path, rows: thread (y, run) forms the clipped row-window counts of SC_RUN columns of row y
__global__ __launch_bounds__(256) void k_score_rows(const unsigned char* __restrict__ cat, int Y, int X, int hw, uint4* __restrict__ rows) {
    const int runs = (X + SC_RUN - 1) / SC_RUN;
    const size_t total = (size_t)Y * runs, stride = (size_t)gridDim.x * blockDim.x;
    for(size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int y = (int)(i / runs), xa = (int)(i - (size_t)y * runs) * SC_RUN, xb = min(X, xa + SC_RUN);
        const unsigned char* const row = cat + (size_t)y * X;
        Counts4 s = {0, 0, 0, 0};
        for(int q = max(xa - hw, 0); q <= min(xa + hw, X - 1); q++) count_in(s, row[q]);
        for(int x = xa; x < xb; x++) {
            if(x > xa) {
                if(x + hw <= X - 1) count_in(s, row[x + hw]);
                if(x - hw - 1 >= 0) count_out(s, row[x - hw - 1]);
            }
            rows[(size_t)y * X + x] = make_uint4(s.a, s.b, s.c, s.d);
        }
    }
}

// general path, columns: thread (run, x) adds the row-window counts over the clipped rows of SC_RUN cells of column x and finishes them
__global__ __launch_bounds__(256) void k_score_cols(const uint4* __restrict__ rows, int Y, int X, int hw, int metric, float* __restrict__ out) {
    const int runs = (Y + SC_RUN - 1) / SC_RUN;
    const size_t total = (size_t)runs * X, stride = (size_t)gridDim.x * blockDim.x;
    for(size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int run = (int)(i / X), x = (int)(i - (size_t)run * X), ya = run * SC_RUN, yb = min(Y, ya + SC_RUN);
        uint4 s = make_uint4(0, 0, 0, 0);
        auto add = [&](const int y) { const uint4 v = rows[(size_t)y * X + x]; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; };
        auto sub = [&](const int y) { const uint4 v = rows[(size_t)y * X + x]; s.x -= v.x; s.y -= v.y; s.z -= v.z; s.w -= v.w; };
        for(int q = max(ya - hw, 0); q <= min(ya + hw, Y - 1); q++) add(q);
        for(int y = ya; y < yb; y++) {
            if(y > ya) {
                if(y + hw <= Y - 1) add(y + hw);
                if(y - hw - 1 >= 0) sub(y - hw - 1);
            }
            out[(size_t)y * X + x] = finish(s.x, s.y, s.z, s.w, y, x, Y, X, hw, metric);
        }
    }
}

// vector calc_score (metric_optimizer.cpp:188-204): counts[0..3] += the numbers of a / b / c / d elements.  A NaN ref is counted nowhere (both
// comparisons fail), a NaN fcst fails `fcst > fthreshold` and lands in c or d, as in the reference.
__global__ __launch_bounds__(256) void k_score_counts(const float* __restrict__ ref, const float* __restrict__ fcst, long long n, float threshold,
                                                      float fthreshold, unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long part[4][4];
    unsigned long long s[4] = {0, 0, 0, 0};
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float r = ref[i], f = fcst[i];
        const bool above = r > threshold, below = r <= threshold;
        if(f > fthreshold) { s[0] += above; s[1] += below; }
        else { s[2] += above; s[3] += below; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for(int k = 0; k < 4; k++) {
        for(int off = 32; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
        if(lane == 0) part[wave][k] = s[k];
    }
    __syncthreads();
    if(threadIdx.x < 4) {
        const unsigned long long t = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if(t) atomicAdd(counts + threadIdx.x, t);
    }
}

void check_metric(int metric) {
    if(!gpp_score_metric_known(metric)) invalid("Unknown metric");   // metric_optimizer.cpp:241-243
}

}   // namespace

extern "C" int gpp_calc_score_table(float a, float b, float c, float d, int metric, float* out) {
    GPP_TRY
    check_metric(metric);
    if(!out) invalid("out is NULL");
    *out = gpp_score_value(a, b, c, d, metric);
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_calc_score(const float* ref, const float* fcst, long long n, float threshold, float fthreshold, int metric, float* out, int mem) {
    GPP_TRY
    check_metric(metric);
    if(n < 0) invalid("negative size");
    if(!out) invalid("out is NULL");
    unsigned long long h[4] = {0, 0, 0, 0};
    if(n > 0) {
        if(!ref || !fcst) invalid("ref / fcst is NULL");
        ensure_device();
        InField r, f;
        r.bind(ref, (size_t)n, mem);
        f.bind(fcst, (size_t)n, mem);
        DevBuf<unsigned long long> counts;
        counts.get(4);
        GPP_HIP(hipMemsetAsync(counts.p, 0, 4 * sizeof(unsigned long long), stream()));
        launch(k_score_counts, grid_capped(blocks_of(n), 8192), 256, 0, r.d, f.d, n, threshold, fthreshold, counts.p);
        GPP_HIP(hipMemcpyAsync(h, counts.p, sizeof(h), hipMemcpyDeviceToHost, stream()));
        GPP_HIP(hipStreamSynchronize(stream()));
    }
    // the reference counts with `float x++`, which stops growing at 2^24
    float t[4];
    for(int k = 0; k < 4; k++) t[k] = (float)std::min<unsigned long long>(h[k], 16777216ull);
    *out = gpp_score_value(t[0], t[1], t[2], t[3], metric);
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_neighbourhood_score(gpp_points* grid, gpp_points* points, const float* fcst, const float* ref, int half_width, int metric,
                                       float threshold, float* out, int mem) {
    GPP_TRY
    if(!grid || !points) invalid("points is NULL");
    if(half_width <= 0) invalid("half_width must be greater than 0");   // neighbourhood_score.cpp:12-14
    check_metric(metric);
    const int Y = grid->ny, X = grid->nx;
    if((long long)Y * X != grid->n) invalid("grid is not a Grid");
    if(grid->n == 0) return GPP_OK;
    if(!fcst || !out) invalid("fcst / out is NULL");
    if(points->n > 0 && !ref) invalid("ref is NULL");
    ensure_device();
    const size_t C = (size_t)grid->n;
    InField f, r;
    OutField o;
    f.bind(fcst, C, mem);
    if(points->n > 0) r.bind(ref, (size_t)points->n, GPP_MEM_HOST);   // the observations are a host vector whatever `mem` says
    o.bind(out, C, mem);
    // the gridded reference is formed in the output plane and classified from there: it never leaves HBM
    gpp_gridding_nearest_device(grid, points, r.d, 1, GPP_MEAN, o.d);
    Staged<unsigned char> cat;
    cat.get(C);
    launch(k_score_classify, blocks_of(C), 256, 0, (const float*)o.d, f.d, C, threshold, cat.p);
    if(half_width <= SC_MAXHW && !path_env("GPP_SCORE_GENERAL")) {
        const int strips = (X + SC_W - 1) / SC_W;
        const long fill = path_env("GPP_SCORE_FILL") ? std::max(1, atoi(path_env("GPP_SCORE_FILL"))) : 1024;   // (tests: workgroups the launch aims for)
        const MarchSegments sg = march_segments(Y, SC_C, std::max(1L, (fill + strips - 1) / strips));   // about a thousand workgroups where the field has them
        launch(k_score_march, dim3(strips, sg.segs), SC_THREADS, 0, (const unsigned char*)cat.p, Y, X, half_width, metric, sg.SH, o.d);
    }
    else {
        const int hw = std::min(half_width, std::max(Y, X));   // a window that covers the field either way
        Staged<uint4> rows;
        rows.get(C);
        const size_t cap = (size_t)1 << 22;   // (the two kernels stride over their grid; the field has cells here, so neither grid is empty)
        launch(k_score_rows, grid_capped(blocks_of((size_t)Y * ((X + SC_RUN - 1) / SC_RUN)), cap), 256, 0, (const unsigned char*)cat.p, Y, X, hw, rows.p);
        launch(k_score_cols, grid_capped(blocks_of((size_t)X * ((Y + SC_RUN - 1) / SC_RUN)), cap), 256, 0, (const uint4*)rows.p, Y, X, hw, metric, o.d);
    }
    return finish_call(o);   // (the workspaces go back to the pool here)
    GPP_CATCH
}
