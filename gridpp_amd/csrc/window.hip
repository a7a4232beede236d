// gridpp::window (src/api/window.cpp:6-156, include/gridpp.h:1602-1611) for gfx950: running statistics along the time axis of a
// (locations, times) matrix, [Y][T] with T contiguous.
//
// The window of column x is [x - back, x + ahead] clipped to [0, T - 1]: back = ahead = length / 2 (centred), back = length - 1 and
// ahead = 0 (`before`).  The host clamps both to T, which changes no result: a window that reaches past either end is clipped there and
// counts as "overshooting the edge" for every x either way.
//
//   k_window_scan<VEC, false>   Mean / Sum / Count, fused.  The reference takes differences of a SEQUENTIAL float32 prefix sum per row
//                               (window.cpp:33-111), and that difference is not the exact window sum (1.9e-4 relative at T = 600,
//                               tests/test_window_restatement.py): a parallel scan cannot reproduce it, so one thread owns one row and
//                               adds along T in the reference's order; the parallelism is across rows.  A workgroup of WIN_ROWS lanes
//                               moves tiles of WIN_ROWS x WIN_COLS values between HBM and LDS with coalesced accesses (16 bytes per
//                               lane where T and the addresses allow: VEC = 4) and every lane walks its own LDS row.  The running
//                               prefix P and count N stay in registers from chunk to chunk; the last WIN_RING of them are kept in an
//                               LDS ring per row, which is where an output finds P[end] (up to `ahead` columns in front of it: the
//                               walk runs `lead` = ahead rounded up to 4 columns in front of the outputs) and P[start - 1].  The next
//                               chunk's loads are issued before the walk of this one.  One read and one write of the matrix.  The
//                               counts of the ring are 16 bits wide: only differences over a window of at most WIN_RING columns are
//                               taken from them.
//   k_window_scan<VEC, true>    the general path's first pass: the same walk, but the tile of P and the tile of N go to two [Y][T]
//                               planes in HBM; k_window_from_planes then forms every output from four plane reads.  Any length, any T.
//   k_window_gather<VEC>        Min / Max / Median / Std / Variance / RandomChoice, fused: the tile carries a column halo of `back`
//                               and `ahead` (rounded up to 4), one thread per output calls row_statistic / row_quantile
//                               (row_stats.h: calc_statistic, util.cpp:19-178) on its LDS row segment.
//   k_window_gather_rows        the same per output on the row in HBM: the general path of those statistics.
//
// LDS rows have an odd number of words, so the 32 lanes of a half wavefront, each on its own row, hit 32 different banks in every
// step of the walk; the cooperative side writes rows of consecutive words.
//
// A span fits the fused tile while back + lead <= GPP_WINDOW_FUSED_SPAN; GPP_WINDOW_GENERAL (a path override) sends every call down
// the general path.  Both give the same bits: the additions of a row are the same sequence in both.
#include "common.h"
#include "row_stats.h"
#include <algorithm>
#include <cstdint>

#pragma clang fp contract(off)

using namespace gpp;

namespace {

constexpr int WIN_ROWS = GPP_WINDOW_TILE_ROWS;    // rows of a tile = lanes of a scan workgroup
constexpr int WIN_COLS = GPP_WINDOW_TILE_COLS;    // columns of a chunk
constexpr int WIN_RING = 64;                      // prefix entries kept per row
constexpr int WIN_SPAN = GPP_WINDOW_FUSED_SPAN;   // back + lead of a fused call: lead + WIN_COLS + back + 1 <= WIN_RING
static_assert(WIN_SPAN + WIN_COLS + 1 <= WIN_RING, "the ring holds P[start - 1] of the oldest pending output and the newest prefix");
static_assert((WIN_RING & (WIN_RING - 1)) == 0 && WIN_ROWS == 64 && WIN_COLS % 4 == 0, "tile geometry");
// scan row: the ring of P, the ring of N (two 16-bit counts per word), the chunk's staging (inputs in, results out), one word of padding
constexpr int SCAN_ROW_WORDS = WIN_RING + WIN_RING / 2 + WIN_COLS + 1;
// gather row: back halo + chunk + ahead halo (each halo rounded up to 4: at most WIN_SPAN + 1 together), the results, one word of padding
constexpr int GATHER_TILE_COLS = WIN_COLS + WIN_SPAN + 1;
constexpr int GATHER_ROW_WORDS = GATHER_TILE_COLS + WIN_COLS + 1;
constexpr int GATHER_THREADS = 256;
static_assert(SCAN_ROW_WORDS % 2 == 1 && GATHER_ROW_WORDS % 2 == 1 && GATHER_TILE_COLS % 4 == 0, "odd row strides, whole 16-byte groups");

// columns [col0, col0 + ncols) of rows [row0, row0 + rows) between HBM and the LDS rows (word `off` of each row); columns outside
// [0, T) are left alone.  VEC = 4: col0, ncols and T are multiples of 4 and the base is 16-byte aligned, a group is inside or outside
// as a whole.  NC: the row length the lanes are dealt over (a compile-time constant >= ncols).
template <int VEC, int NC, int ROW_WORDS>
__device__ __forceinline__ void tile_load(const float* __restrict__ in, long long row0, int rows, int T, int col0, int ncols, float* lds, int off) {
    constexpr int PER_ROW = NC / VEC;
    for(int i = threadIdx.x; i < WIN_ROWS * PER_ROW; i += blockDim.x) {
        const int r = i / PER_ROW, j = (i % PER_ROW) * VEC;
        const int x = col0 + j;
        if(r >= rows || j >= ncols || x < 0 || x >= T) continue;
        const float* src = in + (row0 + r) * (long long)T + x;
        float* dst = lds + r * ROW_WORDS + off + j;
        if constexpr(VEC == 4) {
            const float4 q = *reinterpret_cast<const float4*>(src);
            dst[0] = q.x; dst[1] = q.y; dst[2] = q.z; dst[3] = q.w;
        }
        else dst[0] = src[0];
    }
}
template <int VEC, int NC, int ROW_WORDS>
__device__ __forceinline__ void tile_store(float* __restrict__ out, long long row0, int rows, int T, int col0, const float* lds, int off) {
    constexpr int PER_ROW = NC / VEC;
    for(int i = threadIdx.x; i < WIN_ROWS * PER_ROW; i += blockDim.x) {
        const int r = i / PER_ROW, j = (i % PER_ROW) * VEC;
        const int x = col0 + j;
        if(r >= rows || x < 0 || x >= T) continue;
        float* dst = out + (row0 + r) * (long long)T + x;
        const float* src = lds + r * ROW_WORDS + off + j;
        if constexpr(VEC == 4) *reinterpret_cast<float4*>(dst) = make_float4(src[0], src[1], src[2], src[3]);
        else dst[0] = src[0];
    }
}

// window.cpp:56-109 for one output, given the prefix and the count at `end` and at `start - 1` (both 0 where start == 0: the
// reference reads counts[-1] there and its tests pin 0), n = N[end] - N[start - 1] and the clipped bounds
__device__ __forceinline__ float scan_output(float p_end, float p_before, int n, int x, int start, int end, int T, int back, int ahead,
                                             int statistic, int keep_missing, int missing_edges) {
    if(statistic == GPP_COUNT) return (float)n;                                     // :82-84, whatever the two flags say
    float v = NAN;
    if(n != 0) v = start > 0 ? p_end - p_before : p_end;                            // :71-80
    if(statistic == GPP_MEAN && n != 0) v = v / (float)n;                           // :86-90 (n == 0 with N[end] != 0: NaN / 0 there, NaN here)
    if(keep_missing && n < end - start + 1) v = NAN;                                // :91-95
    if(missing_edges && (x < back || x + ahead + 1 > T)) v = NAN;                   // :97-108
    return v;
}

// the scan workgroup's chunk in two halves: HBM -> registers (issued one chunk ahead, so that the loads are in flight during the walk
// of the chunk before: a workgroup is one wavefront and only four fit a compute unit's LDS, nothing else hides the latency), registers
// -> the staging area of the LDS rows.  Both halves evaluate the same predicate: a register left unset is never written.
template <int VEC>
__device__ __forceinline__ void scan_fetch(const float* __restrict__ in, long long row0, int rows, int T, int col0, float (&reg)[WIN_COLS]) {
    constexpr int PER_ROW = WIN_COLS / VEC;
#pragma unroll
    for(int g = 0; g < WIN_COLS / VEC; g++) {
        const int i = (int)threadIdx.x + WIN_ROWS * g;
        const int r = i / PER_ROW, x = col0 + (i % PER_ROW) * VEC;
        if(r >= rows || x < 0 || x >= T) continue;
        const float* src = in + (row0 + r) * (long long)T + x;
        if constexpr(VEC == 4) {
            const float4 q = *reinterpret_cast<const float4*>(src);
            reg[4 * g] = q.x; reg[4 * g + 1] = q.y; reg[4 * g + 2] = q.z; reg[4 * g + 3] = q.w;
        }
        else reg[g] = src[0];
    }
}
template <int VEC>
__device__ __forceinline__ void scan_commit(const float (&reg)[WIN_COLS], int rows, int T, int col0, float* lds, int off) {
    constexpr int PER_ROW = WIN_COLS / VEC;
#pragma unroll
    for(int g = 0; g < WIN_COLS / VEC; g++) {
        const int i = (int)threadIdx.x + WIN_ROWS * g;
        const int r = i / PER_ROW, j = (i % PER_ROW) * VEC, x = col0 + j;
        if(r >= rows || x < 0 || x >= T) continue;
        float* dst = lds + r * SCAN_ROW_WORDS + off + j;
#pragma unroll
        for(int e = 0; e < VEC; e++) dst[e] = reg[g * VEC + e];
    }
}

template <int VEC, bool PLANES>
__global__ __launch_bounds__(WIN_ROWS) void k_window_scan(const float* __restrict__ in, long long Y, int T, int back, int ahead, int lead,
                                                          int statistic, int keep_missing, int missing_edges, float* __restrict__ out,
                                                          int* __restrict__ out_n) {
    __shared__ float lds[WIN_ROWS * SCAN_ROW_WORDS];
    const int lane = threadIdx.x;
    float* ring_p = lds + lane * SCAN_ROW_WORDS;
    unsigned short* ring_n = reinterpret_cast<unsigned short*>(ring_p + WIN_RING);
    float* stage = ring_p + WIN_RING + WIN_RING / 2;
    constexpr int STAGE = WIN_RING + WIN_RING / 2;
    const long long nblocks = (Y + WIN_ROWS - 1) / WIN_ROWS;
    for(long long rb = blockIdx.x; rb < nblocks; rb += gridDim.x) {
        const long long row0 = rb * WIN_ROWS;
        const int rows = (int)std::min<long long>(WIN_ROWS, Y - row0);
        float P = 0;   // window.cpp:34-54: the running sum and count of the row's valid values
        int N = 0;
        float reg[WIN_COLS];
        // step k: the walk takes the columns [k C + lead, k C + lead + C), then the outputs [k C, k C + C) have all they need
        int k = lead > 0 ? -1 : 0;
        scan_fetch<VEC>(in, row0, rows, T, k * WIN_COLS + lead, reg);
        for(; (long long)k * WIN_COLS < T; k++) {
            const int in0 = k * WIN_COLS + lead, out0 = k * WIN_COLS;
            __syncthreads();   // the stores of the step before have read the staging
            scan_commit<VEC>(reg, rows, T, in0, lds, STAGE);
            __syncthreads();
            scan_fetch<VEC>(in, row0, rows, T, in0 + WIN_COLS, reg);   // the next step's chunk (nothing beyond T)
            if(lane < rows) {
                // Fixed trip counts and no branch, so that the LDS reads of a chunk leave together.  A column outside [0, T) reads
                // whatever the staging holds and adds nothing; its ring slot belongs to a column at least 64 away from it, which no
                // pending output reads (the ring's live span ends 33 columns behind the walk), and its staging word is never stored.
                float v[WIN_COLS];
#pragma unroll
                for(int c = 0; c < WIN_COLS; c++) v[c] = stage[c];
#pragma unroll
                for(int c = 0; c < WIN_COLS; c++) {
                    const int x = in0 + c;
                    const bool counts = x >= 0 && x < T && dev_valid(v[c]);
                    P = counts ? P + v[c] : P;
                    N += counts ? 1 : 0;
                    if(PLANES) { stage[c] = P; reinterpret_cast<int*>(ring_p)[c] = N; }
                    else { ring_p[x & (WIN_RING - 1)] = P; ring_n[x & (WIN_RING - 1)] = (unsigned short)N; }
                }
                if(!PLANES && k >= 0) {
                    float o[WIN_COLS];
#pragma unroll
                    for(int c = 0; c < WIN_COLS; c++) {
                        const int x = min(out0 + c, T - 1);   // (beyond T: a copy of the last column, never stored)
                        const int start = max(0, x - back), end = min(T - 1, x + ahead);
                        const int e = end & (WIN_RING - 1), s = (start - 1) & (WIN_RING - 1);
                        const float p_before = start > 0 ? ring_p[s] : 0.0f;
                        const unsigned n_before = start > 0 ? ring_n[s] : 0u;
                        const int n = (int)((ring_n[e] - n_before) & 0xffffu);
                        o[c] = scan_output(ring_p[e], p_before, n, x, start, end, T, back, ahead, statistic, keep_missing, missing_edges);
                    }
#pragma unroll
                    for(int c = 0; c < WIN_COLS; c++) stage[c] = o[c];
                }
            }
            __syncthreads();
            if(PLANES) {
                tile_store<VEC, WIN_COLS, SCAN_ROW_WORDS>(out, row0, rows, T, in0, lds, STAGE);
                tile_store<VEC, WIN_COLS, SCAN_ROW_WORDS>(reinterpret_cast<float*>(out_n), row0, rows, T, in0, lds, 0);
            }
            else if(k >= 0) tile_store<VEC, WIN_COLS, SCAN_ROW_WORDS>(out, row0, rows, T, out0, lds, STAGE);
        }
    }
}

// the general path's second pass: one thread per output, window.cpp:56-109 from the planes
__global__ __launch_bounds__(256) void k_window_from_planes(const float* __restrict__ P, const int* __restrict__ N, long long total, int T,
                                                            int back, int ahead, int statistic, int keep_missing, int missing_edges,
                                                            float* __restrict__ out) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long long row = i / T;
        const int x = (int)(i - row * T);
        const int start = max(0, x - back), end = min(T - 1, x + ahead);
        const long long base = row * T;
        const float p_before = start > 0 ? P[base + start - 1] : 0.0f;
        const int n_before = start > 0 ? N[base + start - 1] : 0;
        out[i] = scan_output(P[base + end], p_before, N[base + end] - n_before, x, start, end, T, back, ahead, statistic, keep_missing, missing_edges);
    }
}

// window.cpp:112-152 for one output: seg = the clipped window's values in column order
__device__ __forceinline__ float gather_output(const float* seg, int n, bool outside, long long cell, int statistic, int keep_missing,
                                               int missing_edges) {
    int valid = 0;
    for(int i = 0; i < n; i++) valid += dev_valid(seg[i]) ? 1 : 0;
    if(keep_missing && valid < n) return NAN;     // :144-145
    if(missing_edges && outside) return NAN;      // :146-147
    if(statistic == GPP_MEDIAN) return row_quantile(seg, n, 0.5f);
    if(statistic == GPP_RANDOMCHOICE) {           // util.cpp:75-96 draws with rand(); any valid element of the window is a correct draw
        if(valid == 0) return NAN;
        unsigned h = (unsigned)cell * 2654435761u ^ (unsigned)(cell >> 32); h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        int pick = (int)(h % (unsigned)valid);
        for(int i = 0; i < n; i++)
            if(dev_valid(seg[i]) && pick-- == 0) return seg[i];
        return NAN;
    }
    return row_statistic(seg, n, statistic);
}

template <int VEC>
__global__ __launch_bounds__(GATHER_THREADS) void k_window_gather(const float* __restrict__ in, long long Y, int T, int back, int ahead,
                                                                  int statistic, int keep_missing, int missing_edges, float* __restrict__ out) {
    __shared__ float lds[WIN_ROWS * GATHER_ROW_WORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int back4 = (back + 3) & ~3, ahead4 = (ahead + 3) & ~3;
    const int ncols = back4 + WIN_COLS + ahead4;   // <= GATHER_TILE_COLS (the launcher's business)
    const float* tile = lds + lane * GATHER_ROW_WORDS;
    float* result = lds + lane * GATHER_ROW_WORDS + GATHER_TILE_COLS;
    const long long nblocks = (Y + WIN_ROWS - 1) / WIN_ROWS;
    for(long long rb = blockIdx.x; rb < nblocks; rb += gridDim.x) {
        const long long row0 = rb * WIN_ROWS;
        const int rows = (int)std::min<long long>(WIN_ROWS, Y - row0);
        for(int out0 = 0; out0 < T; out0 += WIN_COLS) {
            const int col0 = out0 - back4;   // the tile's first column
            __syncthreads();
            tile_load<VEC, GATHER_TILE_COLS, GATHER_ROW_WORDS>(in, row0, rows, T, col0, ncols, lds, 0);
            __syncthreads();
            if(lane < rows) {
                for(int c = wave; c < WIN_COLS; c += GATHER_THREADS / 64) {
                    const int x = out0 + c;
                    if(x >= T) break;
                    const int start = max(0, x - back), end = min(T - 1, x + ahead);
                    const bool outside = x < back || x + ahead + 1 > T;
                    result[c] = gather_output(tile + (start - col0), end - start + 1, outside, (row0 + lane) * (long long)T + x, statistic,
                                              keep_missing, missing_edges);
                }
            }
            __syncthreads();
            tile_store<VEC, WIN_COLS, GATHER_ROW_WORDS>(out, row0, rows, T, out0, lds, GATHER_TILE_COLS);
        }
    }
}

__global__ __launch_bounds__(256) void k_window_gather_rows(const float* __restrict__ in, long long total, int T, int back, int ahead,
                                                            int statistic, int keep_missing, int missing_edges, float* __restrict__ out) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long long row = i / T;
        const int x = (int)(i - row * T);
        const int start = max(0, x - back), end = min(T - 1, x + ahead);
        const bool outside = x < back || x + ahead + 1 > T;
        out[i] = gather_output(in + row * T + start, end - start + 1, outside, i, statistic, keep_missing, missing_edges);
    }
}

// every kernel here loops with a grid stride: 2^22 workgroups of at most 256 threads keep a launch below 2^32 threads, whatever Y and T
constexpr size_t WIN_MAXGRID = (size_t)1 << 22;

template <int VEC>
void window_launch(const float* in, long long Y, int T, int back, int ahead, int statistic, int keep, int edges, float* out) {
    const bool scan = statistic == GPP_MEAN || statistic == GPP_SUM || statistic == GPP_COUNT;
    const int lead = (ahead + 3) & ~3;
    const bool fused = back + lead <= WIN_SPAN && !path_env("GPP_WINDOW_GENERAL");
    const unsigned tiles = grid_capped(std::max<size_t>(blocks_of(Y, WIN_ROWS), 1), WIN_MAXGRID);
    const long long total = Y * T;
    const unsigned flat = grid_capped(std::max<size_t>(blocks_of(total), 1), WIN_MAXGRID);
    if(scan && fused)
        launch(k_window_scan<VEC, false>, tiles, WIN_ROWS, 0, in, Y, T, back, ahead, lead, statistic, keep, edges, out, (int*)nullptr);
    else if(scan) {
        Staged<float> P;   // the pool of common.h: gpp_release_workspaces() gives the planes back
        Staged<int> N;
        P.get((size_t)total);
        N.get((size_t)total);
        launch(k_window_scan<VEC, true>, tiles, WIN_ROWS, 0, in, Y, T, 0, 0, 0, statistic, keep, edges, P.p, N.p);
        launch(k_window_from_planes, flat, 256, 0, (const float*)P.p, (const int*)N.p, total, T, back, ahead, statistic, keep, edges, out);
        GPP_HIP(hipStreamSynchronize(stream()));   // the planes go back to the pool here
    }
    else if(fused)
        launch(k_window_gather<VEC>, tiles, GATHER_THREADS, 0, in, Y, T, back, ahead, statistic, keep, edges, out);
    else
        launch(k_window_gather_rows, flat, 256, 0, in, total, T, back, ahead, statistic, keep, edges, out);
}

}   // namespace

extern "C" int gpp_window(const float* array, long long ny, int nx, int length, int statistic, int before, int keep_missing, int missing_edges,
                          float* out, int mem) {
    GPP_TRY
    if(length <= 0) invalid("Length variable must be > 0");                                 // window.cpp:10-12
    if(ny < 0 || nx < 0) invalid("negative size");
    if(ny == 0 || nx == 0) return GPP_OK;                                                     // :14-22
    if(length % 2 == 0 && !before) invalid("Length variable must be an odd number");        // :26-28
    switch(statistic) {   // calc_statistic (util.cpp:97-106) throws for the rest inside the reference's loop: refused before any device work
        case GPP_MEAN: case GPP_SUM: case GPP_COUNT: case GPP_MIN: case GPP_MAX: case GPP_MEDIAN: case GPP_STD: case GPP_VARIANCE:
        case GPP_RANDOMCHOICE: break;
        default: runtime("Internal error. Cannot compute statistic");
    }
    if(!array || !out) invalid("array / out is NULL");
    ensure_device();
    const int T = nx;
    const int back = std::min(before ? length - 1 : length / 2, T), ahead = before ? 0 : std::min(length / 2, T);
    const size_t total = (size_t)ny * (size_t)T;
    InField a;
    OutField o;
    a.bind(array, total, mem);
    o.bind(out, total, mem);
    const bool wide = T % 4 == 0 && (((uintptr_t)a.d | (uintptr_t)o.d) & 15) == 0;
    if(wide) window_launch<4>(a.d, ny, T, back, ahead, statistic, keep_missing != 0, missing_edges != 0, o.d);
    else window_launch<1>(a.d, ny, T, back, ahead, statistic, keep_missing != 0, missing_edges != 0, o.d);
    return finish_call(o);
    GPP_CATCH
}
