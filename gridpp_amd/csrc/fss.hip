// gridpp_amd.fractions_skill_score: the Fractions Skill Score (Roberts & Lean 2008; for an ensemble the neighbourhood ensemble probability of
// Schwartz & Sobash 2017) of a forecast against a reference field for T thresholds x H half widths in one call.  No counterpart in the
// reference.  DESIGN.md 4.22 holds the definition; in short, per threshold a cell carries four small integers -- k (valid members that
// meet the threshold), m (valid members), o (the reference meets it) and c (the cell counts: ref valid and m > 0; all four are 0 where it
// does not) -- and per half width every cell whose clipped window holds n > 0 counting cells adds (K / M - O / n)^2 to fbs and
// (K / M)^2 + (O / n)^2 to fbs_worst, K, M, O, n being the exact window sums and the arithmetic double.  No float plane exists anywhere.
//
//   k_fss_classify      2-D forecast, once per call: one thread per cell reads fcst and ref and writes one byte per threshold, 2 k + o,
//                       and the byte m (= c).
//   k_fss_count<CT>     cube, once per FS_TB thresholds: a workgroup takes 256 cells; their members go through LDS FS_EC at a time
//                       (16 lanes read the 64 contiguous bytes of a cell, pitch 17 words so that the 64 rows a wavefront walks lie in
//                       different banks) and thread c walks row c with FS_TB counters in registers.  CT, the type of a plane's cell, is
//                       chosen by E so that 2 E + 1 fits: 8 bits up to E = 127, 16 up to 32767, 32 beyond.
//   k_fss_march<CT>     half widths up to GPP_FSS_FUSED_MAXHW while the packed form holds: row pass and column pass in one kernel in the
//                       shape of k_score_march (score.hip): a strip of FS_W columns, chunks of FS_C rows through LDS as one 32-bit code per
//                       cell (k: bits 0-14, m: 15-29, o: 30, c: 31), a ring of FS_RING rows of row-window sums packed in ONE 64-bit word
//                       with lanes K | M | O | n of bk, bk, bn and bn bits, column sums of ring words, again packed.  blockIdx.z is the
//                       threshold.  The finish step unpacks and forms the two terms in double; the workgroup adds them (wave shuffles,
//                       then LDS) and stores ONE partial per sum.  LDS: 32 x 97 words + 64 x 65 double words + the 96 bytes of the
//                       workgroup sum = 45 792 bytes, three workgroups per CU; both pitches are odd, as in k_score_march, whose bank analysis carries over
//                       with a word where that kernel has a byte.
//   k_fss_rows<CT, RT>  the general path, any half width (the host clamps it to the longer side) and any E: a separable pair, the row
//   k_fss_cols<RT>      sums K, M (RT: 32 bits while (2 hw + 1) E < 2^32, 64 beyond), O, n in a workspace plane, the column sums in 64-bit
//                       counters whatever RT is, so a window sum may pass 2^32; the same finish and the same workgroup sum.  The path
//                       override GPP_FSS_GENERAL forces it ("wide": with 64-bit row sums).  Every thread builds its first window from
//                       min(2 hw + 1, side) reads and then slides over FS_RUN = 32 outputs: the reads per output grow as (2 hw + 33) / 32,
//                       up to side / 32 for a window as wide as the field (no prefix pass bounds it).
//   k_fss_reduce        one workgroup per threshold adds the partials of the march in a fixed order: the result is bit-identical from
//                       call to call.  There is no floating-point atomic anywhere.
//
// Packing bound of the march: bn is the smallest width with (2 hw + 1)^2 < 2^bn, bk = (64 - 2 bn) / 2; the lanes K and M hold at most
// (2 hw + 1)^2 E, so the march is taken while (2 hw + 1)^2 E < 2^bk and E <= 32767 (the 15-bit fields of the code).  At hw = 16: bn = 11,
// bk = 21, E <= 1925.  Lane sums are sums of non-negative terms that fit, and a sliding difference takes out only what was put in, so no lane
// ever borrows from its neighbour.
#include "common.h"
#include "march_geom.h"
#include <algorithm>
#include <cstdint>

#pragma clang fp contract(off)

using namespace gpp;

namespace {

typedef unsigned long long u64;

constexpr int FS_W = GPP_FSS_TILE_COLS;             // output columns of a strip
constexpr int FS_C = GPP_FSS_TILE_ROWS;             // rows of a chunk
constexpr int FS_RING = 64;                         // rows of row-window sums kept
constexpr int FS_MAXHW = GPP_FSS_FUSED_MAXHW;
constexpr int FS_WT = FS_W + 2 * FS_MAXHW;          // codes of a chunk row: the strip and both halos
constexpr int FS_P = FS_WT + 1;                     // their pitch in LDS, in words: odd
constexpr int FS_RP = FS_W + 1;                     // pitch of a ring row in 8-byte words: odd
constexpr int FS_THREADS = 256;
constexpr int FS_PRE = FS_C * FS_WT / FS_THREADS;   // codes of a chunk that one thread moves
constexpr int FS_RUN = 32;                          // outputs per thread of the general path's sliding sums
constexpr int FS_TB = 8;                            // thresholds k_fss_count carries in registers
constexpr int FS_EC = 16;                           // members of a cell that go through LDS together
constexpr int FS_EP = FS_EC + 1;                    // pitch of a cell's members in LDS
constexpr int FS_MAXBLOCKS = 2048;                  // workgroups of the general path's kernels (of a field with cells: the entry point returns before them otherwise)
static_assert(FS_C + 2 * FS_MAXHW <= FS_RING && (FS_RING & (FS_RING - 1)) == 0, "the ring holds every row that a pending output needs");
static_assert(FS_C * FS_WT % FS_THREADS == 0 && FS_THREADS == 8 * FS_C && FS_THREADS == 4 * FS_W && FS_W == 64 && FS_C == 32, "thread layout");
static_assert(FS_P % 2 == 1 && FS_RP % 2 == 1, "odd pitches");

// `v op t` for a valid v and a t that is no NaN: Gt as it stands, Lt with the sides swapped, Leq and Geq as the negation of those two
__device__ __forceinline__ bool dev_raw(float v, float t, int swap) { return swap ? t > v : v > t; }

__global__ __launch_bounds__(256) void k_fss_classify(const float* __restrict__ fcst, const float* __restrict__ ref, size_t C, const float* __restrict__ thr,
                                                      int T, int swap, int neg, unsigned char* __restrict__ mp, unsigned char* __restrict__ kp) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for(size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < C; i += stride) {
        const float f = fcst[i], r = ref[i];
        const bool counts = dev_valid(f) && dev_valid(r);
        mp[i] = counts ? 1 : 0;
        for(int t = 0; t < T; t++) {
            const float th = thr[t];
            const unsigned k = dev_raw(f, th, swap) != (neg != 0), o = dev_raw(r, th, swap) != (neg != 0);
            kp[(size_t)t * C + i] = counts ? (unsigned char)(2 * k + o) : (unsigned char)0;
        }
    }
}

// thresholds thr[0 .. nt), nt <= FS_TB; kp is the plane of the first of them
template <class CT>
__global__ __launch_bounds__(256) void k_fss_count(const float* __restrict__ cube, const float* __restrict__ ref, size_t C, int E, const float* __restrict__ thr,
                                                   int nt, int swap, int neg, int write_m, CT* __restrict__ mp, CT* __restrict__ kp) {
    __shared__ float tile[256 * FS_EP];
    const int tid = threadIdx.x;
    float th[FS_TB];
#pragma unroll
    for(int t = 0; t < FS_TB; t++) th[t] = t < nt ? thr[t] : 0.0f;
    for(size_t c0 = (size_t)blockIdx.x * 256; c0 < C; c0 += (size_t)gridDim.x * 256) {
        unsigned m = 0, raw[FS_TB];
#pragma unroll
        for(int t = 0; t < FS_TB; t++) raw[t] = 0;
        const size_t cell = c0 + tid;
        for(int e0 = 0; e0 < E; e0 += FS_EC) {
            const int ec = min(FS_EC, E - e0);
            __syncthreads();   // every thread has walked the members before
#pragma unroll
            for(int j = 0; j < FS_EC; j++) {
                const int i = tid + 256 * j, c = i / FS_EC, q = i - c * FS_EC;
                if(q < ec && c0 + c < C) tile[c * FS_EP + q] = cube[(c0 + c) * (size_t)E + e0 + q];
            }
            __syncthreads();
            if(cell < C) {
                for(int q = 0; q < ec; q++) {
                    const float v = tile[tid * FS_EP + q];
                    const bool ok = dev_valid(v);
                    m += ok;
#pragma unroll
                    for(int t = 0; t < FS_TB; t++)
                        if(t < nt) raw[t] += ok && dev_raw(v, th[t], swap);
                }
            }
        }
        if(cell < C) {
            const float r = ref[cell];
            const bool counts = dev_valid(r) && m > 0;
            if(write_m) mp[cell] = counts ? (CT)m : (CT)0;
#pragma unroll
            for(int t = 0; t < FS_TB; t++) {
                if(t < nt) {
                    const unsigned k = neg ? m - raw[t] : raw[t], o = dev_raw(r, th[t], swap) != (neg != 0);
                    kp[(size_t)t * C + cell] = counts ? (CT)(2 * k + o) : (CT)0;
                }
            }
        }
    }
}

struct FsSums {
    double a = 0.0, b = 0.0;   // fbs, fbs_worst
    u64 cells = 0;
};

// the two terms of a cell from its exact window sums
__device__ __forceinline__ void fs_finish(FsSums& s, u64 K, u64 M, u64 O, u64 n) {
    if(n == 0) return;
    const double Ff = (double)K / (double)M, Fo = (double)O / (double)n;
    const double d = Ff - Fo;
    s.a += d * d;
    s.b += Ff * Ff + Fo * Fo;
    s.cells++;
}

// every thread of the workgroup (256) comes here once: wave shuffles, then LDS, then one partial per sum in pa / pb (and pc where given)
__device__ __forceinline__ void fs_block_store(FsSums s, double* sh, size_t slot, double* __restrict__ pa, double* __restrict__ pb, u64* __restrict__ pc,
                                               size_t cslot) {
    for(int off = 32; off > 0; off >>= 1) {
        s.a += __shfl_down(s.a, off, 64);
        s.b += __shfl_down(s.b, off, 64);
        s.cells += __shfl_down(s.cells, off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64* const shc = reinterpret_cast<u64*>(sh + 8);
    if(lane == 0) { sh[wave] = s.a; sh[4 + wave] = s.b; shc[wave] = s.cells; }
    __syncthreads();
    if(threadIdx.x == 0) {
        pa[slot] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
        pb[slot] = ((sh[4] + sh[5]) + sh[6]) + sh[7];
        if(pc) pc[cslot] = shc[0] + shc[1] + shc[2] + shc[3];
    }
}

// blockIdx.x: the strip, blockIdx.y: the segment of SH rows (a multiple of FS_C), blockIdx.z: the threshold.  0 <= hw <= FS_MAXHW.
template <class CT>
__global__ __launch_bounds__(FS_THREADS) void k_fss_march(const CT* __restrict__ mp, const CT* __restrict__ kp, size_t C, int Y, int X, int hw, int SH, int bk,
                                                          int bn, double* __restrict__ pa, double* __restrict__ pb, u64* __restrict__ pc) {
    __shared__ unsigned tin[FS_C * FS_P];          // the codes of the chunk's rows, column x0 - hw first; 0 outside the field
    __shared__ u64 ring[FS_RING * FS_RP];          // packed row-window sums of the strip's columns; slot of row y: (y - yl0) % FS_RING
    __shared__ double red[12];
    const CT* const kt = kp + (size_t)blockIdx.z * C;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * FS_W;
    const int ya = blockIdx.y * SH, yb = min(Y, ya + SH);
    const int yl0 = ya - hw;                       // first row the segment loads
    const int nchunk = (yb - 1 + hw - yl0) / FS_C + 1;
    const int Wt = FS_W + 2 * hw;
    const u64 maskk = (1ull << bk) - 1, maskn = (1ull << bn) - 1;
    auto expand = [&](const unsigned code) {
        return (u64)(code & 0x7fffu) | ((u64)((code >> 15) & 0x7fffu) << bk) | ((u64)((code >> 30) & 1u) << (2 * bk)) | ((u64)(code >> 31) << (2 * bk + bn));
    };
    unsigned pre[FS_PRE];
    auto fetch = [&](const int k) {
#pragma unroll
        for(int j = 0; j < FS_PRE; j++) {
            const int i = tid + FS_THREADS * j, r = i / FS_WT, t = i - r * FS_WT;
            const int y = yl0 + k * FS_C + r, x = x0 - hw + t;
            unsigned code = 0;
            if(t < Wt && y >= 0 && y < Y && x >= 0 && x < X) {
                const size_t at = (size_t)y * X + x;
                const unsigned m = mp[at], ko = kt[at];
                code = (ko >> 1) | (m << 15) | ((ko & 1u) << 30) | (m ? 0x80000000u : 0u);
            }
            pre[j] = code;
        }
    };
    FsSums sums;
    fetch(0);
    int ynext = ya;
    for(int k = 0; k < nchunk; k++) {
#pragma unroll
        for(int j = 0; j < FS_PRE; j++) {
            const int i = tid + FS_THREADS * j, r = i / FS_WT;
            tin[r * FS_P + (i - r * FS_WT)] = pre[j];
        }
        __syncthreads();   // the chunk is in LDS; every thread has left the column pass of the chunk before
        if(k + 1 < nchunk) fetch(k + 1);
        {   // row pass: thread (r, sg) slides along the eight columns of segment sg of row r
            const int r = tid & (FS_C - 1), sg = tid / FS_C;
            const unsigned* const row = tin + r * FS_P + 8 * sg;   // the window of column 8 sg + j is row[j .. j + 2 hw]
            u64* const rs = ring + ((k * FS_C + r) & (FS_RING - 1)) * FS_RP + 8 * sg;
            u64 s = 0;
            for(int q = 0; q <= 2 * hw; q++) s += expand(row[q]);
            rs[0] = s;
#pragma unroll
            for(int j = 1; j < 8; j++) {
                s += expand(row[j + 2 * hw]) - expand(row[j - 1]);
                rs[j] = s;
            }
        }
        __syncthreads();   // the ring holds the rows up to ytop
        const int ytop = yl0 + (k + 1) * FS_C - 1;
        const int ylim = max(ynext, min(yb, ytop - hw + 1));   // outputs [ynext, ylim) have their 2 hw + 1 rows in the ring: at most FS_C of them
        {   // column pass: thread (c, g) slides down eight rows of column c
            const int c = tid & (FS_W - 1), x = x0 + c;
            const int y8 = ynext + 8 * (tid / FS_W);
            if(y8 < ylim && x < X) {
                const u64* const rc = ring + c;
                u64 v = 0;
                for(int q = -hw; q <= hw; q++) v += rc[((y8 + q - yl0) & (FS_RING - 1)) * FS_RP];
                for(int j = 0; j < 8; j++) {
                    const int y = y8 + j;
                    if(y >= ylim) break;
                    if(j) v += rc[((y + hw - yl0) & (FS_RING - 1)) * FS_RP] - rc[((y - hw - 1 - yl0) & (FS_RING - 1)) * FS_RP];
                    fs_finish(sums, v & maskk, (v >> bk) & maskk, (v >> (2 * bk)) & maskn, v >> (2 * bk + bn));
                }
            }
        }
        ynext = ylim;
    }
    const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x, nblk = (size_t)gridDim.x * gridDim.y;
    fs_block_store(sums, red, (size_t)blockIdx.z * nblk + blk, pa, pb, blockIdx.z == 0 ? pc : nullptr, blk);
}

template <class RT>
struct FsRow {
    RT K, M;
    unsigned O, n;
};

// general path, rows: thread (y, run) forms the clipped row-window sums of FS_RUN columns of row y
template <class CT, class RT>
__global__ __launch_bounds__(256) void k_fss_rows(const CT* __restrict__ mp, const CT* __restrict__ kt, int Y, int X, long long hw, FsRow<RT>* __restrict__ rows) {
    const long long runs = ((long long)X + FS_RUN - 1) / FS_RUN;
    const size_t total = (size_t)Y * runs, stride = (size_t)gridDim.x * blockDim.x;
    for(size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long long y = (long long)(i / runs), xa = (long long)(i - (size_t)y * runs) * FS_RUN, xb = min((long long)X, xa + FS_RUN);
        const CT* const mrow = mp + (size_t)y * X;
        const CT* const krow = kt + (size_t)y * X;
        FsRow<RT> s = {0, 0, 0, 0};
        auto add = [&](const long long q) { const unsigned m = mrow[q], ko = krow[q]; s.K += ko >> 1; s.M += m; s.O += ko & 1u; s.n += m != 0; };
        auto sub = [&](const long long q) { const unsigned m = mrow[q], ko = krow[q]; s.K -= ko >> 1; s.M -= m; s.O -= ko & 1u; s.n -= m != 0; };
        for(long long q = max(xa - hw, 0ll); q <= min(xa + hw, (long long)X - 1); q++) add(q);
        for(long long x = xa; x < xb; x++) {
            if(x > xa) {
                if(x + hw <= X - 1) add(x + hw);
                if(x - hw - 1 >= 0) sub(x - hw - 1);
            }
            rows[(size_t)y * X + x] = s;
        }
    }
}

// general path, columns: thread (run, x) adds the row sums over the clipped rows of FS_RUN cells of column x in 64-bit counters and finishes them
template <class RT>
__global__ __launch_bounds__(256) void k_fss_cols(const FsRow<RT>* __restrict__ rows, int Y, int X, long long hw, size_t slot0, double* __restrict__ pa,
                                                  double* __restrict__ pb, u64* __restrict__ pc) {
    __shared__ double red[12];
    const long long runs = ((long long)Y + FS_RUN - 1) / FS_RUN;
    const size_t total = (size_t)runs * X, stride = (size_t)gridDim.x * blockDim.x;
    FsSums sums;
    for(size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const long long run = (long long)(i / X), x = (long long)(i - (size_t)run * X), ya = run * FS_RUN, yb = min((long long)Y, ya + FS_RUN);
        u64 K = 0, M = 0, O = 0, n = 0;
        auto add = [&](const long long y) { const FsRow<RT> v = rows[(size_t)y * X + x]; K += v.K; M += v.M; O += v.O; n += v.n; };
        auto sub = [&](const long long y) { const FsRow<RT> v = rows[(size_t)y * X + x]; K -= v.K; M -= v.M; O -= v.O; n -= v.n; };
        for(long long q = max(ya - hw, 0ll); q <= min(ya + hw, (long long)Y - 1); q++) add(q);
        for(long long y = ya; y < yb; y++) {
            if(y > ya) {
                if(y + hw <= Y - 1) add(y + hw);
                if(y - hw - 1 >= 0) sub(y - hw - 1);
            }
            fs_finish(sums, K, M, O, n);
        }
    }
    fs_block_store(sums, red, slot0 + blockIdx.x, pa, pb, pc, blockIdx.x);
}

// blockIdx.x: the threshold of the batch.  Thread i adds the partials i, i + 256, ... in that order, then the 256 sums are added as a fixed tree.
__global__ __launch_bounds__(256) void k_fss_reduce(const double* __restrict__ pa, const double* __restrict__ pb, const u64* __restrict__ pc, size_t nblk,
                                                    double* __restrict__ fbs, double* __restrict__ worst, size_t out_stride, u64* __restrict__ cells) {
    __shared__ double sa[256], sb[256];
    __shared__ u64 sc[256];
    const int tid = threadIdx.x;
    const double* const a = pa + (size_t)blockIdx.x * nblk;
    const double* const b = pb + (size_t)blockIdx.x * nblk;
    double x = 0.0, y = 0.0;
    u64 c = 0;
    for(size_t i = tid; i < nblk; i += 256) {
        x += a[i];
        y += b[i];
        if(cells && blockIdx.x == 0) c += pc[i];
    }
    sa[tid] = x; sb[tid] = y; sc[tid] = c;
    __syncthreads();
    for(int w = 128; w > 0; w >>= 1) {
        if(tid < w) { sa[tid] += sa[tid + w]; sb[tid] += sb[tid + w]; sc[tid] += sc[tid + w]; }
        __syncthreads();
    }
    if(tid == 0) {
        fbs[(size_t)blockIdx.x * out_stride] = sa[0];
        worst[(size_t)blockIdx.x * out_stride] = sb[0];
        if(cells && blockIdx.x == 0) *cells = sc[0];
    }
}

// the widths of the march's lanes for this half width; false where the packed form does not hold (see the head of this file)
bool packed_form(int hw, int E, int Y, int X, int* bk, int* bn) {
    if(hw > FS_MAXHW || E > 32767 || Y > (1 << 30) || X > (1 << 30)) return false;
    const u64 area = (u64)(2 * hw + 1) * (2 * hw + 1);
    int b = 1;
    while(area >= (1ull << b)) b++;
    *bn = b;
    *bk = (64 - 2 * b) / 2;
    return area * (u64)E < (1ull << *bk);
}

struct FssCall {
    const float *fcst, *ref;
    int Y, X, E;
    size_t C;
    int swap, neg;
    int ctb;                       // bytes of a plane's cell
    Staged<unsigned char> mp, kp;  // the planes m and 2 k + o (one per threshold of the batch)
    Staged<unsigned char> rows;    // row sums of the general path
    Staged<double> parts;
    Staged<u64> pcnt;

    template <class CT>
    void count(const float* d_thr, int nt, bool first) {
        for(int t0 = 0; t0 < nt; t0 += FS_TB)
            launch(k_fss_count<CT>, grid_capped(blocks_of(C), FS_MAXBLOCKS), 256, 0, fcst, ref, C, E, d_thr + t0, std::min(FS_TB, nt - t0), swap, neg, first && t0 == 0 ? 1 : 0,
                   (CT*)mp.p, (CT*)kp.p + (size_t)t0 * C);
    }
    void classify(const float* d_thr, int nt, bool first, bool is3d) {
        if(!is3d) launch(k_fss_classify, grid_capped(blocks_of(C), FS_MAXBLOCKS), 256, 0, fcst, ref, C, d_thr, nt, swap, neg, mp.p, kp.p);
        else if(ctb == 1) count<unsigned char>(d_thr, nt, first);
        else if(ctb == 2) count<unsigned short>(d_thr, nt, first);
        else count<unsigned>(d_thr, nt, first);
    }

    template <class CT>
    size_t march(int hw, int nt, int bk, int bn) {
        const int strips = (X + FS_W - 1) / FS_W;
        const long fill = path_env("GPP_FSS_FILL") ? std::max(1, atoi(path_env("GPP_FSS_FILL"))) : 1024;   // (tests: workgroups per threshold the launch aims for)
        const MarchSegments sg = march_segments(Y, FS_C, std::max(1L, (fill + strips - 1) / strips));
        const size_t nblk = (size_t)strips * sg.segs;
        parts.get(2 * nblk * nt);
        pcnt.get(nblk);
        launch(k_fss_march<CT>, dim3(strips, sg.segs, nt), FS_THREADS, 0, (const CT*)mp.p, (const CT*)kp.p, C, Y, X, hw, sg.SH, bk, bn, parts.p, parts.p + nblk * nt, pcnt.p);
        return nblk;
    }

    template <class CT, class RT>
    size_t general(long long hw, int nt) {
        const size_t nblk = grid_capped(blocks_of((size_t)X * (((size_t)Y + FS_RUN - 1) / FS_RUN)), FS_MAXBLOCKS);
        parts.get(2 * nblk * nt);
        pcnt.get(nblk);
        rows.get(C * sizeof(FsRow<RT>));
        for(int t = 0; t < nt; t++) {
            launch(k_fss_rows<CT, RT>, grid_capped(blocks_of((size_t)Y * (((size_t)X + FS_RUN - 1) / FS_RUN)), FS_MAXBLOCKS), 256, 0, (const CT*)mp.p,
                   (const CT*)kp.p + (size_t)t * C, Y, X, hw, (FsRow<RT>*)rows.p);
            launch(k_fss_cols<RT>, (unsigned)nblk, 256, 0, (const FsRow<RT>*)rows.p, Y, X, hw, (size_t)t * nblk, parts.p, parts.p + nblk * nt, t == 0 ? pcnt.p : (u64*)nullptr);
        }
        return nblk;
    }
    template <class CT>
    size_t general_ct(long long hw, int nt, bool wide) { return wide ? general<CT, u64>(hw, nt) : general<CT, unsigned>(hw, nt); }

    // the sums of nt thresholds (whose planes are in kp) at one half width -> fbs[t * stride], worst[t * stride], *cells where given
    void scale(int halfwidth, int nt, double* d_fbs, double* d_worst, size_t stride, u64* d_cells) {
        const char* const force = path_env("GPP_FSS_GENERAL");
        int bk = 0, bn = 0;
        size_t nblk;
        if(!force && packed_form(halfwidth, E, Y, X, &bk, &bn))
            nblk = ctb == 1 ? march<unsigned char>(halfwidth, nt, bk, bn) : march<unsigned short>(halfwidth, nt, bk, bn);
        else {
            const long long hw = std::min(halfwidth, std::max(Y, X));   // a window that covers the field either way
            const bool wide = (force && !strcmp(force, "wide")) || (u64)std::min<long long>(2 * hw + 1, X) * (u64)E >= (1ull << 32);
            nblk = ctb == 1 ? general_ct<unsigned char>(hw, nt, wide) : ctb == 2 ? general_ct<unsigned short>(hw, nt, wide) : general_ct<unsigned>(hw, nt, wide);
        }
        launch(k_fss_reduce, nt, 256, 0, (const double*)parts.p, (const double*)(parts.p + nblk * nt), (const u64*)pcnt.p, nblk, d_fbs, d_worst, stride, d_cells);
    }
};

}   // namespace

extern "C" int gpp_fractions_skill_score(const float* fcst, const float* ref, int ny, int nx, int ne, int is3d, const float* thresholds, int nt,
                                         const int* halfwidths, int nh, int comparison_operator, double* fbs, double* fbs_worst, long long* cells, int mem) {
    GPP_TRY
    if(ny < 0 || nx < 0 || ne < 0 || nt < 0 || nh < 0) invalid("fractions_skill_score: negative size");
    if(!is3d && ne != 1) invalid("fractions_skill_score: a 2-D forecast has ne == 1");
    if((nt > 0 && !thresholds) || (nh > 0 && (!halfwidths || !cells)) || (nt > 0 && nh > 0 && (!fbs || !fbs_worst)))
        invalid("fractions_skill_score: thresholds / halfwidths / fbs / fbs_worst / cells is NULL");
    for(int t = 0; t < nt; t++)
        if(std::isnan(thresholds[t])) invalid("fractions_skill_score: a threshold is NaN");
    for(int h = 0; h < nh; h++)
        if(halfwidths[h] < 0) invalid("Half width must be > 0");
    if(comparison_operator != GPP_LT && comparison_operator != GPP_LEQ && comparison_operator != GPP_GT && comparison_operator != GPP_GEQ)
        invalid("Invalid comparison operator");
    for(int h = 0; h < nh; h++) cells[h] = 0;
    for(size_t i = 0; i < (size_t)nt * nh; i++) fbs[i] = fbs_worst[i] = 0.0;
    const size_t C = (size_t)ny * nx;
    if(nt == 0 || nh == 0 || C == 0 || ne == 0) return GPP_OK;
    if(!fcst || !ref) invalid("fractions_skill_score: fcst / ref is NULL");
    ensure_device();
    InField f, r;
    f.bind(fcst, C * ne, mem & GPP_MEM_DEVICE);
    r.bind(ref, C, mem & GPP_MEM_DEVICE);
    FssCall c{f.d, r.d, ny, nx, ne, C, comparison_operator == GPP_LT || comparison_operator == GPP_GEQ, comparison_operator == GPP_LEQ || comparison_operator == GPP_GEQ,
              ne <= 127 ? 1 : ne <= 32767 ? 2 : 4};
    Staged<float> d_thr;
    d_thr.upload(thresholds, nt);
    // thresholds go in batches whose planes stay within 256 MiB (and within a grid's z extent); the m plane is written with the first
    const int batch = (int)std::max<size_t>(1, std::min<size_t>({(size_t)nt, (size_t)1024, ((size_t)256 << 20) / (C * c.ctb)}));
    c.mp.get(C * c.ctb);
    c.kp.get(C * c.ctb * batch);
    Staged<double> d_sums;
    Staged<u64> d_cells;
    d_sums.get(2 * (size_t)nt * nh);
    d_cells.get(nh);
    double* const d_fbs = d_sums.p;
    double* const d_worst = d_sums.p + (size_t)nt * nh;
    for(int t0 = 0; t0 < nt; t0 += batch) {
        const int n = std::min(batch, nt - t0);
        c.classify(d_thr.p + t0, n, t0 == 0, is3d != 0);
        for(int h = 0; h < nh; h++)
            c.scale(halfwidths[h], n, d_fbs + (size_t)t0 * nh + h, d_worst + (size_t)t0 * nh + h, nh, t0 == 0 ? d_cells.p + h : nullptr);
    }
    static_assert(sizeof(long long) == sizeof(u64), "cells are copied as they are");
    GPP_HIP(hipMemcpyAsync(fbs, d_fbs, (size_t)nt * nh * sizeof(double), hipMemcpyDeviceToHost, stream()));
    GPP_HIP(hipMemcpyAsync(fbs_worst, d_worst, (size_t)nt * nh * sizeof(double), hipMemcpyDeviceToHost, stream()));
    GPP_HIP(hipMemcpyAsync(cells, d_cells.p, (size_t)nh * sizeof(u64), hipMemcpyDeviceToHost, stream()));
    GPP_HIP(hipStreamSynchronize(stream()));   // the workspaces go back to the pool here
    return GPP_OK;
    GPP_CATCH
}
