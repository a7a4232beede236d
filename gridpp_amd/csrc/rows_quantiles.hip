// Many exact quantiles of every row of a [rows][len] array on MI355X (gfx950): gpp_calc_quantiles, out[r][j] = calc_quantile(row r, levels[j]).
//
// The result contract is rows_select.hip's: valid means finite, the order is that of the f2ord keys, index and weight
// arithmetic is quantile_from_order's, levels 0 and 1 are the positional Min / Max of row_statistic.  Once a row of keys is sorted every
// level costs two LDS reads, so the paths below sort where a sort pays and return the bits of rows_quantile on every one of them:
//
//   tile   0 < len <= 160: one wave per 64 consecutive rows, staged as keys at the odd pitch len | 1 exactly as k_rows_tile stages them
//          (rq_stage_tile).  Lane l sorts row l in place with a normalised bitonic network over the next power of two: every comparator
//          puts the smaller key at the lower index, the element indices are the same in every lane (conflict-free at the odd pitch), and
//          the slots from len on are virtual RS_INV keys -- the largest key there is, which is also where the invalid values end up.  The
//          network runs in registers as far as it can: blocks of 8 keys are sorted outright, then every pass fuses two steps on 4 keys.
//          The 64 x nq results of a tile are one contiguous block of the output: they are staged in LDS by chunks of levels and stored
//          coalesced.
//   block  160 < len <= 8192: one 256-thread workgroup per row; the row's keys sorted in LDS by the same network, one
//          comparator per thread and step; then thread j takes level j.
//   loop   any len: rows_quantile once per level (its own tile / block / split dispatch), scattered into column j.  nq == 1 goes here.
//
// Levels 0 and 1 cannot be answered from a sorted row (a zero of either sign is the extreme: the first one in the ORIGINAL order wins),
// so both sorting paths take them from the keys before the sort, and only when such a level is present.
#include "common.h"
#include <algorithm>
#include "rows_select.h"

#pragma clang fp contract(off)
using namespace gpp;

#define RQ_BLOCK_MAXLEN 8192   // block: the keys of one row in LDS, 32 KB at most (4 workgroups = 16 waves per CU)
#define RQ_CHUNK 16            // tile: levels per staged block of results (64 x 17 words of LDS)
// Default dispatch: the fewest levels for which sorting beat one selection per level (measured: DESIGN.md 4.16).  The cost of a sort goes with
// the power of two P the network runs over, so the gates do: tile 2 levels up to P = 128 and 3 at P = 256; block 2 levels up to P = 2048, at
// P = 4096 3 levels up to len = 3584 and 4 beyond (the network skips fewer comparators as len nears P), 5 at P = 8192.
static int rq_min_levels(int len) {
    if(len <= 128) return 2;
    if(len <= RS_TILE_MAXLEN) return 3;
    return len <= 2048 ? 2 : len <= 3584 ? 3 : len <= 4096 ? 4 : 5;
}

// one level out of a sorted row of keys with N valid ones; mn / mx: the positional Min / Max (read only for q == 0 / q == 1)
__device__ __forceinline__ float rq_pick(const unsigned* sorted, int N, float q, float mn, float mx) {
    if(!dev_valid(q) || N == 0) return NAN;
    if(q == 0) return mn;
    if(q == 1) return mx;
    int lo, up;
    rs_indices(q, N, lo, up);
    const float lv = ord2f(sorted[lo]);
    const float uv = up != lo ? ord2f(sorted[up]) : lv;
    return quantile_from_order(q, N, lv, uv, lo, up);
}
#define RQ_CS(x, y) { const unsigned lo_ = min(x, y), hi_ = max(x, y); x = lo_; y = hi_; }

// ---- tile ---------------------------------------------------------------------------------------------------------------
// k_rows_tile's staging, restated (sharing one function changed that kernel's register allocation, which stays as it was: DESIGN.md 4.16).
// A tile of nr <= 64 consecutive rows (n = nr * len values at src) goes HBM -> registers -> LDS as keys at the odd row pitch len | 1, by
// the 64 lanes of one wave: 16-byte loads when vec_ok (the array is 16-byte aligned, and a tile starts 256 * len bytes behind it), 4-byte
// loads otherwise and for the rest of a partial tile.  `magic` = 2^32 / len + 1: idx / len == umulhi(idx, magic) for idx < 64 * 160.
__device__ __forceinline__ void rq_stage_tile(unsigned* keys, const float* __restrict__ src, int n, int len, unsigned magic, int vec_ok, int lane) {
    const int pitch = len | 1;
    auto put = [&](int idx, float v) {
        const int r = len == 1 ? idx : (int)__umulhi((unsigned)idx, magic);
        keys[r * pitch + (idx - r * len)] = rs_key(v);
    };
    if(vec_ok) {
        const float4* src4 = reinterpret_cast<const float4*>(src);
        const int n4 = n >> 2;
        for(int i = lane; i < n4; i += 64) {
            const float4 v = src4[i];
            put(4 * i, v.x); put(4 * i + 1, v.y); put(4 * i + 2, v.z); put(4 * i + 3, v.w);
        }
        for(int idx = 4 * n4 + lane; idx < n; idx += 64) put(idx, src[idx]);
    }
    else
        for(int idx = lane; idx < n; idx += 64) put(idx, src[idx]);
}

// The normalised bitonic network on one lane-private row of LDS.  Stage k (2, 4, ... P) merges sorted blocks of k / 2: a flip step
// (i with k - 1 - i inside every block of k) and then half-cleaners at the distances k / 4 ... 1 (i with i + j).  Returns N.
__device__ __forceinline__ int rq_lane_sort(unsigned* row, const int len) {
    auto ld = [&](int i) { return i < len ? row[i] : RS_INV; };   // (i is the same in every lane: a scalar branch)
    auto st = [&](int i, unsigned v) { if(i < len) row[i] = v; };
    int N = 0;
    // stages 2, 4 and 8 on eight registers
    for(int b = 0; b < len; b += 8) {
        unsigned e0 = ld(b), e1 = ld(b + 1), e2 = ld(b + 2), e3 = ld(b + 3), e4 = ld(b + 4), e5 = ld(b + 5), e6 = ld(b + 6), e7 = ld(b + 7);
        N += (e0 != RS_INV) + (e1 != RS_INV) + (e2 != RS_INV) + (e3 != RS_INV) + (e4 != RS_INV) + (e5 != RS_INV) + (e6 != RS_INV) + (e7 != RS_INV);
        RQ_CS(e0, e1) RQ_CS(e2, e3) RQ_CS(e4, e5) RQ_CS(e6, e7)
        RQ_CS(e0, e3) RQ_CS(e1, e2) RQ_CS(e4, e7) RQ_CS(e5, e6)
        RQ_CS(e0, e1) RQ_CS(e2, e3) RQ_CS(e4, e5) RQ_CS(e6, e7)
        RQ_CS(e0, e7) RQ_CS(e1, e6) RQ_CS(e2, e5) RQ_CS(e3, e4)
        RQ_CS(e0, e2) RQ_CS(e1, e3) RQ_CS(e4, e6) RQ_CS(e5, e7)
        RQ_CS(e0, e1) RQ_CS(e2, e3) RQ_CS(e4, e5) RQ_CS(e6, e7)
        st(b, e0); st(b + 1, e1); st(b + 2, e2); st(b + 3, e3); st(b + 4, e4); st(b + 5, e5); st(b + 6, e6); st(b + 7, e7);
    }
    for(int k = 16; (k >> 1) < len; k <<= 1) {
        // the flip step fused with the half-cleaner at k / 4: the keys o, o + h, k - 1 - o - h, k - 1 - o of every block of k (h = k / 4)
        const int h = k >> 2;
        for(int base = 0; base < len; base += k)
            for(int o = 0; o < h && base + o < len; o++) {
                const int i0 = base + o, i1 = i0 + h, i3 = base + k - 1 - o, i2 = i3 - h;
                unsigned a = ld(i0), b = ld(i1), c = ld(i2), d = ld(i3);
                RQ_CS(a, d) RQ_CS(b, c)
                RQ_CS(a, b) RQ_CS(c, d)
                st(i0, a); st(i1, b); st(i2, c); st(i3, d);
            }
        // the half-cleaners at k / 8 ... 1, two at a time: the keys i, i + g, i + 2 g, i + 3 g (g = j / 2) take the steps j and g
        int j = k >> 3;
        for(; j >= 2; j >>= 2) {
            const int g = j >> 1;
            for(int base = 0; base < len; base += 2 * j)
                for(int o = 0; o < g && base + o < len; o++) {
                    const int i0 = base + o;
                    unsigned a = ld(i0), b = ld(i0 + g), c = ld(i0 + 2 * g), d = ld(i0 + 3 * g);
                    RQ_CS(a, c) RQ_CS(b, d)
                    RQ_CS(a, b) RQ_CS(c, d)
                    st(i0, a); st(i0 + g, b); st(i0 + 2 * g, c); st(i0 + 3 * g, d);
                }
        }
        if(j == 1)   // an odd number of half-cleaners: the last one alone
            for(int i = 0; i + 1 < len; i += 2) {
                unsigned a = row[i], b = row[i + 1];
                RQ_CS(a, b)
                row[i] = a; row[i + 1] = b;
            }
    }
    return N;
}

// One wave per workgroup and one workgroup per tile of 64 rows (the host launches it so; the loop strides only beyond 2^20 tiles).  LDS: 64 rows of keys at pitch len | 1, then 64 rows of `qc` results at pitch
// qc | 1.  magic / qmagic / tmagic: 2^32 / d + 1 for d = len, qc and the size of the last chunk of levels (rq_stage_tile).
__global__ __launch_bounds__(64) void k_rowsq_tile(const float* __restrict__ in, long rows, int len, unsigned magic, int vec_ok,
                                                   const float* __restrict__ levels, int nq, int qc, unsigned qmagic, unsigned tmagic, int ends,
                                                   float* __restrict__ out) {
    extern __shared__ unsigned rq_lds[];
    const int lane = threadIdx.x;
    const int pitch = len | 1, qpitch = qc | 1;
    unsigned* row = rq_lds + lane * pitch;
    float* stage = reinterpret_cast<float*>(rq_lds + 64 * pitch);
    const long ntiles = (rows + 63) / 64;
    for(long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long row0 = tile * 64;
        const int nr = (int)min(64L, rows - row0);
        __syncthreads();   // the previous tile's picks are over
        rq_stage_tile(rq_lds, in + row0 * len, nr * len, len, magic, vec_ok, lane);
        __syncthreads();
        int N = 0;
        float mn = NAN, mx = NAN;
        if(lane < nr) {
            if(ends) {   // row_statistic's Min / Max in the original order: the first valid value, replaced on a strict compare only
                bool have = false;
                for(int i = 0; i < len; i++) {
                    const unsigned k = row[i];
                    if(k == RS_INV) continue;
                    const float v = ord2f(k);
                    if(!have) { mn = v; mx = v; have = true; }
                    else { if(v < mn) mn = v; if(v > mx) mx = v; }
                }
            }
            N = rq_lane_sort(row, len);
        }
        for(int j0 = 0; j0 < nq; j0 += qc) {
            const int c = min(qc, nq - j0);
            const unsigned cm = c == qc ? qmagic : tmagic;
            __syncthreads();   // the previous chunk has left the staging area
            if(lane < nr)
                for(int jj = 0; jj < c; jj++) stage[lane * qpitch + jj] = rq_pick(row, N, levels[j0 + jj], mn, mx);
            __syncthreads();
            float* dst = out + row0 * nq + j0;
            for(int idx = lane; idx < nr * c; idx += 64) {   // c == nq: one contiguous block; otherwise runs of c floats
                const int r = c == 1 ? idx : (int)__umulhi((unsigned)idx, cm);
                const int jj = idx - r * c;
                dst[(long)r * nq + jj] = stage[r * qpitch + jj];
            }
        }
    }
}

// ---- block --------------------------------------------------------------------------------------------------------------
// One workgroup per row (the host launches it so; the loop strides only beyond 2^20 rows).  LDS: len keys.  P: the power of two the network runs over (slots from len on are virtual).
__global__ __launch_bounds__(256) void k_rowsq_block(const float* __restrict__ in, long rows, int len, int P, const float* __restrict__ levels, int nq,
                                                     int ends, float* __restrict__ out) {
    extern __shared__ unsigned rq_lds[];
    __shared__ unsigned long long s_ends[2];
    const int tid = threadIdx.x;
    const int half = P >> 1;
    for(long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* src = in + r * len;
        __syncthreads();   // the previous row's picks are over
        if(tid == 0) { s_ends[0] = ~0ull; s_ends[1] = 0ull; }
        for(int i = tid; i < len; i += 256) rq_lds[i] = rs_key(src[i]);
        __syncthreads();
        float mn = NAN, mx = NAN;
        if(ends) {   // positional Min / Max as reductions on (key with the zeros merged, index): the lowest index wins among equals
            unsigned long long a = ~0ull, b = 0ull;
            for(int i = tid; i < len; i += 256) {
                const unsigned k = rq_lds[i];
                if(k == RS_INV) continue;
                const unsigned long long hi = (unsigned long long)rs_canon(k) << 32;
                a = min(a, hi | (unsigned)i); b = max(b, hi | (0xFFFFFFFFu - (unsigned)i));
            }
            if(a != ~0ull) { atomicMin(&s_ends[0], a); atomicMax(&s_ends[1], b); }
            __syncthreads();
            if(s_ends[0] != ~0ull) {   // (the same for every thread; both indices are below len)
                mn = ord2f(rq_lds[(unsigned)(s_ends[0] & 0xFFFFFFFFull)]);
                mx = ord2f(rq_lds[0xFFFFFFFFu - (unsigned)(s_ends[1] & 0xFFFFFFFFull)]);
            }
            __syncthreads();
        }
        for(int k = 2; k <= P; k <<= 1) {
            for(int t = tid; t < half; t += 256) {   // flip: o with k - 1 - o inside every block of k (comparator t: block t / (k / 2))
                const int o = t & ((k >> 1) - 1), base = (t - o) << 1;
                const int i = base + o, p = base + k - 1 - o;
                if(p < len) { const unsigned x = rq_lds[i], y = rq_lds[p]; rq_lds[i] = min(x, y); rq_lds[p] = max(x, y); }
            }
            __syncthreads();
            for(int j = k >> 2; j >= 1; j >>= 1) {
                for(int t = tid; t < half; t += 256) {   // half-cleaner: i with i + j inside every block of 2 j
                    const int o = t & (j - 1);
                    const int i = ((t - o) << 1) + o, p = i + j;
                    if(p < len) { const unsigned x = rq_lds[i], y = rq_lds[p]; rq_lds[i] = min(x, y); rq_lds[p] = max(x, y); }
                }
                __syncthreads();
            }
        }
        int lo = 0, hi = len;   // N: the first RS_INV of the sorted row (every thread reads the same words)
        while(lo < hi) {
            const int mid = (lo + hi) >> 1;
            if(rq_lds[mid] != RS_INV) lo = mid + 1; else hi = mid;
        }
        float* dst = out + r * nq;
        for(int j = tid; j < nq; j += 256) dst[j] = rq_pick(rq_lds, lo, levels[j], mn, mx);
    }
}

// ---- loop ---------------------------------------------------------------------------------------------------------------
__global__ void k_rowsq_scatter(const float* __restrict__ col, long rows, int nq, int j, float* __restrict__ out) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if(r < rows) out[r * nq + j] = col[r];
}

// ---- host ---------------------------------------------------------------------------------------------------------------
namespace gpp {

namespace {
enum RqPath { RQ_LOOP, RQ_TILE, RQ_BLOCK };

RqPath rq_choose(int len, int nq) {
    const bool tile_ok = nq > 1 && len > 0 && len <= RS_TILE_MAXLEN;
    const bool block_ok = nq > 1 && len > RS_TILE_MAXLEN && len <= RQ_BLOCK_MAXLEN;
    if(const char* e = path_env("GPP_ROWS_QUANTILES")) {   // forces a path where its preconditions hold (tests, A/B timings)
        if(!strcmp(e, "loop")) return RQ_LOOP;
        if(!strcmp(e, "tile") && tile_ok) return RQ_TILE;
        if(!strcmp(e, "block") && block_ok) return RQ_BLOCK;
    }
    if(nq >= rq_min_levels(len)) {
        if(tile_ok) return RQ_TILE;
        if(block_ok) return RQ_BLOCK;
    }
    return RQ_LOOP;
}
}   // namespace

void rows_quantiles(const float* d_in, long rows, int len, const float* h_levels, int nq, float* d_out) {
    if(rows <= 0 || nq <= 0) return;
    Staged<float> lv;
    lv.upload(h_levels, (size_t)nq);
    int ends = 0;
    for(int j = 0; j < nq; j++) ends |= h_levels[j] == 0 || h_levels[j] == 1;
    switch(rq_choose(len, nq)) {
    case RQ_TILE: {
        const int qc = std::min(nq, RQ_CHUNK), tail = nq % qc ? nq % qc : qc;
        const size_t lds = ((size_t)64 * (len | 1) + (size_t)64 * (qc | 1)) * sizeof(unsigned);
        // One workgroup per tile (grid-stride only beyond 2^20 tiles): a grid sized to the resident set, as k_rows_tile's is, has to guess how
        // many waves fit a CU, and a guess one too high leaves 256 workgroups to run their share of the tiles alone at the end
        const int vec_ok = (reinterpret_cast<size_t>(d_in) & 15) == 0;
        launch(k_rowsq_tile, grid_capped((rows + 63) / 64, (size_t)1 << 20), 64, lds, d_in, rows, len, magic_div(len), vec_ok, lv.p, nq, qc, magic_div(qc), magic_div(tail), ends, d_out);
        break;
    }
    case RQ_BLOCK: {
        launch(k_rowsq_block, grid_capped(rows, (size_t)1 << 20), 256, (size_t)len * sizeof(unsigned), d_in, rows, len, pow2_at_least(len), lv.p, nq, ends, d_out);
        break;
    }
    default:
        if(nq == 1) { rows_quantile(d_in, rows, len, lv.p, 0, d_out); break; }   // (out is the column)
        Staged<float> col;
        float* d_col = col.get((size_t)rows);
        for(int j = 0; j < nq; j++) {
            rows_quantile(d_in, rows, len, lv.p + j, 0, d_col);
            launch(k_rowsq_scatter, blocks_of(rows), 256, 0, d_col, rows, nq, j, d_out);
        }
    }
}

}   // namespace gpp

// gridpp_amd.calc_quantiles: out[r][j] = calc_quantile(row r, quantiles[j]); the levels are a host array whatever `mem` says
extern "C" int gpp_calc_quantiles(const float* array, long rows, int len, const float* quantiles, int nq, float* out, int mem) {
    GPP_TRY
    if(rows < 0 || len < 0 || nq < 0) invalid("calc_quantiles: negative size");
    if(nq > 0 && !quantiles) invalid("calc_quantiles: quantiles is NULL");
    for(int j = 0; j < nq; j++)
        if(quantiles[j] < 0 || quantiles[j] > 1) invalid("calc_quantiles: Quantiles must be between 0 and 1 inclusive");   // (NaN passes)
    if(rows == 0 || nq == 0) return GPP_OK;
    if(!out || (len > 0 && !array)) invalid("calc_quantiles: array / out is NULL");
    ensure_device();
    InField in;
    OutField o;
    in.bind(array, (size_t)rows * len, mem);
    o.bind(out, (size_t)rows * nq, mem);
    rows_quantiles(in.d, rows, len, quantiles, nq, o.d);
    return finish_call(o);
    GPP_CATCH
}
