// Exact quantiles of the rows of a [rows][len] array on MI355X (gfx950): src/api/util.cpp:111-207 for many rows at once.
//
// A quantile is an order statistic (two of them and a weight), so every path below returns the bits of row_quantile
// (row_stats.h): valid means finite, the order is that of the f2ord keys (-0.0 below +0.0), the weights are
// quantile_from_order's, q == 0 / q == 1 are the positional Min / Max of row_statistic (lowest index among equals).
//
//   tile   len <= 160: one wave per 64 consecutive rows.  The tile goes HBM -> registers -> LDS as KEYS (invalid ->
//          0xFFFFFFFF) at an odd row pitch, then lane l selects within row l: a count walk (N, smallest and largest key),
//          a 4-way search between those two keys (three pivots per walk, 16 walks at most) and one walk for the upper
//          order statistic.  Every walk is conflict-free (odd pitch) and costs one compare per pivot and element.
//   block  one 256-thread workgroup per row, coalesced reads: count pass, then an 8-bit radix select on the keys with the
//          histogram in LDS, starting at the first byte in which the row's smallest and largest key differ.
//   split  few long rows: the same passes with several workgroups per row and the per-row state and histograms in an HBM
//          workspace that k_split_init writes in every call.
//   lane   one lane per row from memory (row_quantile itself): len == 0, and what the others are compared with.
//
// The upper order statistic needs no second selection on any path: with the k-th smallest key known, count(key <= it)
// >= k + 2 means the (k+1)-th is the same value, otherwise it is the smallest key above it -- one more walk.
#include "common.h"
#include <algorithm>
#include "rows_select.h"

#pragma clang fp contract(off)
using namespace gpp;

#include "row_stats.h"

#define RS_SPLIT_MINLEN (1 << 15) // default dispatch: rows at least this long ...
#define RS_SPLIT_MAXROWS 2048     // ... and at most this many of them take several workgroups per row (measured: DESIGN.md 4.14)
// (RS_TILE_MAXLEN, RS_INV, rs_key, rs_indices and rs_canon: rows_select.h, shared with rows_quantiles.hip)

__device__ __forceinline__ float rs_level(const float* __restrict__ q, int qfield, long r) { return q ? (qfield ? q[r] : q[0]) : 0.5f; }

// ---- lane ---------------------------------------------------------------------------------------------------------------
__global__ void k_rows_lane(const float* __restrict__ in, long rows, int len, const float* __restrict__ q, int qfield, float* __restrict__ out) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if(r < rows) out[r] = row_quantile(in + r * len, len, rs_level(q, qfield, r));
}

// ---- tile ---------------------------------------------------------------------------------------------------------------
// selection within one row of keys in LDS, lane-private
__device__ __forceinline__ float rs_lane_select(const unsigned* row, const int len, const float q) {
    int N = 0; unsigned kmin = RS_INV, kmax = 0;
#pragma unroll 4
    for(int i = 0; i < len; i++) {
        const unsigned k = row[i];
        if(k != RS_INV) { N++; kmin = min(kmin, k); kmax = max(kmax, k); }
    }
    if(!dev_valid(q) || N == 0) return NAN;
    if(q == 0 || q == 1) {   // row_statistic's Min / Max: the first valid value, replaced on a strict compare only
        float m = NAN; bool have = false;
        for(int i = 0; i < len; i++) {
            const unsigned k = row[i];
            if(k == RS_INV) continue;
            const float v = ord2f(k);
            if(!have) { m = v; have = true; }
            else if(q == 0 ? v < m : v > m) m = v;
        }
        return m;
    }
    int lo, up;
    rs_indices(q, N, lo, up);
    const int need = lo + 1;
    unsigned a = kmin, b = kmax;   // count(key < a) < need <= count(key <= b); every pivot is below kmax, so no invalid key is counted
    while(a < b) {
        const unsigned span = b - a, p2 = a + (span >> 1), p1 = a + (span >> 2), p3 = p2 + (span >> 2);
        int c1 = 0, c2 = 0, c3 = 0;
#pragma unroll 4
        for(int i = 0; i < len; i++) {
            const unsigned k = row[i];
            c1 += k <= p1 ? 1 : 0; c2 += k <= p2 ? 1 : 0; c3 += k <= p3 ? 1 : 0;
        }
        if(c1 >= need) b = p1;
        else if(c2 >= need) { a = p1 + 1; b = p2; }
        else if(c3 >= need) { a = p2 + 1; b = p3; }
        else a = p3 + 1;
    }
    const float lv = ord2f(a);
    float uv = lv;
    if(up != lo) {
        int cle = 0; unsigned nxt = RS_INV;
#pragma unroll 4
        for(int i = 0; i < len; i++) {
            const unsigned k = row[i];
            if(k <= a) cle++; else nxt = min(nxt, k);
        }
        if(cle < lo + 2) uv = ord2f(nxt);   // (nxt is valid: up <= N - 1, so a key above the lo-th exists)
    }
    return quantile_from_order(q, N, lv, uv, lo, up);
}

// One wave per workgroup, grid-stride over tiles of 64 rows.  `magic` = 2^32 / len + 1: idx / len == umulhi(idx, magic) for idx < 64 * 160.
__global__ __launch_bounds__(64) void k_rows_tile(const float* __restrict__ in, long rows, int len, unsigned magic, int vec_ok,
                                                  const float* __restrict__ q, int qfield, float* __restrict__ out) {
    extern __shared__ unsigned rs_keys[];   // 64 rows at pitch len | 1
    const int lane = threadIdx.x;
    const int pitch = len | 1;
    const long ntiles = (rows + 63) / 64;
    auto put = [&](int idx, float v) {
        const int r = len == 1 ? idx : (int)__umulhi((unsigned)idx, magic);
        rs_keys[r * pitch + (idx - r * len)] = rs_key(v);
    };
    for(long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long row0 = tile * 64;
        const int nr = (int)min(64L, rows - row0);
        const int n = nr * len;
        const float* src = in + row0 * len;
        __syncthreads();   // the previous tile's walks are over
        if(vec_ok) {       // (the base is 16-byte aligned, and a tile starts 256 * len bytes behind it)
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
        __syncthreads();
        if(lane < nr) out[row0 + lane] = rs_lane_select(rs_keys + lane * pitch, len, rs_level(q, qfield, row0 + lane));
    }
}

// ---- the passes of block and split: 256 threads over the elements [i0, i1) of one row ---------------------------------------
// s[0] += valid values, s[1] = min key, s[2] = max key (LDS)
__device__ __forceinline__ void rs_range_count(const float* __restrict__ row, long i0, long i1, int tid, unsigned* s) {
    unsigned n = 0, mn = RS_INV, mx = 0;
#pragma unroll 4
    for(long i = i0 + tid; i < i1; i += 256) {
        const unsigned k = rs_key(row[i]);
        if(k != RS_INV) { n++; mn = min(mn, k); mx = max(mx, k); }
    }
    if(n) { atomicAdd(&s[0], n); atomicMin(&s[1], mn); atomicMax(&s[2], mx); }
}
// hist[digit at `shift`] += 1 for the keys that agree with `prefix` above that digit (hist: 256 words of LDS)
__device__ __forceinline__ void rs_range_hist(const float* __restrict__ row, long i0, long i1, int tid, unsigned prefix, int shift, unsigned* hist) {
    const unsigned himask = shift + 8 >= 32 ? 0u : ~0u << (shift + 8);
#pragma unroll 4
    for(long i = i0 + tid; i < i1; i += 256) {
        const unsigned k = rs_key(row[i]);
        if(k != RS_INV && (k & himask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
}
// *nxt = the smallest valid key above kth (LDS)
__device__ __forceinline__ void rs_range_next(const float* __restrict__ row, long i0, long i1, int tid, unsigned kth, unsigned* nxt) {
    unsigned m = RS_INV;
#pragma unroll 4
    for(long i = i0 + tid; i < i1; i += 256) {
        const unsigned k = rs_key(row[i]);
        if(k > kth) m = min(m, k);
    }
    if(m != RS_INV) atomicMin(nxt, m);
}
// positional Min / Max as a reduction on (value, index): min of key << 32 | i, or max of key << 32 | ~i, with rs_canon's keys (LDS)
__device__ __forceinline__ void rs_range_minmax(const float* __restrict__ row, long i0, long i1, int tid, bool is_min, unsigned long long* packed) {
    unsigned long long m = is_min ? ~0ull : 0ull;
    for(long i = i0 + tid; i < i1; i += 256) {
        const unsigned k = rs_key(row[i]);
        if(k == RS_INV) continue;
        const unsigned long long hi = (unsigned long long)rs_canon(k) << 32;
        if(is_min) m = min(m, hi | (unsigned)i); else m = max(m, hi | (0xFFFFFFFFu - (unsigned)i));
    }
    if(is_min) { if(m != ~0ull) atomicMin(packed, m); }
    else if(m != 0ull) atomicMax(packed, m);
}
__device__ __forceinline__ long rs_packed_index(unsigned long long packed, bool is_min) {
    const unsigned lowbits = (unsigned)(packed & 0xFFFFFFFFull);
    return (long)(is_min ? lowbits : 0xFFFFFFFFu - lowbits);
}
// The digit that holds the need-th smallest (1-based) of the keys counted in hist[0 .. 256), by the 64 lanes of one wave: the one
// lane that finds it returns true with the digit, the number of keys with a smaller digit and the number in the digit's bin.
__device__ __forceinline__ bool rs_pick_digit(const unsigned* hist, unsigned need, int lane, unsigned& d, unsigned& below, unsigned& here) {
    const unsigned b0 = hist[4 * lane], b1 = hist[4 * lane + 1], b2 = hist[4 * lane + 2], b3 = hist[4 * lane + 3];
    const unsigned s4 = b0 + b1 + b2 + b3;
    unsigned incl = s4;
    for(int off = 1; off < 64; off <<= 1) {
        const unsigned t = __shfl_up(incl, off);
        if(lane >= off) incl += t;
    }
    unsigned c = incl - s4;
    if(!(c < need && need <= incl)) return false;
    if(need <= c + b0) { d = 0; here = b0; }
    else {
        c += b0;
        if(need <= c + b1) { d = 1; here = b1; }
        else {
            c += b1;
            if(need <= c + b2) { d = 2; here = b2; }
            else { c += b2; d = 3; here = b3; }
        }
    }
    d += 4 * lane; below = c;
    return true;
}
// the first digit (as a shift) in which the smallest and the largest key of a row differ, and the bits both share above it
__device__ __forceinline__ void rs_first_digit(unsigned kmin, unsigned kmax, int& shift, unsigned& prefix) {
    shift = ((31 - __clz((int)(kmin ^ kmax))) >> 3) << 3;
    prefix = shift + 8 >= 32 ? 0u : kmin & (~0u << (shift + 8));
}

// ---- block --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rows_block(const float* __restrict__ in, long rows, int len, const float* __restrict__ q, int qfield,
                                                    float* __restrict__ out) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s[4];
    __shared__ unsigned long long s64;
    const int tid = threadIdx.x;
    for(long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* row = in + r * len;
        if(tid == 0) { s[0] = 0; s[1] = RS_INV; s[2] = 0; }
        __syncthreads();
        rs_range_count(row, 0, len, tid, s);
        __syncthreads();
        const int N = (int)s[0];
        const unsigned kmin = s[1], kmax = s[2];
        const float qq = rs_level(q, qfield, r);
        __syncthreads();
        float res;   // (every branch below is taken by the whole workgroup: qq, N and the keys are the same for all threads)
        if(!dev_valid(qq) || N == 0) res = NAN;
        else if(qq == 0 || qq == 1) {
            const bool is_min = qq == 0;
            if(tid == 0) s64 = is_min ? ~0ull : 0ull;
            __syncthreads();
            rs_range_minmax(row, 0, len, tid, is_min, &s64);
            __syncthreads();
            res = row[rs_packed_index(s64, is_min)];
        }
        else {
            int lo, up;
            rs_indices(qq, N, lo, up);
            unsigned need = (unsigned)(lo + 1), less = 0, eq = (unsigned)N, prefix = kmin;
            if(kmin != kmax) {
                int shift;
                rs_first_digit(kmin, kmax, shift, prefix);
                for(; shift >= 0; shift -= 8) {
                    hist[tid] = 0;
                    __syncthreads();
                    rs_range_hist(row, 0, len, tid, prefix, shift, hist);
                    __syncthreads();
                    if(tid < 64) {
                        unsigned d, below, here;
                        if(rs_pick_digit(hist, need, tid, d, below, here)) { s[0] = d; s[1] = below; s[2] = here; }
                    }
                    __syncthreads();
                    const unsigned d = s[0], below = s[1];
                    eq = s[2];
                    __syncthreads();
                    need -= below; less += below; prefix |= d << shift;
                }
            }
            const float lv = ord2f(prefix);
            float uv = lv;
            if(up != lo && (int)(less + eq) < lo + 2) {
                if(tid == 0) s[3] = RS_INV;
                __syncthreads();
                rs_range_next(row, 0, len, tid, prefix, &s[3]);
                __syncthreads();
                uv = ord2f(s[3]);
            }
            res = quantile_from_order(qq, N, lv, uv, lo, up);
        }
        if(tid == 0) out[r] = res;
        __syncthreads();
    }
}

// ---- split --------------------------------------------------------------------------------------------------------------
// per-row state in HBM; k_split_init writes every word of it in every call
struct RsSplitRow {
    unsigned N, kmin, kmax, next;
    unsigned prefix, need, less, eq;
    int mode, shift, lo, up;        // mode 0: result written, 1: selection, 2: Min, 3: Max; shift < 0: the lo-th key is `prefix`
    unsigned long long packed;
    float q; unsigned pad;
    unsigned hist[4][256];
};
__device__ __forceinline__ void rs_chunk(int len, long& i0, long& i1) {   // the elements of workgroup blockIdx.x of gridDim.x
    const long per = ((long)len + gridDim.x - 1) / gridDim.x;
    i0 = min((long)len, per * blockIdx.x); i1 = min((long)len, i0 + per);
}
__global__ __launch_bounds__(256) void k_split_init(RsSplitRow* __restrict__ S) {
    RsSplitRow& st = S[blockIdx.x];
    const int tid = threadIdx.x;
    for(int p = 0; p < 4; p++) st.hist[p][tid] = 0;
    if(tid == 0) {
        st.N = 0; st.kmin = RS_INV; st.kmax = 0; st.next = RS_INV;
        st.prefix = 0; st.need = 0; st.less = 0; st.eq = 0;
        st.mode = 0; st.shift = -8; st.lo = 0; st.up = 0;
        st.packed = 0; st.q = NAN; st.pad = 0;
    }
}
__global__ __launch_bounds__(256) void k_split_count(const float* __restrict__ in, int len, RsSplitRow* __restrict__ S) {
    __shared__ unsigned s[3];
    const int tid = threadIdx.x;
    const long r = blockIdx.y;
    if(tid == 0) { s[0] = 0; s[1] = RS_INV; s[2] = 0; }
    __syncthreads();
    long i0, i1;
    rs_chunk(len, i0, i1);
    rs_range_count(in + r * len, i0, i1, tid, s);
    __syncthreads();
    if(tid == 0 && s[0]) { atomicAdd(&S[r].N, s[0]); atomicMin(&S[r].kmin, s[1]); atomicMax(&S[r].kmax, s[2]); }
}
__global__ void k_split_plan(long rows, const float* __restrict__ q, int qfield, RsSplitRow* __restrict__ S, float* __restrict__ out) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if(r >= rows) return;
    RsSplitRow& st = S[r];
    const float qq = rs_level(q, qfield, r);
    const int N = (int)st.N;
    st.q = qq;
    if(!dev_valid(qq) || N == 0) { out[r] = NAN; return; }   // (mode stays 0)
    if(qq == 0 || qq == 1) { st.mode = qq == 0 ? 2 : 3; st.packed = qq == 0 ? ~0ull : 0ull; return; }
    int lo, up;
    rs_indices(qq, N, lo, up);
    st.mode = 1; st.lo = lo; st.up = up;
    st.need = (unsigned)(lo + 1); st.less = 0; st.eq = (unsigned)N;
    if(st.kmin == st.kmax) { st.prefix = st.kmin; st.shift = -8; }
    else {
        int shift; unsigned prefix;
        rs_first_digit(st.kmin, st.kmax, shift, prefix);
        st.prefix = prefix; st.shift = shift;
    }
}
__global__ __launch_bounds__(256) void k_split_hist(const float* __restrict__ in, int len, RsSplitRow* __restrict__ S, int pass) {
    __shared__ unsigned hist[256];
    const int tid = threadIdx.x;
    const long r = blockIdx.y;
    RsSplitRow& st = S[r];
    if(st.mode != 1 || st.shift < 0) return;   // (the same for the whole workgroup)
    hist[tid] = 0;
    __syncthreads();
    long i0, i1;
    rs_chunk(len, i0, i1);
    rs_range_hist(in + r * len, i0, i1, tid, st.prefix, st.shift, hist);
    __syncthreads();
    if(hist[tid]) atomicAdd(&st.hist[pass][tid], hist[tid]);
}
__global__ __launch_bounds__(64) void k_split_pick(RsSplitRow* __restrict__ S, int pass) {
    RsSplitRow& st = S[blockIdx.x];
    const int shift = st.shift;
    const unsigned need = st.need, less = st.less, prefix = st.prefix;
    if(st.mode != 1 || shift < 0) return;
    unsigned d, below, here;
    if(rs_pick_digit(st.hist[pass], need, threadIdx.x, d, below, here)) {
        st.need = need - below; st.less = less + below; st.eq = here;
        st.prefix = prefix | (d << shift); st.shift = shift - 8;
    }
}
__global__ __launch_bounds__(256) void k_split_final(const float* __restrict__ in, int len, RsSplitRow* __restrict__ S) {
    __shared__ unsigned nxt;
    __shared__ unsigned long long s64;
    const int tid = threadIdx.x;
    const long r = blockIdx.y;
    RsSplitRow& st = S[r];
    const int mode = st.mode;
    const bool upper = mode == 1 && st.up != st.lo && (int)(st.less + st.eq) < st.lo + 2;
    if(mode < 2 && !upper) return;
    const bool is_min = mode == 2;
    if(tid == 0) { nxt = RS_INV; s64 = is_min ? ~0ull : 0ull; }
    __syncthreads();
    long i0, i1;
    rs_chunk(len, i0, i1);
    if(upper) rs_range_next(in + r * len, i0, i1, tid, st.prefix, &nxt);
    else rs_range_minmax(in + r * len, i0, i1, tid, is_min, &s64);
    __syncthreads();
    if(tid != 0) return;
    if(upper) { if(nxt != RS_INV) atomicMin(&st.next, nxt); }
    else if(is_min) { if(s64 != ~0ull) atomicMin(&st.packed, s64); }
    else if(s64 != 0ull) atomicMax(&st.packed, s64);
}
__global__ void k_split_finish(const float* __restrict__ in, long rows, int len, const RsSplitRow* __restrict__ S, float* __restrict__ out) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if(r >= rows) return;
    const RsSplitRow& st = S[r];
    if(st.mode == 0) return;
    if(st.mode >= 2) { out[r] = in[r * len + rs_packed_index(st.packed, st.mode == 2)]; return; }
    const float lv = ord2f(st.prefix);
    float uv = lv;
    if(st.up != st.lo && (int)(st.less + st.eq) < st.lo + 2) uv = ord2f(st.next);
    out[r] = quantile_from_order(st.q, (int)st.N, lv, uv, st.lo, st.up);
}

__global__ void k_quantile_range(const float* __restrict__ q, long nq, int* __restrict__ flag) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if(i < nq && (q[i] < 0 || q[i] > 1)) *flag = 1;   // util.cpp:113-115 (NaN passes)
}

// ---- host ---------------------------------------------------------------------------------------------------------------
namespace gpp {

namespace {
enum RsPath { RS_LANE, RS_TILE, RS_BLOCK, RS_SPLIT };

RsPath rs_choose(long rows, int len) {
    const bool tile_ok = len > 0 && len <= RS_TILE_MAXLEN;
    const bool block_ok = len > 0;
    const bool split_ok = len > 0 && rows <= 65535;   // (rows are the grid's y dimension)
    if(const char* e = path_env("GPP_ROWS_SELECT")) {   // forces a path where its preconditions hold (tests, A/B timings)
        if(!strcmp(e, "lane")) return RS_LANE;
        if(!strcmp(e, "tile") && tile_ok) return RS_TILE;
        if(!strcmp(e, "block") && block_ok) return RS_BLOCK;
        if(!strcmp(e, "split") && split_ok) return RS_SPLIT;
    }
    if(len <= 0) return RS_LANE;
    if(tile_ok) return RS_TILE;
    if(split_ok && rows <= RS_SPLIT_MAXROWS && len >= RS_SPLIT_MINLEN) return RS_SPLIT;
    return RS_BLOCK;
}

void rs_split(const float* d_in, long rows, int len, const float* d_q, int q_per_row, float* d_out) {
    Staged<RsSplitRow> ws;   // (returned to the pool at the end of the call: the library's one stream keeps the next borrower behind these kernels)
    RsSplitRow* S = ws.get((size_t)rows);
    // workgroups per row: enough to fill the chip eight times over, at least 4096 elements each
    const long want = std::max<long>(1, 2048 / rows), most = std::max<long>(1, ((long)len + 4095) / 4096);
    const dim3 grid((unsigned)std::min(want, most), (unsigned)rows), rowgrid((unsigned)((rows + 63) / 64));
    launch(k_split_init, (unsigned)rows, 256, 0, S);
    launch(k_split_count, grid, 256, 0, d_in, len, S);
    launch(k_split_plan, rowgrid, 64, 0, rows, d_q, q_per_row, S, d_out);
    for(int pass = 0; pass < 4; pass++) {
        launch(k_split_hist, grid, 256, 0, d_in, len, S, pass);
        launch(k_split_pick, (unsigned)rows, 64, 0, S, pass);
    }
    launch(k_split_final, grid, 256, 0, d_in, len, S);
    launch(k_split_finish, rowgrid, 64, 0, d_in, rows, len, S, d_out);
}
}   // namespace

void rows_quantile(const float* d_in, long rows, int len, const float* d_q, int q_per_row, float* d_out) {
    if(rows <= 0) return;
    switch(rs_choose(rows, len)) {
    case RS_TILE: {
        const size_t lds = (size_t)64 * (len | 1) * sizeof(unsigned);
        const long waves_per_cu = std::max<long>(1, std::min<long>(16, (160 * 1024) / (long)lds));
        const int vec_ok = (reinterpret_cast<size_t>(d_in) & 15) == 0;
        launch(k_rows_tile, grid_capped((rows + 63) / 64, 256 * waves_per_cu), 64, lds, d_in, rows, len, magic_div(len), vec_ok, d_q, q_per_row, d_out);
        break;
    }
    case RS_BLOCK:
        launch(k_rows_block, grid_capped(rows, 256 * 8), 256, 0, d_in, rows, len, d_q, q_per_row, d_out);
        break;
    case RS_SPLIT:
        rs_split(d_in, rows, len, d_q, q_per_row, d_out);
        break;
    default:
        launch(k_rows_lane, blocks_of(rows), 256, 0, d_in, rows, len, d_q, q_per_row, d_out);
    }
}

bool quantile_out_of_range(const float* d_q, long nq) {
    if(nq <= 0) return false;
    Staged<int> flag;
    int* d_flag = flag.get(1);
    int h = 0;
    GPP_HIP(hipMemsetAsync(d_flag, 0, sizeof(int), stream()));
    launch(k_quantile_range, blocks_of(nq), 256, 0, d_q, nq, d_flag);
    GPP_HIP(hipMemcpyAsync(&h, d_flag, sizeof(int), hipMemcpyDeviceToHost, stream()));
    GPP_HIP(hipStreamSynchronize(stream()));
    return h != 0;
}

}   // namespace gpp
