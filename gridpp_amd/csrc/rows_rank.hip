// The rank of every value within its row of a [rows][len] array on MI355X (gfx950), and what follows from it: gpp_calc_ranks (ranks and / or
// the sorted rows), gpp_reorder_by_ranks (ensemble copula coupling: the sorted `values` handed out by the ranks of a template) and
// gpp_calc_crps (the rank form of the CRPS of an ensemble).  DESIGN.md 4.18.
//
// Order: valid means finite (rows_select.h); valid values compare numerically, so -0.0 == +0.0 (rs_canon merges their keys), and equal values
// are ordered by position, lower index first -- numpy.argsort(kind="stable") on the valid values of a row.  rank[i] = -1 for an invalid value;
// sorted[rank[i]] = a[i] with the bits of a[i], NaN from N (the number of valid values) on.
//
//   tile   0 < len <= 160: one wave per 64 consecutive rows, staged as keys at the odd pitch len | 1 (rq_stage_tile of rows_quantiles.hip,
//          restated).  Lane l owns row l and COUNTS ranks: eight keys a_i in registers per sweep over the row, rank[i] = #{j : a_j before a_i}.
//          No sort, no index payload, len * len / 8 LDS reads; the element indices are the same in every lane (conflict-free at the odd pitch).
//          Every output derives from the ranks: the sorted row is the scatter sorted[rank[i]] = a[i], kept in LDS as one BYTE per slot (the
//          position that goes there) and resolved when the tile leaves; the reorder holds the values' slots and the template's ranks of the
//          same tile in LDS together, as bytes again; the CRPS is two sums in double.  Results leave coalesced.
//   block  160 < len <= 8192: one 256-thread workgroup per row.  (canonical key << 32 | position) sorted in LDS by the normalised bitonic
//          network of k_rowsq_block -- the composite keys are distinct, so the network's order IS the stable order; then rank[position] = slot.
//          Where no rank is asked for (sort_rows, the values of a reorder, the CRPS) the 32-bit keys alone are sorted, half the LDS traffic.
//   long   any len: rocprim::segmented_radix_sort_pairs on (canonical key, position), stable by construction; ranks are the scatter of the
//          sorted positions.  Keeps "rows of any length and any number"; no speed is claimed for it.
#include "common.h"
#include <algorithm>
#include <rocprim/rocprim.hpp>
#include "rows_select.h"

#pragma clang fp contract(off)
using namespace gpp;

#define RR_BLOCK_MAXLEN 8192   // block: 8 bytes of LDS per value, 64 KB at most
#define RR_LONG_CHUNK (1L << 27)   // long, and the scratch rows of the block reorder: values per pass (the segmented sort takes 32-bit sizes)
typedef unsigned long long rr_u64;

extern __shared__ __align__(16) unsigned rr_lds[];

// ---- tile ---------------------------------------------------------------------------------------------------------------
// rq_stage_tile, restated (sharing one function changes the register allocation of the kernels of rows_quantiles.hip: DESIGN.md 4.16).  A
// tile of nr <= 64 consecutive rows (n = nr * len values at src) goes HBM -> registers -> LDS as keys at the odd row pitch len | 1, by the 64
// lanes of one wave: 16-byte loads when vec_ok, 4-byte loads otherwise and for the rest of a partial tile.  `magic` = 2^32 / len + 1:
// idx / len == umulhi(idx, magic) for idx < 64 * 160.
__device__ __forceinline__ void rr_stage_tile(unsigned* keys, const float* __restrict__ src, int n, int len, unsigned magic, int vec_ok, int lane) {
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
// What a lane knows about its row leaves the tile through BYTES: a rank or a position within a row of up to 160 values fits one, 0xFF
// stands for "none" (rank -1, an empty slot), and an area of 64 rows of bytes is a quarter of an area of words -- which is what lets three
// waves share a CU at len = 160.  Rows of bytes lie at the pitch rr_bpitch: a multiple of 4 with an odd number of words.
#define RR_NONE 0xFFu
__device__ __forceinline__ int rr_bpitch(int len) { return 4 * (((len + 3) >> 2) | 1); }
__device__ __forceinline__ void rr_fill_none(unsigned char* brow, int len) {   // a lane-private row of bytes, all "none"
    unsigned* w = reinterpret_cast<unsigned*>(brow);
    for(int i = 0; i < rr_bpitch(len) / 4; i++) w[i] = 0xFFFFFFFFu;
}
// flush(idx, r, c) for every element idx = r * len + c of a tile of nr rows, consecutive lanes on consecutive elements
template <class Flush>
__device__ __forceinline__ void rr_flush_tile(int nr, int len, unsigned magic, int lane, Flush&& flush) {
    for(int idx = lane; idx < nr * len; idx += 64) {
        const int r = len == 1 ? idx : (int)__umulhi((unsigned)idx, magic);
        flush(idx, r, idx - r * len);
    }
}

// The ranks of a lane-private row of keys by counting, eight elements per sweep: emit(i, rank) once for every i < len in ascending order of
// i, rank = -1 for an invalid key.  A key a_j counts for a_i when it is smaller, or equal and j < i: `<=` before the eight, `<` behind them,
// and inside them whichever their positions say (all of it decided at compile time or by scalar loop bounds).  An invalid a_j (RS_INV, the
// largest key) never counts for a valid a_i; slots from len on read as RS_INV.
template <class Emit>
__device__ __forceinline__ void rr_lane_ranks(const unsigned* row, const int len, Emit&& emit) {
    for(int b = 0; b < len; b += 8) {
        unsigned c[8];
        int cnt[8];
#pragma unroll
        for(int k = 0; k < 8; k++) { c[k] = b + k < len ? rs_canon(row[b + k]) : RS_INV; cnt[k] = 0; }
        for(int j = 0; j < b; j++) {
            const unsigned cj = rs_canon(row[j]);
#pragma unroll
            for(int k = 0; k < 8; k++) cnt[k] += cj <= c[k];
        }
#pragma unroll
        for(int jj = 0; jj < 8; jj++)
#pragma unroll
            for(int k = 0; k < 8; k++) cnt[k] += jj < k ? c[jj] <= c[k] : c[jj] < c[k];
        for(int j = b + 8; j < len; j++) {
            const unsigned cj = rs_canon(row[j]);
#pragma unroll
            for(int k = 0; k < 8; k++) cnt[k] += cj < c[k];
        }
#pragma unroll
        for(int k = 0; k < 8; k++)
            if(b + k < len) emit(b + k, c[k] == RS_INV ? -1 : cnt[k]);
    }
}
// One wave per workgroup and one workgroup per tile of 64 rows (the loop strides only beyond 2^20 tiles).  LDS: 64 rows of keys at the pitch
// len | 1, then one area of bytes per output: rank[i] for the ranks, and for the sorted rows the inverse, slot -> position, so that the
// flush gathers sorted[slot] = the key at that position (its bits) and writes NaN where no position was entered (the slots from N on).
__global__ __launch_bounds__(64) void k_rank_tile(const float* __restrict__ in, long rows, int len, unsigned magic, int vec_ok, int* __restrict__ ranks,
                                                  float* __restrict__ sorted) {
    const int lane = threadIdx.x;
    const int pitch = len | 1, bp = rr_bpitch(len);
    unsigned* keys = rr_lds;
    unsigned char* rk = reinterpret_cast<unsigned char*>(rr_lds + 64 * pitch);
    unsigned char* inv = rk + (ranks ? 64 * bp : 0);
    const long ntiles = (rows + 63) / 64;
    for(long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long row0 = tile * 64;
        const int nr = (int)min(64L, rows - row0);
        __syncthreads();   // the previous tile has left LDS
        rr_stage_tile(keys, in + row0 * len, nr * len, len, magic, vec_ok, lane);
        __syncthreads();
        if(lane < nr) {
            if(sorted) rr_fill_none(inv + lane * bp, len);
            rr_lane_ranks(keys + lane * pitch, len, [&](int i, int r) {
                if(ranks) rk[lane * bp + i] = (unsigned char)r;   // (-1 -> RR_NONE)
                if(sorted && r >= 0) inv[lane * bp + r] = (unsigned char)i;   // (r < len)
            });
        }
        __syncthreads();
        if(ranks)
            rr_flush_tile(nr, len, magic, lane, [&](int idx, int r, int c) {
                const unsigned b = rk[r * bp + c];
                ranks[row0 * len + idx] = b == RR_NONE ? -1 : (int)b;
            });
        if(sorted)
            rr_flush_tile(nr, len, magic, lane, [&](int idx, int r, int c) {
                const unsigned b = inv[r * bp + c];
                sorted[row0 * len + idx] = b == RR_NONE ? NAN : ord2f(keys[r * pitch + b]);   // (b: a position of the row, below len)
            });
    }
}

// out[i] = sorted(values)[rank of templ[i]].  LDS: the keys of `values`, replaced by the template's once the values' inverse (slot -> position)
// stands in bytes; then per element of the template the position in `values` it receives (RR_NONE: its rank is -1 or not below Nv), and the
// flush gathers those values from HBM, where the tile has just been read.
__global__ __launch_bounds__(64) void k_reorder_tile(const float* __restrict__ values, const float* __restrict__ templ, long rows, int len, unsigned magic,
                                                     int vec_ok, float* __restrict__ out) {
    const int lane = threadIdx.x;
    const int pitch = len | 1, bp = rr_bpitch(len);
    unsigned* keys = rr_lds;
    unsigned char* inv = reinterpret_cast<unsigned char*>(rr_lds + 64 * pitch);
    unsigned char* from = inv + 64 * bp;
    const long ntiles = (rows + 63) / 64;
    for(long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long row0 = tile * 64;
        const int nr = (int)min(64L, rows - row0);
        __syncthreads();
        rr_stage_tile(keys, values + row0 * len, nr * len, len, magic, vec_ok, lane);
        __syncthreads();
        if(lane < nr) {
            rr_fill_none(inv + lane * bp, len);
            rr_lane_ranks(keys + lane * pitch, len, [&](int i, int r) { if(r >= 0) inv[lane * bp + r] = (unsigned char)i; });
        }
        __syncthreads();   // every lane is through with the keys of `values`
        rr_stage_tile(keys, templ + row0 * len, nr * len, len, magic, vec_ok, lane);
        __syncthreads();
        if(lane < nr)
            rr_lane_ranks(keys + lane * pitch, len, [&](int i, int r) { from[lane * bp + i] = r >= 0 ? inv[lane * bp + r] : (unsigned char)RR_NONE; });
        __syncthreads();
        rr_flush_tile(nr, len, magic, lane, [&](int idx, int r, int c) {
            const unsigned b = from[r * bp + c];
            out[row0 * len + idx] = b == RR_NONE ? NAN : values[(row0 + r) * len + b];   // (b: a position of the row, below len)
        });
    }
}

// CRPS = (1 / N) sum |x_i - y| - (1 / N^2) sum (2 r_i - N + 1) x_i, both sums in double in the order of the row
__global__ __launch_bounds__(64) void k_crps_tile(const float* __restrict__ in, const float* __restrict__ ref, long rows, int len, unsigned magic,
                                                  int vec_ok, float* __restrict__ out) {
    const int lane = threadIdx.x;
    const int pitch = len | 1;
    const long ntiles = (rows + 63) / 64;
    for(long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long row0 = tile * 64;
        const int nr = (int)min(64L, rows - row0);
        __syncthreads();
        rr_stage_tile(rr_lds, in + row0 * len, nr * len, len, magic, vec_ok, lane);
        __syncthreads();
        if(lane < nr) {
            const unsigned* row = rr_lds + lane * pitch;
            const float yf = ref[row0 + lane];
            const double y = (double)yf;
            int N = 0;
            for(int i = 0; i < len; i++) N += row[i] != RS_INV;
            double s1 = 0, s2 = 0;
            rr_lane_ranks(row, len, [&](int i, int r) {
                if(r < 0) return;
                const double x = (double)ord2f(row[i]);
                s1 += fabs(x - y);
                s2 += (double)(2 * r - N + 1) * x;
            });
            out[row0 + lane] = N == 0 || !dev_valid(yf) ? NAN : (float)(s1 / (double)N - s2 / ((double)N * (double)N));
        }
    }
}

// ---- block --------------------------------------------------------------------------------------------------------------
// k_rowsq_block's network on the len words (32 or 64 bits) of one row in LDS.  P: the power of two the network runs over; the slots from len
// on are virtual words larger than any real one.  The caller has written the words; ends with a barrier.
template <class T>
__device__ __forceinline__ void rr_block_sort(T* w, int len, int P, int tid) {
    __syncthreads();
    const int half = P >> 1;
    for(int k = 2; k <= P; k <<= 1) {
        for(int t = tid; t < half; t += 256) {   // flip: o with k - 1 - o inside every block of k
            const int o = t & ((k >> 1) - 1), base = (t - o) << 1;
            const int i = base + o, p = base + k - 1 - o;
            if(p < len) { const T x = w[i], y = w[p]; w[i] = min(x, y); w[p] = max(x, y); }
        }
        __syncthreads();
        for(int j = k >> 2; j >= 1; j >>= 1) {
            for(int t = tid; t < half; t += 256) {   // half-cleaner: i with i + j inside every block of 2 j
                const int o = t & (j - 1);
                const int i = ((t - o) << 1) + o, p = i + j;
                if(p < len) { const T x = w[i], y = w[p]; w[i] = min(x, y); w[p] = max(x, y); }
            }
            __syncthreads();
        }
    }
}
// the first slot of a sorted row of 32-bit keys that holds a key >= k (every thread reads the same words)
__device__ __forceinline__ int rr_lower_bound(const unsigned* w, int len, unsigned k) {
    int lo = 0, hi = len;
    while(lo < hi) {
        const int mid = (lo + hi) >> 1;
        if(w[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One workgroup per row (the loop strides only beyond 2^20 rows).  LDS: len words of 8 bytes, (canonical key << 32 | position): the words
// are distinct, so the network's order is the stable order; an invalid value's word is RS_INV << 32 | position.
// REORDER == 0: ranks[position] = slot (-1 for an invalid value) and, when asked for, sorted[slot] = the value at that position (NaN from N on).
// REORDER == 1: `in` is the template and `aux` the sorted `values` rows (NaN from their Nv on): out[position] = aux[slot], NaN for an invalid value.
template <int REORDER>
__global__ __launch_bounds__(256) void k_rank_block(const float* __restrict__ in, const float* __restrict__ aux, long rows, int len, int P,
                                                    int* __restrict__ ranks, float* __restrict__ out) {
    rr_u64* w = reinterpret_cast<rr_u64*>(rr_lds);
    const int tid = threadIdx.x;
    for(long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* src = in + r * len;
        __syncthreads();   // the previous row has left LDS
        for(int i = tid; i < len; i += 256) w[i] = ((rr_u64)rs_canon(rs_key(src[i])) << 32) | (unsigned)i;
        rr_block_sort(w, len, P, tid);
        for(int p = tid; p < len; p += 256) {
            const rr_u64 e = w[p];
            const unsigned i = (unsigned)(e & 0xFFFFFFFFull);   // (a position of this row: below len)
            const bool valid = (unsigned)(e >> 32) != RS_INV;
            if(REORDER) out[r * len + i] = valid ? aux[r * len + p] : NAN;
            else {
                if(ranks) ranks[r * len + i] = valid ? p : -1;
                if(out) out[r * len + p] = valid ? src[i] : NAN;
            }
        }
    }
}
// The sorted rows alone: the row's 32-bit keys (rs_key: -0.0 below +0.0) sorted in LDS, half the words of k_rank_block.  Equal values carry
// equal bits, so their order shows only where a row holds zeros of BOTH signs: there the run of zeros is written again in the order of the
// row (one wave walks the row, 64 values a step).
__global__ __launch_bounds__(256) void k_sort_block(const float* __restrict__ in, long rows, int len, int P, float* __restrict__ out) {
    unsigned* w = rr_lds;
    const int tid = threadIdx.x;
    for(long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* src = in + r * len;
        __syncthreads();   // the previous row has left LDS
        for(int i = tid; i < len; i += 256) w[i] = rs_key(src[i]);
        rr_block_sort(w, len, P, tid);
        const int z0 = rr_lower_bound(w, len, 0x7FFFFFFFu), z1 = rr_lower_bound(w, len, 0x80000000u), z2 = rr_lower_bound(w, len, 0x80000001u);
        if(z1 > z0 && z2 > z1) {   // (the same for every thread)
            __syncthreads();       // every thread has its three bounds
            if(tid < 64) {
                int c = z0;
                for(int base = 0; base < len; base += 64) {
                    const int i = base + tid;
                    const float v = i < len ? src[i] : 1.0f;
                    const unsigned long long m = __ballot(v == 0.0f);
                    if(v == 0.0f) w[c + __popcll(m & ((1ull << tid) - 1ull))] = rs_key(v);   // (c + ... < z2: the row holds z2 - z0 zeros)
                    c += __popcll(m);
                }
            }
            __syncthreads();
        }
        for(int p = tid; p < len; p += 256) {
            const unsigned k = w[p];
            out[r * len + p] = k != RS_INV ? ord2f(k) : NAN;
        }
    }
}
// the CRPS of one row per workgroup from its sorted 32-bit canonical keys (a zero of either sign is 0 in both sums); the four wave sums meet in LDS
__global__ __launch_bounds__(256) void k_crps_block(const float* __restrict__ in, const float* __restrict__ ref, long rows, int len, int P,
                                                    float* __restrict__ out) {
    unsigned* w = rr_lds;
    double* red = reinterpret_cast<double*>(rr_lds);   // (8 doubles: len > 160 words are there)
    const int tid = threadIdx.x;
    for(long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* src = in + r * len;
        __syncthreads();
        for(int i = tid; i < len; i += 256) w[i] = rs_canon(rs_key(src[i]));
        rr_block_sort(w, len, P, tid);
        const int N = rr_lower_bound(w, len, RS_INV);   // the first invalid key of the sorted row
        const float yf = ref[r];
        const double y = (double)yf;
        double s1 = 0, s2 = 0;
        for(int p = tid; p < N; p += 256) {
            const double x = (double)ord2f(w[p]);
            s1 += fabs(x - y);
            s2 += (double)(2 * p - N + 1) * x;
        }
        for(int d = 32; d >= 1; d >>= 1) { s1 += __shfl_down(s1, d, 64); s2 += __shfl_down(s2, d, 64); }
        __syncthreads();   // every thread has read its words
        if((tid & 63) == 0) { red[2 * (tid >> 6)] = s1; red[2 * (tid >> 6) + 1] = s2; }
        __syncthreads();
        if(tid == 0) {
            const double t1 = ((red[0] + red[2]) + red[4]) + red[6], t2 = ((red[1] + red[3]) + red[5]) + red[7];
            out[r] = N == 0 || !dev_valid(yf) ? NAN : (float)(t1 / (double)N - t2 / ((double)N * (double)N));
        }
    }
}

// ---- long ---------------------------------------------------------------------------------------------------------------
__global__ void k_rank_long_keys(const float* __restrict__ in, long n, int len, unsigned* __restrict__ keys, int* __restrict__ pos) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n) return;
    keys[i] = rs_canon(rs_key(in[i]));
    pos[i] = (int)(i % len);
}
// k_rank_block's outputs from the sorted (key, position) pairs of n = rows * len values in HBM
template <int REORDER>
__global__ void k_rank_long_emit(const float* __restrict__ in, const float* __restrict__ aux, const unsigned* __restrict__ skeys,
                                 const int* __restrict__ spos, long n, int len, int* __restrict__ ranks, float* __restrict__ out) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if(g >= n) return;
    const long row = g / len;
    const int p = (int)(g - row * len);
    const long at = row * len + spos[g];   // (a position of this row: 0 <= spos < len)
    const bool valid = skeys[g] != RS_INV;
    if(REORDER) out[at] = valid ? aux[g] : NAN;
    else {
        if(ranks) ranks[at] = valid ? p : -1;
        if(out) out[g] = valid ? in[at] : NAN;
    }
}
// one workgroup per row; len == 0 (no keys at all) gives NaN
__global__ __launch_bounds__(256) void k_crps_long(const unsigned* __restrict__ skeys, const float* __restrict__ ref, long rows, int len,
                                                   float* __restrict__ out) {
    __shared__ double red[8];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    for(long r = blockIdx.x; r < rows; r += gridDim.x) {
        const unsigned* k = skeys + r * len;
        __syncthreads();
        if(tid == 0) s_n = 0;
        __syncthreads();
        int n = 0;
        for(int p = tid; p < len; p += 256) n += k[p] != RS_INV;
        if(n) atomicAdd(&s_n, n);
        __syncthreads();
        const int N = s_n;
        const float yf = ref[r];
        const double y = (double)yf;
        double s1 = 0, s2 = 0;
        for(int p = tid; p < N; p += 256) {   // the valid keys come first
            const double x = (double)ord2f(k[p]);
            s1 += fabs(x - y);
            s2 += (double)(2 * p - N + 1) * x;
        }
        for(int d = 32; d >= 1; d >>= 1) { s1 += __shfl_down(s1, d, 64); s2 += __shfl_down(s2, d, 64); }
        if((tid & 63) == 0) { red[2 * (tid >> 6)] = s1; red[2 * (tid >> 6) + 1] = s2; }
        __syncthreads();
        if(tid == 0) {
            const double t1 = ((red[0] + red[2]) + red[4]) + red[6], t2 = ((red[1] + red[3]) + red[5]) + red[7];
            out[r] = N == 0 || !dev_valid(yf) ? NAN : (float)(t1 / (double)N - t2 / ((double)N * (double)N));
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
namespace gpp {

namespace {
enum RrPath { RR_TILE, RR_BLOCK, RR_LONG };

RrPath rr_choose(int len) {
    const bool tile_ok = len > 0 && len <= RS_TILE_MAXLEN;
    const bool block_ok = len > RS_TILE_MAXLEN && len <= RR_BLOCK_MAXLEN;
    if(const char* e = path_env("GPP_ROWS_RANKS")) {   // forces a path where its preconditions hold (tests, A/B timings)
        if(!strcmp(e, "long")) return RR_LONG;
        if(!strcmp(e, "tile") && tile_ok) return RR_TILE;
        if(!strcmp(e, "block") && block_ok) return RR_BLOCK;
    }
    return tile_ok ? RR_TILE : block_ok ? RR_BLOCK : RR_LONG;
}
constexpr size_t RR_MAXGRID = (size_t)1 << 20;   // the tile and block kernels stride over their grid beyond it
// the keys of a tile and `bytes` areas of bytes (rr_bpitch, restated for the host).  At len = 160 that is 41 216 + 10 496 bytes per area of
// bytes: with two of them 62 208, within the 64 KB a kernel gets unasked
size_t rr_tile_lds(int len, int bytes) { return (size_t)64 * (len | 1) * sizeof(unsigned) + (size_t)bytes * 64 * 4 * (((len + 3) >> 2) | 1); }

struct SegBegin {   // the bounds of the equal segments of the long path
    unsigned len;
    __host__ __device__ unsigned operator()(unsigned i) const { return i * len; }
};
// (canonical key, position) of n = rows * len values at d_in, sorted row by row into skeys / spos
void rr_long_sort(const float* d_in, long rows, int len, unsigned* keys, int* pos, unsigned* skeys, int* spos) {
    const long n = rows * len;
    launch(k_rank_long_keys, blocks_of(n), 256, 0, d_in, n, len, keys, pos);
    auto begin = rocprim::make_transform_iterator(rocprim::counting_iterator<unsigned>(0u), SegBegin{(unsigned)len});
    size_t sb = 0;
    GPP_HIP(rocprim::segmented_radix_sort_pairs((void*)nullptr, sb, keys, skeys, pos, spos, (unsigned)n, (unsigned)rows, begin, begin + 1, 0u, 32u, stream()));
    DevBuf<char> tmp;
    tmp.get(sb);
    GPP_HIP(rocprim::segmented_radix_sort_pairs((void*)tmp.p, sb, keys, skeys, pos, spos, (unsigned)n, (unsigned)rows, begin, begin + 1, 0u, 32u, stream()));
    GPP_HIP(hipStreamSynchronize(stream()));   // `tmp` is released here
}
long rr_chunk_rows(int len) { return std::max<long>(1, RR_LONG_CHUNK / len); }   // (rows * len stays below 2^31: len is an int)
struct LongWs {
    Staged<unsigned> keys, skeys;
    Staged<int> pos, spos;
    void get(size_t n) { keys.get(n); skeys.get(n); pos.get(n); spos.get(n); }
};
}   // namespace

// d_ranks and / or d_sorted (either may be nullptr) of the rows of d_in; launches on the library stream
void rows_ranks(const float* d_in, long rows, int len, int* d_ranks, float* d_sorted) {
    if(rows <= 0 || len <= 0 || (!d_ranks && !d_sorted)) return;
    switch(rr_choose(len)) {
    case RR_TILE: {
        const size_t lds = rr_tile_lds(len, (d_ranks != nullptr) + (d_sorted != nullptr));
        const int vec_ok = (reinterpret_cast<size_t>(d_in) & 15) == 0;
        launch(k_rank_tile, grid_capped((rows + 63) / 64, RR_MAXGRID), 64, lds, d_in, rows, len, magic_div(len), vec_ok, d_ranks, d_sorted);
        break;
    }
    case RR_BLOCK:
        if(d_ranks)
            launch(k_rank_block<0>, grid_capped(rows, RR_MAXGRID), 256, (size_t)len * sizeof(rr_u64), d_in, (const float*)nullptr, rows, len, pow2_at_least(len), d_ranks,
                   d_sorted);
        else   // the sorted rows alone: 32-bit keys
            launch(k_sort_block, grid_capped(rows, RR_MAXGRID), 256, (size_t)len * sizeof(unsigned), d_in, rows, len, pow2_at_least(len), d_sorted);
        break;
    default: {
        LongWs ws;
        const long step = rr_chunk_rows(len);
        ws.get((size_t)(std::min(step, rows) * len));
        for(long r0 = 0; r0 < rows; r0 += step) {
            const long nr = std::min(step, rows - r0), n = nr * len;
            rr_long_sort(d_in + r0 * len, nr, len, ws.keys.p, ws.pos.p, ws.skeys.p, ws.spos.p);
            launch(k_rank_long_emit<0>, blocks_of(n), 256, 0, d_in + r0 * len, (const float*)nullptr, ws.skeys.p, ws.spos.p, n, len, d_ranks ? d_ranks + r0 * len : nullptr,
                   d_sorted ? d_sorted + r0 * len : nullptr);
        }
    }
    }
}

// d_out[r][i] = sorted(d_values row r)[rank of d_templ[r][i]], NaN where the template's value is invalid or its rank reaches past the valid values
void rows_reorder(const float* d_values, const float* d_templ, long rows, int len, float* d_out) {
    if(rows <= 0 || len <= 0) return;
    const RrPath path = rr_choose(len);
    if(path == RR_TILE) {
        const size_t lds = rr_tile_lds(len, 2);
        const int vec_ok = ((reinterpret_cast<size_t>(d_values) | reinterpret_cast<size_t>(d_templ)) & 15) == 0;
        launch(k_reorder_tile, grid_capped((rows + 63) / 64, RR_MAXGRID), 64, lds, d_values, d_templ, rows, len, magic_div(len), vec_ok, d_out);
        return;
    }
    // block and long: the sorted `values` rows go through a scratch array in HBM, a bounded number of rows at a time
    const long step = rr_chunk_rows(len);
    Staged<float> sorted;
    sorted.get((size_t)(std::min(step, rows) * len));
    LongWs ws;
    if(path == RR_LONG) ws.get((size_t)(std::min(step, rows) * len));
    for(long r0 = 0; r0 < rows; r0 += step) {
        const long nr = std::min(step, rows - r0), n = nr * len;
        const float *v = d_values + r0 * len, *t = d_templ + r0 * len;
        if(path == RR_BLOCK) {
            const int P = pow2_at_least(len);
            const size_t lds = (size_t)len * sizeof(rr_u64);
            launch(k_sort_block, grid_capped(nr, RR_MAXGRID), 256, (size_t)len * sizeof(unsigned), v, nr, len, P, sorted.p);
            launch(k_rank_block<1>, grid_capped(nr, RR_MAXGRID), 256, lds, t, (const float*)sorted.p, nr, len, P, (int*)nullptr, d_out + r0 * len);
        }
        else {
            const dim3 grid(blocks_of(n));
            rr_long_sort(v, nr, len, ws.keys.p, ws.pos.p, ws.skeys.p, ws.spos.p);
            launch(k_rank_long_emit<0>, grid, 256, 0, v, (const float*)nullptr, ws.skeys.p, ws.spos.p, n, len, (int*)nullptr, sorted.p);
            rr_long_sort(t, nr, len, ws.keys.p, ws.pos.p, ws.skeys.p, ws.spos.p);
            launch(k_rank_long_emit<1>, grid, 256, 0, t, (const float*)sorted.p, ws.skeys.p, ws.spos.p, n, len, (int*)nullptr, d_out + r0 * len);
        }
    }
}

// d_out[r] = the CRPS of the valid members of row r against d_ref[r]
void rows_crps(const float* d_ens, const float* d_ref, long rows, int len, float* d_out) {
    if(rows <= 0) return;
    if(len <= 0) {   // no member at all: NaN
        launch(k_crps_long, grid_capped(rows, RR_MAXGRID), 256, 0, (const unsigned*)nullptr, d_ref, rows, 0, d_out);
        return;
    }
    switch(rr_choose(len)) {
    case RR_TILE: {
        const size_t lds = rr_tile_lds(len, 0);
        const int vec_ok = (reinterpret_cast<size_t>(d_ens) & 15) == 0;
        launch(k_crps_tile, grid_capped((rows + 63) / 64, RR_MAXGRID), 64, lds, d_ens, d_ref, rows, len, magic_div(len), vec_ok, d_out);
        break;
    }
    case RR_BLOCK:
        launch(k_crps_block, grid_capped(rows, RR_MAXGRID), 256, (size_t)len * sizeof(unsigned), d_ens, d_ref, rows, len, pow2_at_least(len), d_out);
        break;
    default: {
        LongWs ws;
        const long step = rr_chunk_rows(len);
        ws.get((size_t)(std::min(step, rows) * len));
        for(long r0 = 0; r0 < rows; r0 += step) {
            const long nr = std::min(step, rows - r0);
            rr_long_sort(d_ens + r0 * len, nr, len, ws.keys.p, ws.pos.p, ws.skeys.p, ws.spos.p);
            launch(k_crps_long, grid_capped(nr, RR_MAXGRID), 256, 0, (const unsigned*)ws.skeys.p, d_ref + r0, nr, len, d_out + r0);
        }
    }
    }
}

}   // namespace gpp

// gridpp_amd.calc_ranks / sort_rows: both outputs come from one launch, either may be NULL
extern "C" int gpp_calc_ranks(const float* array, long rows, int len, int* ranks, float* sorted, int mem) {
    GPP_TRY
    if(rows < 0 || len < 0) invalid("calc_ranks: negative size");
    if(rows == 0 || len == 0) return GPP_OK;
    if(!array) invalid("calc_ranks: array is NULL");
    if(!ranks && !sorted) invalid("calc_ranks: ranks and sorted are both NULL");
    ensure_device();
    const size_t n = (size_t)rows * len;
    InField in;
    OutInts r;
    OutField s;
    in.bind(array, n, mem);
    r.bind(ranks, n, mem);
    s.bind(sorted, n, mem);
    rows_ranks(in.d, rows, len, r.d, s.d);
    return finish_call(r, s);
    GPP_CATCH
}

// gridpp_amd.reorder_by_ranks
extern "C" int gpp_reorder_by_ranks(const float* values, const float* templ, long rows, int len, float* out, int mem) {
    GPP_TRY
    if(rows < 0 || len < 0) invalid("reorder_by_ranks: negative size");
    if(rows == 0 || len == 0) return GPP_OK;
    if(!values || !templ || !out) invalid("reorder_by_ranks: values / template / out is NULL");
    ensure_device();
    const size_t n = (size_t)rows * len;
    InField v, t;
    OutField o;
    v.bind(values, n, mem);
    t.bind(templ, n, mem);
    o.bind(out, n, mem);
    rows_reorder(v.d, t.d, rows, len, o.d);
    return finish_call(o);
    GPP_CATCH
}

// gridpp_amd.calc_crps
extern "C" int gpp_calc_crps(const float* ensemble, const float* ref, long rows, int len, float* out, int mem) {
    GPP_TRY
    if(rows < 0 || len < 0) invalid("calc_crps: negative size");
    if(rows == 0) return GPP_OK;
    if(!ref || !out || (len > 0 && !ensemble)) invalid("calc_crps: ensemble / ref / out is NULL");
    ensure_device();
    InField e, y;
    OutField o;
    e.bind(len > 0 ? ensemble : nullptr, (size_t)rows * len, mem);
    y.bind(ref, (size_t)rows, mem);
    o.bind(out, (size_t)rows, mem);
    rows_crps(e.d, y.d, rows, len, o.d);
    return finish_call(o);
    GPP_CATCH
}
