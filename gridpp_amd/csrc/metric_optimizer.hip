// gridpp::get_optimal_threshold and gridpp::metric_optimizer_curve (include/gridpp.h, src/api/metric_optimizer.cpp:105-184) for gfx950,
// as the exact optimum over the plateaus of the score function, not as a restatement of Boost's brent_find_minima.
//
// s(x) = calc_score(ref, fcst, threshold, x, metric) changes only where x crosses a value of fcst.  With the pairs sorted by fcst, the
// table at the plateau that begins at the last element i of a run of equal finite values is
//     c = #{ref > t in sorted[0 .. i]},  d = #{ref <= t in sorted[0 .. i]},  a = #{ref > t} - c,  b = #{ref <= t} - d
// so one sort, one scan of the two predicates and one ordered reduction over the plateaus answer every threshold t.  The sort key puts
// NaN first, then -inf, the finite values (-0 as +0), then +inf: NaN and -inf fail `fcst > x` for every finite x and so lie in every
// prefix (c / d), +inf passes it and lies in none (a / b); none of the three defines a plateau.  The work is done once per call:
//
//   k_mo_keys     one thread per element: fcst -> a 32-bit key whose unsigned order is the order above.
//   (rocPRIM)     radix_sort_pairs of (key, ref), all 32 bits.
//   k_mo_totals   workgroup (tile b, group q): the numbers of ref > t and ref <= t in the tile for the MO_G thresholds of group q.
//   k_mo_scan     workgroup (threshold, predicate): exclusive scan of the tile totals in 64 bits, and their sum.  The carry across
//                 workgroups is therefore "block totals, a scan of the totals, a second pass": no workgroup waits for another inside a
//                 launch, the kernel boundaries are the only hand-offs.
//   k_mo_sweep    the hot path.  Workgroup (tile b, group q), MO_THREADS lanes, lane l holds the MO_IPT consecutive sorted elements
//                 l * ipt .. of the tile in registers (ipt = MO_IPT unless the tile is shrunk, below) and MO_G thresholds: the sorted keys
//                 and ref are read once per group of thresholds, not once per threshold.  Per threshold: the lane's own counts, an
//                 exclusive scan of them over the workgroup (shuffles inside a wave, 4 wave totals through LDS), plus the tile's carry;
//                 then the lane walks its elements again, and where key[i] is finite and differs from key[i + 1] it forms the four counts
//                 (64-bit, capped at 2^24 at the conversion to float, as gpp_calc_score does), evaluates gpp_score_value (score.h) and
//                 appends the plateau to a MoRun: first and last plateau with their scores, the largest valid score, the lowest plateau
//                 that attains it, and the first later plateau whose score differs.  mo_combine joins two MoRuns of adjacent stretches;
//                 it is associative, so the lanes' MoRuns are joined in order by shuffles, the 4 waves' through LDS, and one MoRun per
//                 (threshold, tile) goes to HBM.
//   k_mo_finish   one wave per threshold joins the tiles' MoRuns in order, forms the midpoint in double and applies the reference's
//                 filters (metric_optimizer.cpp:165-182 with its constants as floats).
//
// One hipStreamSynchronize per call, after the copy of the T results.  Thresholds are taken MO_BATCH at a time so that the per-tile
// workspace stays small; the sort is shared by all batches.
//
// Budget of k_mo_sweep: MO_G = 4 thresholds per workgroup and MO_IPT = 8 elements per lane: 2 * MO_IPT = 16 registers of elements, per
// threshold a MoRun of 8 words, two 64-bit carries, two 64-bit totals and two counters, 4 * 18 = 72; the build reports 119 vector registers,
// no accumulation registers, no scratch, 4 waves per SIMD.  LDS: 4 waves * (2 * MO_G counters + MO_G MoRuns of 32 bytes) = 640 bytes per
// workgroup.  (16 elements per lane: 184 registers, 2 waves per SIMD, and a million values fill 245 workgroups, fewer than the chip has
// compute units: the sweep of 20 thresholds took 139 us against 101 us with 8 -- DESIGN.md 4.13.)
//
// GPP_MO_TILE (a path override, tests): elements per workgroup, 1 .. MO_THREADS * MO_IPT (2048, the default).  Every lane then holds
// ceil(tile / MO_THREADS) elements, so that small inputs cross many workgroup boundaries -- in the carry, in key[i + 1] and in runs of
// equal scores.  The result does not depend on it.
#include "common.h"
#include "score.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <cstdint>

#pragma clang fp contract(off)

using namespace gpp;

namespace {

constexpr int MO_THREADS = 256;
constexpr int MO_IPT = GPP_MO_TILE_ITEMS / MO_THREADS;   // elements a lane holds
constexpr int MO_G = GPP_MO_GROUP;                       // thresholds a workgroup holds
constexpr int MO_BATCH = 64;                             // thresholds per sequence of launches
constexpr long long MO_MAX_TILES = 1 << 20;
static_assert(GPP_MO_TILE_ITEMS % MO_THREADS == 0 && MO_BATCH % MO_G == 0 && MO_THREADS == 256, "layout");

typedef unsigned long long u64;

// ---- the sort key -------------------------------------------------------------------------------------------------------------------
constexpr unsigned MO_KEY_NEG_INF = 0x007fffffu, MO_KEY_POS_INF = 0xff800000u;   // NaN is 0; finite keys lie strictly between these two
__device__ __forceinline__ unsigned mo_encode(float f) {
    if(isnan(f)) return 0u;
    if(f == 0.0f) f = 0.0f;   // -0 is +0: one plateau
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float mo_decode(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ __forceinline__ bool mo_key_finite(unsigned k) { return k > MO_KEY_NEG_INF && k < MO_KEY_POS_INF; }

__global__ __launch_bounds__(256) void k_mo_keys(const float* __restrict__ fcst, long long n, unsigned* __restrict__ key) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) key[i] = mo_encode(fcst[i]);
}

// ---- a stretch of plateaus ------------------------------------------------------------------------------------------------------------
constexpr unsigned MO_HAS = 1;       // the stretch has a plateau: fu, fs, lu, ls are set
constexpr unsigned MO_BEST = 2;      // ... and one with a valid score: best, lo are set
constexpr unsigned MO_HI = 4;        // a plateau above lo inside the stretch has another score: hi is set (else the run reaches the end)
constexpr unsigned MO_LOFIRST = 8;   // lo is the first plateau of the stretch
struct MoRun {
    float fu, fs, lu, ls;   // first / last plateau: its value of fcst and its score
    float best, lo, hi;
    unsigned flags;
};
static_assert(sizeof(MoRun) == 32, "eight words");

__device__ __forceinline__ MoRun mo_empty() { return MoRun{0, 0, 0, 0, 0, 0, 0, 0u}; }
__device__ __forceinline__ MoRun mo_single(float u, float s) {
    return MoRun{u, s, u, s, s, u, 0, dev_valid(s) ? (MO_HAS | MO_BEST | MO_LOFIRST) : MO_HAS};
}
// L lies below R
__device__ __forceinline__ MoRun mo_combine(const MoRun& L, const MoRun& R) {
    if(!(R.flags & MO_HAS)) return L;
    if(!(L.flags & MO_HAS)) return R;
    MoRun o;
    o.fu = L.fu; o.fs = L.fs; o.lu = R.lu; o.ls = R.ls;
    const bool lb = L.flags & MO_BEST, rb = R.flags & MO_BEST;
    if(!rb || (lb && L.best >= R.best)) {   // a tie goes to the lower stretch
        o.best = L.best; o.lo = L.lo; o.hi = L.hi; o.flags = L.flags;
        if(lb && !(L.flags & MO_HI)) {      // L's run reaches its end: it goes on through R while R begins with the same score
            if(rb && R.best == L.best && (R.flags & MO_LOFIRST)) { o.hi = R.hi; o.flags |= R.flags & MO_HI; }
            else { o.hi = R.fu; o.flags |= MO_HI; }
        }
    }
    else {
        o.best = R.best; o.lo = R.lo; o.hi = R.hi; o.flags = R.flags & ~MO_LOFIRST;
    }
    return o;
}
__device__ __forceinline__ MoRun mo_shfl_down(const MoRun& m, int off) {
    MoRun o;
    o.fu = __shfl_down(m.fu, off, 64); o.fs = __shfl_down(m.fs, off, 64); o.lu = __shfl_down(m.lu, off, 64); o.ls = __shfl_down(m.ls, off, 64);
    o.best = __shfl_down(m.best, off, 64); o.lo = __shfl_down(m.lo, off, 64); o.hi = __shfl_down(m.hi, off, 64);
    o.flags = __shfl_down(m.flags, off, 64);
    return o;
}
// lane 0 gets the join of the 64 lanes' stretches in lane order (lane l holds [l, l + off) before the step with `off`)
__device__ __forceinline__ MoRun mo_wave_join(MoRun m, int lane) {
    for(int off = 1; off < 64; off <<= 1) {
        const MoRun up = mo_shfl_down(m, off);
        if(lane + off < 64) m = mo_combine(m, up);
    }
    return m;
}

// the elements of lane `tid` of tile `b`: positions [p0, p0 + cnt)
__device__ __forceinline__ void mo_range(long long n, int tile, long long b, int tid, long long& p0, int& cnt) {
    const int ipt = (tile + MO_THREADS - 1) / MO_THREADS;
    const long long end = min(n, (b + 1) * (long long)tile);
    p0 = b * (long long)tile + (long long)tid * ipt;
    cnt = (int)max(0LL, min((long long)ipt, end - p0));
}

// tot[(2 tl + w) * nblocks + b], tl = the threshold's index in the batch, w = 0: ref > t, 1: ref <= t
__global__ __launch_bounds__(MO_THREADS) void k_mo_totals(const float* __restrict__ sref, long long n, int tile, const float* __restrict__ thr, int tb,
                                                          long long nblocks, unsigned* __restrict__ tot) {
    __shared__ unsigned part[MO_THREADS / 64][2 * MO_G];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = blockIdx.x;
    float t[MO_G];
    unsigned c[2 * MO_G];
#pragma unroll
    for(int g = 0; g < MO_G; g++) {
        const int tl = blockIdx.y * MO_G + g;
        t[g] = tl < tb ? thr[tl] : NAN;
        c[2 * g] = c[2 * g + 1] = 0;
    }
    long long p0;
    int cnt;
    mo_range(n, tile, b, tid, p0, cnt);
    for(int j = 0; j < cnt; j++) {
        const float r = sref[p0 + j];
#pragma unroll
        for(int g = 0; g < MO_G; g++) { c[2 * g] += r > t[g]; c[2 * g + 1] += r <= t[g]; }
    }
#pragma unroll
    for(int k = 0; k < 2 * MO_G; k++) {
        for(int off = 32; off > 0; off >>= 1) c[k] += __shfl_down(c[k], off, 64);
        if(lane == 0) part[wave][k] = c[k];
    }
    __syncthreads();
    if(tid < 2 * MO_G) {
        const int tl = blockIdx.y * MO_G + tid / 2;
        if(tl < tb) tot[(size_t)(2 * tl + (tid & 1)) * nblocks + b] = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
    }
}

// row = blockIdx.x = 2 tl + w: base[row * nblocks + b] = the sum of tot[row * nblocks + 0 .. b - 1], total[row] = the sum of all
__global__ __launch_bounds__(MO_THREADS) void k_mo_scan(const unsigned* __restrict__ tot, long long nblocks, u64* __restrict__ base, u64* __restrict__ total) {
    __shared__ u64 wsum[MO_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned* const in = tot + (size_t)blockIdx.x * nblocks;
    u64* const out = base + (size_t)blockIdx.x * nblocks;
    const long long per = (nblocks + MO_THREADS - 1) / MO_THREADS;
    const long long ia = min(nblocks, tid * per), ib = min(nblocks, ia + per);
    u64 s = 0;
    for(long long i = ia; i < ib; i++) s += in[i];
    u64 incl = s;
    for(int off = 1; off < 64; off <<= 1) {
        const u64 v = __shfl_up(incl, off, 64);
        if(lane >= off) incl += v;
    }
    if(lane == 63) wsum[wave] = incl;
    __syncthreads();
    u64 run = incl - s;
    for(int w = 0; w < wave; w++) run += wsum[w];
    for(long long i = ia; i < ib; i++) { out[i] = run; run += in[i]; }
    if(tid == MO_THREADS - 1) total[blockIdx.x] = run;
}

__device__ __forceinline__ float mo_count(u64 v) { return (float)min(v, (u64)16777216ull); }   // the reference counts with `float x++`, which stops at 2^24

__global__ __launch_bounds__(MO_THREADS) void k_mo_sweep(const unsigned* __restrict__ skey, const float* __restrict__ sref, long long n, int tile,
                                                         const float* __restrict__ thr, int tb, long long nblocks, const u64* __restrict__ base,
                                                         const u64* __restrict__ total, int metric, MoRun* __restrict__ runs) {
    __shared__ unsigned wcount[MO_THREADS / 64][2 * MO_G];
    __shared__ MoRun wrun[MO_THREADS / 64][MO_G];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = blockIdx.x;
    long long p0;
    int cnt;
    mo_range(n, tile, b, tid, p0, cnt);
    const unsigned after = (cnt > 0 && p0 + cnt < n) ? skey[p0 + cnt] : 0u;   // the key behind the lane's last element (0, no finite key, behind the last of all)
    unsigned key[MO_IPT + 1];   // key[j] for j >= cnt: `after`
    float ref[MO_IPT];
#pragma unroll
    for(int j = 0; j < MO_IPT; j++) {
        key[j] = j < cnt ? skey[p0 + j] : after;
        ref[j] = j < cnt ? sref[p0 + j] : NAN;   // NaN counts nowhere
    }
    key[MO_IPT] = after;
    float t[MO_G];
    unsigned c[2 * MO_G];
#pragma unroll
    for(int g = 0; g < MO_G; g++) {
        const int tl = blockIdx.y * MO_G + g;
        t[g] = tl < tb ? thr[tl] : NAN;
        c[2 * g] = c[2 * g + 1] = 0;
    }
#pragma unroll
    for(int j = 0; j < MO_IPT; j++)
#pragma unroll
        for(int g = 0; g < MO_G; g++) { c[2 * g] += ref[j] > t[g]; c[2 * g + 1] += ref[j] <= t[g]; }
    // exclusive scan of the lanes' counts over the workgroup
    unsigned before[2 * MO_G];
#pragma unroll
    for(int k = 0; k < 2 * MO_G; k++) {
        unsigned incl = c[k];
        for(int off = 1; off < 64; off <<= 1) {
            const unsigned v = __shfl_up(incl, off, 64);
            if(lane >= off) incl += v;
        }
        if(lane == 63) wcount[wave][k] = incl;
        before[k] = incl - c[k];
    }
    __syncthreads();
    u64 pa[MO_G], pb[MO_G], ta[MO_G], tbb[MO_G];
    MoRun m[MO_G];
    const int live = min(MO_G, tb - (int)blockIdx.y * MO_G);   // the thresholds of this group: the last group of a batch may hold fewer
#pragma unroll
    for(int g = 0; g < MO_G; g++) {
        const int tl = min(blockIdx.y * MO_G + g, tb - 1);   // (a group's unused slots repeat the last threshold's carry; nothing of them is stored)
        for(int w = 0; w < wave; w++) { before[2 * g] += wcount[w][2 * g]; before[2 * g + 1] += wcount[w][2 * g + 1]; }
        pa[g] = base[(size_t)(2 * tl) * nblocks + b] + before[2 * g];
        pb[g] = base[(size_t)(2 * tl + 1) * nblocks + b] + before[2 * g + 1];
        ta[g] = total[2 * tl];
        tbb[g] = total[2 * tl + 1];
        m[g] = mo_empty();
    }
#pragma unroll
    for(int j = 0; j < MO_IPT; j++) {
        if(j < cnt) {
            const bool plateau = mo_key_finite(key[j]) && key[j] != key[j + 1];
            const float u = mo_decode(key[j]);
#pragma unroll
            for(int g = 0; g < MO_G; g++) {
                pa[g] += ref[j] > t[g];
                pb[g] += ref[j] <= t[g];
                if(plateau && g < live) {
                    const float s = gpp_score_value(mo_count(ta[g] - pa[g]), mo_count(tbb[g] - pb[g]), mo_count(pa[g]), mo_count(pb[g]), metric);
                    m[g] = mo_combine(m[g], mo_single(u, s));
                }
            }
        }
    }
#pragma unroll
    for(int g = 0; g < MO_G; g++) {
        if(g >= live) break;   // (the same for every lane)
        const MoRun w = mo_wave_join(m[g], lane);
        if(lane == 0) wrun[wave][g] = w;
    }
    __syncthreads();
    if(tid < MO_G) {
        const int tl = blockIdx.y * MO_G + tid;
        if(tl < tb) {
            MoRun w = wrun[0][tid];
            for(int k = 1; k < MO_THREADS / 64; k++) w = mo_combine(w, wrun[k][tid]);
            runs[(size_t)tl * nblocks + b] = w;
        }
    }
}

// workgroup tl (one wave): x of threshold tl of the batch
__global__ __launch_bounds__(64) void k_mo_finish(const MoRun* __restrict__ runs, long long nblocks, float* __restrict__ out) {
    const int lane = threadIdx.x;
    const MoRun* const in = runs + (size_t)blockIdx.x * nblocks;
    const long long per = (nblocks + 63) / 64;
    const long long ia = min(nblocks, lane * per), ib = min(nblocks, ia + per);
    MoRun m = mo_empty();
    for(long long i = ia; i < ib; i++) m = mo_combine(m, in[i]);
    m = mo_wave_join(m, lane);
    if(lane != 0) return;
    float x = NAN;
    if(m.flags & MO_BEST) {
        const float lo = m.lo, hi = (m.flags & MO_HI) ? m.hi : m.lu;
        x = (float)(((double)lo + (double)hi) / 2.0);
        if(hi > lo && !(x < hi)) x = lo;                       // adjacent floats: the midpoint rounds up to the next plateau
        if(m.best <= 0.0001f) x = NAN;                         // metric_optimizer.cpp:167-168
        if(fabsf(m.best - m.fs) < 0.001f || fabsf(m.best - m.ls) < 0.001f) x = NAN;   // :177-182
    }
    out[blockIdx.x] = x;
}

void check_metric(int metric) {
    if(!gpp_score_metric_known(metric)) invalid("Unknown metric");   // metric_optimizer.cpp:241-243
}

// x[0 .. T): the optimal forecast threshold of every thresholds[k] (host arrays); n > 0, T > 0
void mo_solve(const float* ref, const float* fcst, long long n, const float* thresholds, int T, int metric, float* x, int mem) {
    ensure_device();
    int tile = GPP_MO_TILE_ITEMS;
    if(path_env("GPP_MO_TILE")) tile = std::min(GPP_MO_TILE_ITEMS, std::max(1, atoi(path_env("GPP_MO_TILE"))));   // (tests: elements per workgroup)
    const long long nblocks = (n + tile - 1) / tile;
    if(nblocks > MO_MAX_TILES) invalid("too many values");
    InField r, f;
    r.bind(ref, (size_t)n, mem);
    f.bind(fcst, (size_t)n, mem);
    Staged<unsigned> key, skey;
    Staged<float> sref;
    key.get((size_t)n);
    skey.get((size_t)n);
    sref.get((size_t)n);
    launch(k_mo_keys, grid_capped(blocks_of(n), 8192), 256, 0, f.d, n, key.p);
    size_t sb = 0;
    GPP_HIP(rocprim::radix_sort_pairs((void*)nullptr, sb, key.p, skey.p, r.d, sref.p, (size_t)n, 0u, 32u, stream()));
    Staged<char> tmp;
    tmp.get(sb);
    GPP_HIP(rocprim::radix_sort_pairs((void*)tmp.p, sb, key.p, skey.p, r.d, sref.p, (size_t)n, 0u, 32u, stream()));
    const int TB = std::min(T, MO_BATCH);
    Staged<float> dthr, dout;
    dthr.upload(thresholds, (size_t)T);
    dout.get((size_t)T);
    Staged<unsigned> tot;
    Staged<u64> base, total;
    Staged<MoRun> runs;
    tot.get((size_t)2 * TB * nblocks);
    base.get((size_t)2 * TB * nblocks);
    total.get((size_t)2 * TB);
    runs.get((size_t)TB * nblocks);
    for(int t0 = 0; t0 < T; t0 += TB) {
        const int tb = std::min(TB, T - t0);
        const dim3 grid((unsigned)nblocks, (unsigned)((tb + MO_G - 1) / MO_G));
        launch(k_mo_totals, grid, MO_THREADS, 0, (const float*)sref.p, n, tile, (const float*)dthr.p + t0, tb, nblocks, tot.p);
        launch(k_mo_scan, 2 * tb, MO_THREADS, 0, (const unsigned*)tot.p, nblocks, base.p, total.p);
        launch(k_mo_sweep, grid, MO_THREADS, 0, (const unsigned*)skey.p, (const float*)sref.p, n, tile, (const float*)dthr.p + t0, tb, nblocks, (const u64*)base.p,
               (const u64*)total.p, metric, runs.p);
        launch(k_mo_finish, tb, 64, 0, (const MoRun*)runs.p, nblocks, dout.p + t0);
    }
    GPP_HIP(hipMemcpyAsync(x, dout.p, (size_t)T * sizeof(float), hipMemcpyDeviceToHost, stream()));
    GPP_HIP(hipStreamSynchronize(stream()));   // the one synchronisation of the call; the workspaces go back to the pool here
}

}   // namespace

extern "C" int gpp_get_optimal_threshold(const float* ref, const float* fcst, long long n, float threshold, int metric, float* out, int mem) {
    GPP_TRY
    check_metric(metric);
    if(n < 0) invalid("negative size");
    if(!out) invalid("out is NULL");
    *out = NAN;
    if(n == 0) return GPP_OK;
    if(!ref || !fcst) invalid("ref / fcst is NULL");
    mo_solve(ref, fcst, n, &threshold, 1, metric, out, mem);
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_metric_optimizer_curve(const float* ref, const float* fcst, long long n, const float* thresholds, int num_thresholds, int metric,
                                          float* out_ref, float* out_fcst, int* out_count, int mem) {
    GPP_TRY
    check_metric(metric);
    if(n < 0 || num_thresholds < 0) invalid("negative size");
    if(!out_count) invalid("out_count is NULL");
    *out_count = 0;
    if(num_thresholds == 0) return GPP_OK;
    if(!thresholds || !out_ref || !out_fcst) invalid("thresholds / out_ref / out_fcst is NULL");
    if(n == 0) return GPP_OK;   // every threshold gives NaN
    if(!ref || !fcst) invalid("ref / fcst is NULL");
    std::vector<float> x((size_t)num_thresholds, NAN);
    mo_solve(ref, fcst, n, thresholds, num_thresholds, metric, x.data(), mem);
    int count = 0;
    for(int k = 0; k < num_thresholds; k++)
        if(is_valid(x[k])) {   // metric_optimizer.cpp:121-124
            out_ref[count] = x[k];
            out_fcst[count] = thresholds[k];
            count++;
        }
    *out_count = count;
    return GPP_OK;
    GPP_CATCH
}
