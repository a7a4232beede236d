// gridpp::downscale_probability (src/api/downscale_probability.cpp:7-67) and gridpp::mask_threshold_downscale_consensus /
// _quantile (src/api/mask_threshold_downscale_consensus.cpp:12-82) for gfx950.
//
// The reference walks the output grid, looks up the nearest input cell (I, J) and loops over that cell's E members in a
// nested std::vector (one std::sort per cell for the order statistics).  Here the nearest index is found once per call
// (gpp_nearest_device) and one pass over the output cells follows.  The cubes are (Y, X, E) with E contiguous, so a cell's
// members are one run of 4 E bytes: a group of G lanes (G = 4 ... 64, chosen from E so that a lane reads at most four
// members up to E = 256) reads the run with unit stride across its lanes, 64 / G cells per wavefront.
//
//   k_ens_probability   two integers per cell (valid members, members that pass the test): summed across the group's lanes,
//                       any order is exact.
//   k_ens_mask          the group stages the masked row in LDS (ivalues_true / ivalues_false are loaded only where selected)
//                       and the row is reduced in member order by row_statistic / row_quantile of row_stats.h, the
//                       restatement of util.cpp:19-178 every other consumer uses.  Quantiles strictly between 0 and 1 find
//                       their two order statistics with all lanes of the group (rank counting over the staged row) and join
//                       them with quantile_from_order.
//   k_ens_mask_rows +   rows longer than GPP_ENSEMBLE_ROW_CAP members are not staged: the masked rows go to an HBM scratch
//   k_ens_rows_result   slab and one thread per cell runs the same row functions on its row from memory.  A slab holds 2^26
//                       masked members; GPP_ENSEMBLE_SLAB (a path override) sets another number, so that the tests run
//                       several slabs, a ragged last one included, on a grid of a hundred cells.
//
// The group size (group_of) and its way into a template argument (dispatch_group) are in ensemble_downscale.h, shared with the
// cube-layout kernels of a plan (downscale_plan.hip); the NaN / Count fills go through fill_f32 (runtime.hip).
#include "common.h"
#include "row_stats.h"
#include "ensemble_downscale.h"
#include <algorithm>

using namespace gpp;

namespace {

__device__ __forceinline__ bool compare(float a, float b, int op) {   // include/gridpp.h:138-143
    return op == GPP_LT ? a < b : (op == GPP_LEQ ? a <= b : (op == GPP_GT ? a > b : a >= b));
}

template <int G>
__device__ __forceinline__ int group_sum(int v) {
#pragma unroll
    for(int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
    return v;
}
template <int G>
__device__ __forceinline__ unsigned group_or(unsigned v) {
#pragma unroll
    for(int o = G / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o, G);
    return v;
}

// downscale_probability.cpp:20-63
template <int G>
__global__ __launch_bounds__(256) void k_ens_probability(const int* __restrict__ nn, const float* __restrict__ values, int E,
                                                         const float* __restrict__ threshold, int nq, int op, float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int cell = (int)(t / G), lane = (int)(t % G);
    const bool active = cell < nq;
    const int n0 = active ? nn[cell] : -1;
    int count = 0, total = 0;
    if(n0 >= 0) {
        const float* row = values + (size_t)n0 * E;
        const float th = threshold[cell];
        for(int k = lane; k < E; k += G) {
            const float m = row[k];
            if(dev_valid(m)) { ++count; total += compare(m, th, op) ? 1 : 0; }
        }
    }
    count = group_sum<G>(count);
    total = group_sum<G>(total);
    if(active && lane == 0) out[cell] = count == 0 ? NAN : (float)total / (float)count;
}

// mask_threshold_downscale_consensus.cpp:39-70: member k of the masked row
__device__ __forceinline__ float masked_member(const float* __restrict__ vt, const float* __restrict__ vf, const float* __restrict__ tv,
                                               size_t i, float th, int op) {
    const float t = tv[i];
    if(!dev_valid(t)) return NAN;
    return compare(t, th, op) ? vt[i] : vf[i];
}

__device__ __forceinline__ unsigned cell_hash(int cell, unsigned seed) {
    unsigned h = (unsigned)cell * 2654435761u ^ seed; h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    return h;
}

// what the reference computes from a masked row (:72-77), one thread, row in LDS or in memory
__device__ float row_result(const float* row, int n, int statistic, float quantile, int cell, unsigned seed) {
    if(statistic == GPP_QUANTILE) return row_quantile(row, n, quantile);
    if(statistic == GPP_MEDIAN) return row_quantile(row, n, 0.5f);   // util.cpp:96-105
    if(statistic == GPP_RANDOMCHOICE) {   // util.cpp:74-95 uses rand(); any valid member is a correct draw
        int N = 0;
        for(int i = 0; i < n; i++) if(dev_valid(row[i])) N++;
        return N > 0 ? row_kth(row, n, (int)(cell_hash(cell, seed) % (unsigned)N)) : NAN;
    }
    return row_statistic(row, n, statistic);
}

// the k0-th and k1-th smallest (0-based) valid values of a staged row with all lanes of the group: an element's rank is
// the number of valid elements before it in the order (f2ord, position) -- the order row_kth bisects on, so the values
// have the same bits.  Every lane returns both.
template <int G>
__device__ __forceinline__ void group_kth2(const float* row, int n, int k0, int k1, int lane, float& v0, float& v1) {
    unsigned b0 = 0, b1 = 0;
    for(int i = lane; i < n; i += G) {
        const float v = row[i];
        if(!dev_valid(v)) continue;
        const unsigned oi = f2ord(v);
        int rank = 0;
        for(int j = 0; j < n; j++) {
            const float w = row[j];
            if(!dev_valid(w)) continue;
            const unsigned oj = f2ord(w);
            rank += (oj < oi || (oj == oi && j < i)) ? 1 : 0;
        }
        if(rank == k0) b0 = __float_as_uint(v);
        if(rank == k1) b1 = __float_as_uint(v);
    }
    v0 = __uint_as_float(group_or<G>(b0));
    v1 = __uint_as_float(group_or<G>(b1));
}

// CAP: members a group's LDS row holds (E <= CAP is the launcher's business)
template <int G, int CAP>
__global__ __launch_bounds__(256) void k_ens_mask(const int* __restrict__ nn, const float* __restrict__ vt, const float* __restrict__ vf,
                                                  const float* __restrict__ tv, int E, const float* __restrict__ threshold, int nq, int op,
                                                  int statistic, float quantile, unsigned seed, float* __restrict__ out) {
    __shared__ float rows[256 / G][CAP];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int cell = (int)(t / G), lane = (int)(t % G);
    const bool active = cell < nq;
    float* row = rows[threadIdx.x / G];
    const int n = active ? E : 0;
    if(active) {
        const size_t base = (size_t)nn[cell] * E;
        const float th = threshold[cell];
        for(int k = lane; k < E; k += G) row[k] = masked_member(vt, vf, tv, base + k, th, op);
    }
    __syncthreads();
    const bool median = statistic == GPP_MEDIAN;
    const float q = median ? 0.5f : quantile;
    float value;
    if((statistic == GPP_QUANTILE || median) && dev_valid(q) && q != 0 && q != 1) {   // row_quantile (util.cpp:111-178) with the group
        int N = 0;
        for(int k = lane; k < n; k += G) N += dev_valid(row[k]) ? 1 : 0;
        N = group_sum<G>(N);
        value = NAN;
        if(N > 0) {   // (the same in every lane of the group)
            const float pos = q * (float)(N - 1);
            const int lowerIndex = (int)floorf(pos), upperIndex = (int)ceilf(pos);
            float lv, uv;
            group_kth2<G>(row, n, lowerIndex, upperIndex, lane, lv, uv);
            value = quantile_from_order(q, N, lv, uv, lowerIndex, upperIndex);
        }
    }
    else if(lane == 0) value = row_result(row, n, statistic, quantile, cell, seed);
    else return;
    if(active && lane == 0) out[cell] = value;
}

// rows that do not fit the LDS row: masked rows of cells [q0, q0 + nc) to scratch[nc][E], one wavefront per cell
__global__ __launch_bounds__(256) void k_ens_mask_rows(const int* __restrict__ nn, const float* __restrict__ vt, const float* __restrict__ vf,
                                                       const float* __restrict__ tv, int E, const float* __restrict__ threshold, int q0, int nc,
                                                       int op, float* __restrict__ scratch) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if(c >= nc) return;
    const int cell = q0 + c;
    const size_t base = (size_t)nn[cell] * E;
    const float th = threshold[cell];
    float* row = scratch + (size_t)c * E;
    for(int k = lane; k < E; k += 64) row[k] = masked_member(vt, vf, tv, base + k, th, op);
}
__global__ __launch_bounds__(256) void k_ens_rows_result(const float* __restrict__ scratch, int E, int q0, int nc, int statistic, float quantile,
                                                         unsigned seed, float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if(c >= nc) return;
    out[q0 + c] = row_result(scratch + (size_t)c * E, E, statistic, quantile, q0 + c, seed);
}

// members the LDS row of a group of G lanes holds: the four per lane that group_of allows, the whole cap for the largest group
constexpr int row_cap(int G) { return G == 64 ? GPP_ENSEMBLE_ROW_CAP : 4 * G; }

void check_operator(int op) {
    if(op != GPP_LT && op != GPP_LEQ && op != GPP_GT && op != GPP_GEQ) invalid("Invalid comparison operator");
}

// checks of the two direct entry points (those of the ensemble itself follow in ensemble_probability / ensemble_mask_threshold)
void check_grids(gpp_points* igrid, gpp_points* ogrid) {
    if(!igrid || !ogrid) invalid("grid is NULL");
    if(igrid->n > 0 && igrid->nx <= 0) invalid("the input must be a Grid");
    if(igrid->type != ogrid->type) invalid("Coordinate types must be the same");   // as gpp_nearest_levels
}
void check_ensemble(int ne, int op) {
    if(ne < 0) invalid("negative number of ensemble members");
    check_operator(op);
}

void fill(OutField& o, size_t n, float v) {
    fill_f32(o.d, n, v);
    finish_call(o);
}

void nearest_index(gpp_points* igrid, gpp_points* ogrid, DevBuf<int>& idx) {
    igrid->to_device();
    ogrid->to_device();
    idx.get(ogrid->n);
    gpp_nearest_device(igrid, ogrid->d_x.p, ogrid->d_y.p, ogrid->d_z.p, ogrid->n, 1, idx.p);
}

// masked members per scratch slab (2^26 = 256 MiB; GPP_ENSEMBLE_SLAB overrides it so that the tests can reach the loop over slabs)
long long slab_members() {
    const char* e = path_env("GPP_ENSEMBLE_SLAB");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? v : (1ll << 26);
}

unsigned g_seed = 0x9e3779b9u;   // RandomChoice: a different draw every call (under the API lock)

}   // namespace

void gpp::ensemble_probability(const NearestIndex& index, size_t n_in, int nq, const float* values, int ne, const float* threshold,
                               int comparison_operator, float* out, int mem) {
    check_ensemble(ne, comparison_operator);
    if(nq == 0) return;
    if(!out) invalid("out is NULL");
    ensure_device();
    OutField o;
    o.bind(out, nq, mem);
    if(n_in == 0 || ne == 0) {   // no nearest cell (as gpp_nearest_levels) / count == 0 (:53-55)
        fill(o, nq, NAN);
        return;
    }
    if(!values || !threshold) invalid("values / threshold is NULL");
    InField v, th;
    v.bind(values, n_in * ne, mem);
    th.bind(threshold, nq, mem);
    const int* idx = index();
    dispatch_group(group_of(ne), [&](auto g) {
        constexpr int G = decltype(g)::value;
        launch(k_ens_probability<G>, blocks_of((size_t)nq * G), 256, 0, idx, v.d, ne, th.d, nq, comparison_operator, o.d);
    });
    finish_call(o);
}

void gpp::ensemble_mask_threshold(const NearestIndex& index, size_t n_in, int nq, const float* ivalues_true, const float* ivalues_false,
                                  const float* threshold_values, int ne, const float* threshold, int comparison_operator, int statistic,
                                  float quantile, float* out, int mem) {
    check_ensemble(ne, comparison_operator);
    switch(statistic) {   // util.cpp:19-110
        case GPP_MEAN: case GPP_MIN: case GPP_MEDIAN: case GPP_MAX: case GPP_QUANTILE: case GPP_STD: case GPP_VARIANCE:
        case GPP_SUM: case GPP_COUNT: case GPP_RANDOMCHOICE: break;
        default: runtime("Internal error. Cannot compute statistic");
    }
    if(statistic == GPP_QUANTILE && (quantile < 0 || quantile > 1))   // util.cpp:112-113 (a NaN passes and gives NaN)
        invalid("calc_quantile: Quantile must be between 0 and 1 inclusive");
    if(nq == 0) return;
    if(!out) invalid("out is NULL");
    ensure_device();
    OutField o;
    o.bind(out, nq, mem);
    if(n_in == 0 || ne == 0) {   // no nearest cell: all missing; no member: calc_statistic of nothing (Count -> 0)
        fill(o, nq, (n_in > 0 && statistic == GPP_COUNT) ? 0.0f : NAN);
        return;
    }
    if(!ivalues_true || !ivalues_false || !threshold_values || !threshold) invalid("a field is NULL");
    const size_t nin = n_in * ne;
    InField vt, vf, tv, th;
    vt.bind(ivalues_true, nin, mem);
    vf.bind(ivalues_false, nin, mem);
    tv.bind(threshold_values, nin, mem);
    th.bind(threshold, nq, mem);
    const int* idx = index();
    const unsigned seed = (g_seed = g_seed * 1664525u + 1013904223u);
    if(ne <= GPP_ENSEMBLE_ROW_CAP) {
        dispatch_group(group_of(ne), [&](auto g) {
            constexpr int G = decltype(g)::value;
            launch(k_ens_mask<G, row_cap(G)>, blocks_of((size_t)nq * G), 256, 0, idx, vt.d, vf.d, tv.d, ne, th.d, nq, comparison_operator, statistic, quantile, seed, o.d);
        });
    }
    else {   // slabs of at most 2^26 masked members (256 MiB)
        const int slab = (int)std::max<long long>(1, std::min<long long>(nq, slab_members() / ne));
        DevBuf<float> scratch;
        scratch.get((size_t)slab * ne);
        for(int q0 = 0; q0 < nq; q0 += slab) {
            const int nc = std::min(slab, nq - q0);
            launch(k_ens_mask_rows, (nc + 3) / 4, 256, 0, idx, vt.d, vf.d, tv.d, ne, th.d, q0, nc, comparison_operator, scratch.p);
            launch(k_ens_rows_result, blocks_of(nc), 256, 0, (const float*)scratch.p, ne, q0, nc, statistic, quantile, seed, o.d);
        }
    }
    finish_call(o);
}

extern "C" int gpp_downscale_probability(gpp_points* igrid, gpp_points* ogrid, const float* values, int ne, const float* threshold,
                                         int comparison_operator, float* out, int mem) {
    GPP_TRY
    check_grids(igrid, ogrid);
    DevBuf<int> idx;
    ensemble_probability([&] { nearest_index(igrid, ogrid, idx); return (const int*)idx.p; }, (size_t)igrid->n, ogrid->n, values, ne, threshold,
                         comparison_operator, out, mem);
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_mask_threshold_downscale(gpp_points* igrid, gpp_points* ogrid, const float* ivalues_true, const float* ivalues_false,
                                            const float* threshold_values, int ne, const float* threshold, int comparison_operator,
                                            int statistic, float quantile, float* out, int mem) {
    GPP_TRY
    check_grids(igrid, ogrid);
    DevBuf<int> idx;
    ensemble_mask_threshold([&] { nearest_index(igrid, ogrid, idx); return (const int*)idx.p; }, (size_t)igrid->n, ogrid->n, ivalues_true,
                            ivalues_false, threshold_values, ne, threshold, comparison_operator, statistic, quantile, out, mem);
    return GPP_OK;
    GPP_CATCH
}
