// local_distribution_correction on the device (src/api/local_distribution_correction.cpp:18-203).
//
// Per grid cell: the stations within the structure's localization distance (KDTree::get_neighbours, match included), rho =
// corr_background(cell, station), every valid non-negative (pobs, pbackground) pair of those stations over the nT times kept
// with that rho.  The kept pairs are sorted twice -- by (pobs, rho) and by (pbackground, rho) -- trimmed to the quantile
// range, turned into two cumulative-rho curves and the cell's background is mapped through them (:114-199).
//
// THE TIE RULE.  The reference sorts the pairs by value alone with an unstable sort, so on tied values (precipitation: many
// zeros) its result depends on the order its R-tree returns the neighbours in.  Here ties in value are ordered by rho
// ascending: the 64-bit key `value bits << 32 | rho bits` of two non-negative floats orders as an integer (-0 is stored as
// +0), two pairs that still tie are identical, and the result does not depend on the order the bins are walked in.  On
// tie-free data it is the reference's result.
//
// Layout: the counted-then-filled CSR pattern of gpp_smart (radius_csr.h).  k_ldc_count counts the kept pairs and settles
// every cell that needs no curve (invalid background, too few pairs, branch 1, no pair at all); k_ldc_fill writes the two
// key arrays of the other cells, per chunk of at most CSR_CAP pairs; then one wavefront per cell does the rest:
//   k_ldc_cell_lds   count <= LDC_LDS_MAX: both key arrays sorted by a bitonic network in LDS, the curves built in LDS
//   k_ldc_cell_hbm   above that (or every cell, under the path override GPP_LDC_HBM): the keys sorted in HBM by rocPRIM's
//                    segmented radix sort, the curves built in an HBM workspace -- no capacity limit
// Both call ldc_finish, so they differ in where the arrays live and in nothing else.  The cumulative sums and sum_rho are
// sequential float32 sums over the SORTED order (one lane per curve): the curves carry the reference's bits, and sum_rho
// -- the one quantity whose summation order the reference leaves to its R-tree -- is the same for every walk order.
#include "common.h"
#include "oi_common.h"
#include "radius_csr.h"
#include "curve.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>

using namespace gpp;

namespace {

typedef unsigned long long u64;

constexpr int LDC_LDS_MAX = 512;   // pairs per cell the LDS path takes: 2 x 512 keys + 4 x 513 floats = 16 400 bytes per wavefront

// the bits of a non-negative float as a sort key (-0 -> +0)
__device__ __forceinline__ unsigned key_bits(float v) { return __float_as_uint(v == 0.0f ? 0.0f : v); }
__device__ __forceinline__ bool ldc_kept(float o, float b) {   // :99-102
    return dev_valid(o) && dev_valid(b) && !(o < 0) && !(b < 0);
}

// Kept pairs per cell, and the result of every cell that needs no curve: out = background (:70) where the background is not
// valid (:72) or count < min_points (:114); 0 where background < 0.01 (branch 1, :156; the comparison is made in double, as
// the reference's literal makes it); with no pair at all the curve is the lone (0, 0) point and branch 2 applies (:160-176).
// cnt = 0 marks a settled cell.
__global__ __launch_bounds__(256) void k_ldc_count(IxView ix, float R, const float* __restrict__ px, const float* __restrict__ py,
                                                   const float* __restrict__ pz, int nq, const float* __restrict__ background,
                                                   const float* __restrict__ pobs, const float* __restrict__ pbg, int nS, int nT,
                                                   int min_points, int* __restrict__ cnt, int* __restrict__ max_cnt, float* __restrict__ out) {
    const int y = blockIdx.x * blockDim.x + threadIdx.x;
    if(y >= nq) return;
    const float b = background[y];
    float r = b;
    int c = 0;
    if(dev_valid(b)) {
        visit_radius(ix, px[y], py[y], pz[y], R, true, [&](int, int orig, float) {
            for(int t = 0; t < nT; ++t) c += ldc_kept(pobs[(size_t)t * nS + orig], pbg[(size_t)t * nS + orig]) ? 1 : 0;
        });
        if(c < min_points) c = 0;
        else if((double)b < 0.01) { r = 0.0f; c = 0; }
        else if(c == 0 && (double)b < 0.1) r = 0.0f;   // 2a cannot hold (3 * 0), 2b, else 2c
    }
    out[y] = r;
    cnt[y] = c;
    if(c > LDC_LDS_MAX) atomicMax(max_cnt, c);
}

// The two key arrays of the cells k_ldc_count left open, at the cell's CSR offset
__global__ __launch_bounds__(256) void k_ldc_fill(IxView ix, DevStructure st, const float* __restrict__ px, const float* __restrict__ py,
                                                  const float* __restrict__ pz, const float* __restrict__ pe, const float* __restrict__ pl,
                                                  int q0, int nq, const float* __restrict__ pobs, const float* __restrict__ pbg, int nS, int nT,
                                                  const int* __restrict__ cnt, const long long* __restrict__ offset, long long base,
                                                  u64* __restrict__ kr, u64* __restrict__ kf) {
    const int y = q0 + blockIdx.x * blockDim.x + threadIdx.x;
    if(y >= q0 + nq || cnt[y] == 0) return;
    const float x1 = px[y], y1 = py[y], z1 = pz[y], e1 = pe[y], l1 = pl[y];
    long long w = offset[y] - base;
    visit_radius(ix, x1, y1, z1, st.R, true, [&](int j, int orig, float) {
        const float4 g = ix.sgeo[j];
        const unsigned rb = key_bits(d_corr(st, x1, y1, z1, e1, l1, g.x, g.y, g.z, g.w, ix.smeta[j].x, true));   // corr_background(p1, p2) (:96)
        for(int t = 0; t < nT; ++t) {
            const float o = pobs[(size_t)t * nS + orig], b = pbg[(size_t)t * nS + orig];
            if(!ldc_kept(o, b)) continue;
            kr[w] = ((u64)key_bits(o) << 32) | rb;
            kf[w] = ((u64)key_bits(b) << 32) | rb;
            ++w;
        }
    });
}

// :120-198 for one cell from its two SORTED key arrays (c >= 1 keys each; background valid and >= 0.01), by the 64 lanes of
// one wavefront that is a block of its own.  vr / qr / vf / qf: room for c + 1 floats each (LDS or HBM).
__device__ __forceinline__ void ldc_finish(const u64* kr, const u64* kf, float* vr, float* qr, float* vf, float* qf, const int c,
                                           const float b, const float min_quantile, const float max_quantile, float* out) {
    const int lane = threadIdx.x;
    int d1 = min((int)((float)c * max_quantile), c), d0 = min((int)((float)c * min_quantile), d1);   // :121-122
    const int m = d1 - d0, n = m + 1;   // n: the curve's length with its (0, 0) point (:127)
    for(int i = lane; i < m; i += 64) {
        const u64 a = kr[d0 + i], f = kf[d0 + i];
        vr[i + 1] = __uint_as_float((unsigned)(a >> 32)); qr[i + 1] = __uint_as_float((unsigned)a);
        vf[i + 1] = __uint_as_float((unsigned)(f >> 32)); qf[i + 1] = __uint_as_float((unsigned)f);
    }
    if(lane == 0) vr[0] = qr[0] = vf[0] = qf[0] = 0.0f;
    __syncthreads();
    const float ref_last = vr[m], fcst_last = vf[m];
    // the branches depend on sorted values only (:160-185)
    if(ref_last <= 0) {
        if(lane == 0 && (b < 3 * fcst_last || (double)b < 0.1)) *out = 0.0f;   // 2a, 2b; 2c keeps the background
        return;
    }
    if(b >= fcst_last) {
        if(lane == 0) *out = b + (ref_last - fcst_last);   // 3
        return;
    }
    // 4: cumulative rho (:135-141), sequential as the reference's; lane 0 the ref curve and sum_rho (:109), lane 1 the fcst curve
    float sum_rho = 0;
    if(lane == 0) {
        for(int s = 1; s < n; ++s) qr[s] = qr[s - 1] + qr[s];
        for(int i = 0; i < c; ++i) sum_rho += __uint_as_float((unsigned)kr[i]);
    }
    if(lane == 1)
        for(int s = 1; s < n; ++s) qf[s] = qf[s - 1] + qf[s];
    __syncthreads();
    const float sum_r = qr[m], sum_f = qf[m];
    __syncthreads();
    for(int s = 1 + lane; s < n; s += 64) {   // :151-154
        qr[s] = min_quantile + qr[s] / sum_r * (max_quantile - min_quantile);
        qf[s] = min_quantile + qf[s] / sum_f * (max_quantile - min_quantile);
    }
    __syncthreads();
    if(lane != 0) return;
    // both abscissa arrays are non-decreasing (sorted values; rounding keeps the normalised cumulative sums monotone) unless a sum of
    // rho is 0, which makes its quantiles NaN: interpolate's scans skip those, the bisection cannot
    const float q = curve::interpolate(b, vf, qf, n, true);         // :188
    const float new_ref = curve::interpolate(q, qr, vr, n, sum_r > 0);   // :189
    const float w0 = 1 - d_expf_cr(-0.01f * sum_rho);               // :191-193
    const float w1 = 1 - w0;
    *out = w0 * new_ref + w1 * b;
}

// One wavefront (= one block) per cell: load the keys, pad to a power of two with the largest key, bitonic sort, finish
__global__ __launch_bounds__(64) void k_ldc_cell_lds(const u64* __restrict__ kr, const u64* __restrict__ kf, const long long* __restrict__ offset,
                                                     long long base, const int* __restrict__ cnt, int q0, const float* __restrict__ background,
                                                     float min_quantile, float max_quantile, float* __restrict__ out) {
    __shared__ u64 skr[LDC_LDS_MAX], skf[LDC_LDS_MAX];
    __shared__ float sv[4][LDC_LDS_MAX + 1];
    const int y = q0 + blockIdx.x, lane = threadIdx.x;
    const int c = cnt[y];
    if(c == 0 || c > LDC_LDS_MAX) return;
    const long long off = offset[y] - base;
    int P = 1;
    while(P < c) P <<= 1;
    for(int i = lane; i < P; i += 64) {
        skr[i] = i < c ? kr[off + i] : ~0ull;
        skf[i] = i < c ? kf[off + i] : ~0ull;
    }
    __syncthreads();
    for(int k = 2; k <= P; k <<= 1)
        for(int j = k >> 1; j > 0; j >>= 1) {
            for(int i = lane; i < P; i += 64) {
                const int l = i ^ j;
                if(l > i) {
                    const bool up = (i & k) == 0;
                    const u64 a = skr[i], a2 = skr[l], f = skf[i], f2 = skf[l];
                    if((a > a2) == up) { skr[i] = a2; skr[l] = a; }
                    if((f > f2) == up) { skf[i] = f2; skf[l] = f; }
                }
            }
            __syncthreads();
        }
    ldc_finish(skr, skf, sv[0], sv[1], sv[2], sv[3], c, background[y], min_quantile, max_quantile, out + y);
}

// The same from keys already sorted in HBM; the four float arrays of a cell at 4 * (pairs before it + cells before it) of `ws`
__global__ __launch_bounds__(64) void k_ldc_cell_hbm(const u64* __restrict__ kr, const u64* __restrict__ kf, const long long* __restrict__ offset,
                                                     long long base, const int* __restrict__ cnt, int q0, int every_cell,
                                                     const float* __restrict__ background, float min_quantile, float max_quantile,
                                                     float* __restrict__ ws, float* __restrict__ out) {
    const int y = q0 + blockIdx.x;
    const int c = cnt[y];
    if(c == 0 || (!every_cell && c <= LDC_LDS_MAX)) return;
    const long long off = offset[y] - base;
    float* w = ws + 4 * (off + blockIdx.x);
    const size_t len = (size_t)c + 1;
    ldc_finish(kr + off, kf + off, w, w + len, w + 2 * len, w + 3 * len, c, background[y], min_quantile, max_quantile, out + y);
}

// CSR offsets of a chunk as the 32-bit segment bounds rocPRIM's segmented sort takes (a chunk holds at most CSR_CAP pairs)
struct ChunkOffset {
    long long base;
    __host__ __device__ unsigned operator()(long long o) const { return (unsigned)(o - base); }
};

void sort_segments(const u64* in, u64* outk, long long size, const long long* offset, long long base, int nseg) {
    auto begin = rocprim::make_transform_iterator(offset, ChunkOffset{base});
    size_t sb = 0;
    GPP_HIP(rocprim::segmented_radix_sort_keys((void*)nullptr, sb, in, outk, (unsigned)size, (unsigned)nseg, begin, begin + 1, 0u, 64u, stream()));
    DevBuf<char> tmp;
    tmp.get(sb);
    GPP_HIP(rocprim::segmented_radix_sort_keys((void*)tmp.p, sb, in, outk, (unsigned)size, (unsigned)nseg, begin, begin + 1, 0u, 64u, stream()));
    GPP_HIP(hipStreamSynchronize(stream()));   // `tmp` is released here
}

}   // namespace

extern "C" int gpp_local_distribution_correction(gpp_points* grid, const float* background, gpp_points* points, const float* pobs,
                                                 const float* pbackground, int nT, const gpp_structure* st, float min_quantile,
                                                 float max_quantile, int min_points, float* out, int mem) {
    GPP_TRY
    if(!grid || !points || !st) invalid("NULL argument");
    if(grid->n > 0 && grid->nx <= 0) invalid("the background must be on a Grid");
    if(grid->type != points->type)
        invalid("Both background grid and observations points must be of same coordinate type (lat/lon or x/y)");
    if(nT < 0) invalid("the number of times must be >= 0");
    if(!is_valid(min_quantile) || !is_valid(max_quantile) || !(0 <= min_quantile && min_quantile <= max_quantile && max_quantile <= 1))
        invalid("min_quantile and max_quantile must be finite with 0 <= min_quantile <= max_quantile <= 1");
    const int nq = grid->n, nS = points->n;
    if(nq == 0) return GPP_OK;
    if(!background || !out) invalid("background or out is NULL");
    if(nS > 0 && nT > 0 && (!pobs || !pbackground)) invalid("pobs or pbackground is NULL");
    ensure_device();
    DevStructure d = gpp_resolve_structure(st);
    if(d.fh) runtime("local_distribution_correction: spatially varying structure functions are not supported on the GPU path yet");
    OutField o;
    o.bind(out, nq, mem);
    InField b, po, pb;
    b.bind(background, nq, mem);
    if(nS == 0) {   // no station: the background
        GPP_HIP(hipMemcpyAsync(o.d, b.d, sizeof(float) * nq, hipMemcpyDeviceToDevice, stream()));
        return finish_call(o);
    }
    po.bind(nT > 0 ? pobs : nullptr, (size_t)nT * nS, mem);
    pb.bind(nT > 0 ? pbackground : nullptr, (size_t)nT * nS, mem);
    grid->to_device();
    gpp_obs_index* ix = gpp_build_obs_index(points);
    const IxView iv = view_of(ix);
    DevBuf<int> cnt, max_cnt;
    cnt.get(nq);
    max_cnt.get(1);
    GPP_HIP(hipMemsetAsync(max_cnt.p, 0, sizeof(int), stream()));
    launch(k_ldc_count, blocks_of(nq), 256, 0, iv, d.R, grid->d_x.p, grid->d_y.p, grid->d_z.p, nq, b.d, po.d, pb.d, nS, nT, min_points, cnt.p, max_cnt.p, o.d);
    DevBuf<long long> wide, offset;
    const long long total = scan_counts(cnt.p, nq, wide, offset);
    if(total > 0) {
        int most = 0;
        GPP_HIP(hipMemcpy(&most, max_cnt.p, sizeof(int), hipMemcpyDeviceToHost));
        const char* e = path_env("GPP_LDC_HBM");
        const bool every_cell = e && atoi(e) != 0;
        DevBuf<u64> kr, kf, kr2, kf2;
        DevBuf<float> ws;
        for(auto ch : chunks_of(offset, nq, total)) {   // (one chunk unless the keys exceed CSR_CAP entries)
            const int q0 = ch.first, n = ch.second - ch.first;
            long long base = 0, end = total;
            if(total > CSR_CAP) {
                GPP_HIP(hipMemcpy(&base, offset.p + q0, sizeof(long long), hipMemcpyDeviceToHost));
                GPP_HIP(hipMemcpy(&end, offset.p + ch.second, sizeof(long long), hipMemcpyDeviceToHost));
            }
            const long long size = end - base;
            if(size == 0) continue;
            kr.get((size_t)size); kf.get((size_t)size);
            launch(k_ldc_fill, blocks_of(n), 256, 0, iv, d, grid->d_x.p, grid->d_y.p, grid->d_z.p, grid->d_elev.p, grid->d_laf.p, q0, n, po.d, pb.d, nS, nT, (const int*)cnt.p,
                   (const long long*)offset.p, base, kr.p, kf.p);
            if(!every_cell)
                launch(k_ldc_cell_lds, n, 64, 0, (const u64*)kr.p, (const u64*)kf.p, (const long long*)offset.p, base, (const int*)cnt.p, q0, b.d, min_quantile, max_quantile, o.d);
            if(every_cell || most > LDC_LDS_MAX) {
                kr2.get((size_t)size); kf2.get((size_t)size);
                sort_segments(kr.p, kr2.p, size, offset.p + q0, base, n);
                sort_segments(kf.p, kf2.p, size, offset.p + q0, base, n);
                ws.get(4 * ((size_t)size + n));
                launch(k_ldc_cell_hbm, n, 64, 0, (const u64*)kr2.p, (const u64*)kf2.p, (const long long*)offset.p, base, (const int*)cnt.p, q0, every_cell ? 1 : 0, b.d,
                       min_quantile, max_quantile, ws.p, o.d);
            }
        }
    }
    return finish_call(o);
    GPP_CATCH
}
