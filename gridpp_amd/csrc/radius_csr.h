// The pieces the radius-query consumers share (radius.hip, ldc.hip): the view of a point set's bin index, the walk over the bins
// that overlap a query's box with the reference's membership test (KDTree::get_neighbours), and the counted-then-filled CSR
// layout of variable-length results (a counting pass, a device-wide exclusive scan, filling passes of at most CSR_CAP entries).
#pragma once
#include "common.h"
#include "oi_common.h"
#include <rocprim/rocprim.hpp>
#include <algorithm>

namespace gpp {
namespace {

struct IxView {
    const float4* sgeo;
    const float2* smeta;
    const int* bin_start;
    int axis_a, axis_b, nbx, nby;
    float amin, bmin, inv_s;
};
IxView view_of(gpp_obs_index* ix) {
    return IxView{ix->d_sgeo.p, ix->d_smeta.p, ix->d_bin_start.p, ix->axis_a, ix->axis_b, ix->nbx, ix->nby, ix->amin, ix->bmin, ix->inv_s};
}

__device__ __forceinline__ int bin_of(float v, float lo, float inv_s, int nb) {
    const float f = floorf((v - lo) * inv_s);
    return (int)fminf(fmaxf(f, 0.0f), (float)(nb - 1));
}

// f(sorted position, original index, distance) for every point the reference's get_neighbours would return
template <class F>
__device__ __forceinline__ void visit_radius(const IxView& ix, float x, float y, float z, float radius, bool include_match, F f) {
    if(!(radius > 0)) return;   // an empty or NaN box holds nothing strictly inside
    const float lox = x - radius, hix = x + radius, loy = y - radius, hiy = y + radius, loz = z - radius, hiz = z + radius;
    const float alo = ix.axis_a == 0 ? lox : (ix.axis_a == 1 ? loy : loz), ahi = ix.axis_a == 0 ? hix : (ix.axis_a == 1 ? hiy : hiz);
    const float blo = ix.axis_b == 1 ? loy : (ix.axis_b == 2 ? loz : lox), bhi = ix.axis_b == 1 ? hiy : (ix.axis_b == 2 ? hiz : hix);
    const int bx0 = bin_of(alo, ix.amin, ix.inv_s, ix.nbx), bx1 = bin_of(ahi, ix.amin, ix.inv_s, ix.nbx);
    const int by0 = bin_of(blo, ix.bmin, ix.inv_s, ix.nby), by1 = bin_of(bhi, ix.bmin, ix.inv_s, ix.nby);
    for(int row = by0; row <= by1; ++row) {
        const int js = ix.bin_start[row * ix.nbx + bx0], je = ix.bin_start[row * ix.nbx + bx1 + 1];
        for(int j = js; j < je; ++j) {
            const float4 g = ix.sgeo[j];
            if(!(g.x > lox && g.x < hix && g.y > loy && g.y < hiy && g.z > loz && g.z < hiz)) continue;   // kdtree.cpp:46,53
            const float dx = g.x - x, dy = g.y - y, dz = g.z - z;
            const float d = sqrtf(dx * dx + dy * dy + dz * dz);                                          // kdtree.cpp:189-194
            if(!(include_match ? d <= radius : (d <= radius && d > 0))) continue;                        // kdtree.cpp:247-260
            f(j, __float_as_int(ix.smeta[j].y), d);
        }
    }
}

__global__ void k_widen(const int* __restrict__ in, int n, long long* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n) out[i] = in[i];
}

// entries per filling pass (2^28 = 1 GiB of float values; GPP_CSR_CAP overrides it so that the tests can reach the chunked path)
long long csr_cap() {
    const char* e = path_env("GPP_CSR_CAP");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? v : (1ll << 28);
}
#define CSR_CAP csr_cap()

// exclusive scan of the per-location counts into 64-bit offsets [nq + 1]; returns the total
long long scan_counts(const int* cnt, int nq, DevBuf<long long>& wide, DevBuf<long long>& offset) {
    wide.get((size_t)nq + 1);
    offset.get((size_t)nq + 1);
    GPP_HIP(hipMemsetAsync(wide.p + nq, 0, sizeof(long long), stream()));
    launch(k_widen, blocks_of(nq), 256, 0, cnt, nq, wide.p);
    size_t sb = 0;
    GPP_HIP(rocprim::exclusive_scan((void*)nullptr, sb, wide.p, offset.p, 0LL, (size_t)(nq + 1), rocprim::plus<long long>(), stream()));
    DevBuf<char> tmp;
    tmp.get(sb);
    GPP_HIP(rocprim::exclusive_scan((void*)tmp.p, sb, wide.p, offset.p, 0LL, (size_t)(nq + 1), rocprim::plus<long long>(), stream()));
    long long total = 0;
    GPP_HIP(hipMemcpyAsync(&total, offset.p + nq, sizeof(long long), hipMemcpyDeviceToHost, stream()));
    GPP_HIP(hipStreamSynchronize(stream()));
    return total;
}

// Query chunks [q0, q1) whose CSR segments fit CSR_CAP entries (the offsets come to the host only when one pass is not enough)
std::vector<std::pair<int, int>> chunks_of(const DevBuf<long long>& offset, int nq, long long total) {
    std::vector<std::pair<int, int>> ch;
    if(total <= CSR_CAP) { ch.emplace_back(0, nq); return ch; }
    std::vector<long long> h((size_t)nq + 1);
    GPP_HIP(hipMemcpy(h.data(), offset.p, sizeof(long long) * h.size(), hipMemcpyDeviceToHost));
    int q0 = 0;
    while(q0 < nq) {
        int q1 = (int)(std::upper_bound(h.begin() + q0, h.end(), h[q0] + CSR_CAP) - h.begin()) - 1;
        if(q1 <= q0) q1 = q0 + 1;   // a single location with more than CSR_CAP neighbours still gets its own pass
        ch.emplace_back(q0, q1);
        q0 = q1;
    }
    return ch;
}

}   // namespace
}   // namespace gpp
