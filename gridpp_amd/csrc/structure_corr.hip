// StructureFunction::corr / corr_background of ONE point against many (include/gridpp.h:2078,2086; src/api/structure.cpp:13-25,
// 113-135,231-267) for gfx950.
//
//   k_structure_corr_many   one second point per lane, 256 lanes per workgroup, at most CORR_MAX_BLOCKS workgroups (8 per compute unit)
//                           and a grid stride with a 64-bit index beyond that.  The structure arrives resolved at the first point
//                           (gpp_structure_at: ONE nearest-neighbour lookup per call, as structure.cpp:234-243 does it), so the kernel
//                           is the device function d_corr of oi_common.h -- the one k_structure_corr and the OI kernels run -- and
//                           nothing else: the values are those of the scalar entry bit for bit.  The five coordinates of a second point
//                           are read at `stride` floats from one lane to the next: 1 for the SoA arrays of a point-set handle
//                           (coalesced, 20 B in and 4 B out per point), 7 for the uploaded records of gpp_structure_corr_many (bound by
//                           that upload, not by the kernel).  No LDS, no scratch.
#include "oi_common.h"

using namespace gpp;

namespace {

constexpr int CORR_BLOCK = 256;
constexpr long long CORR_MAX_BLOCKS = 2048;

__global__ __launch_bounds__(CORR_BLOCK) void k_structure_corr_many(const DevStructure st, const float4 p1, const float l1, const float* __restrict__ x,
                                                                    const float* __restrict__ y, const float* __restrict__ z,
                                                                    const float* __restrict__ elev, const float* __restrict__ laf,
                                                                    const int stride, const long long n, const int background,
                                                                    float* __restrict__ out) {
    const long long step = (long long)gridDim.x * CORR_BLOCK;
    for(long long i = (long long)blockIdx.x * CORR_BLOCK + threadIdx.x; i < n; i += step) {
        const long long k = i * stride;
        out[i] = d_corr(st, p1.x, p1.y, p1.z, p1.w, l1, x[k], y[k], z[k], elev[k], laf[k], background != 0);
    }
}

// resolve the structure at p1 and launch over n second points whose coordinates lie at x, y, z, elev, laf + i * stride (device memory)
void corr_launch(const gpp_structure* s, const float p1[7], const float* x, const float* y, const float* z, const float* elev,
                 const float* laf, int stride, long long n, int background, float* d_out) {
    const gpp_structure t = gpp_structure_at(s, p1[5], p1[6]);
    const DevStructure d = gpp_resolve_structure(&t);
    launch(k_structure_corr_many, grid_capped(blocks_of(n, CORR_BLOCK), CORR_MAX_BLOCKS), CORR_BLOCK, 0, d, make_float4(p1[0], p1[1], p1[2], p1[3]), p1[4], x, y, z, elev, laf, stride, n, background, d_out);
}

}   // namespace

extern "C" int gpp_structure_corr_many(const gpp_structure* s, const float p1[7], const float* p2, long long n, int background, float* rho) {
    GPP_TRY
    if(!s) invalid("structure is NULL");
    if(!p1) invalid("p1 is NULL");
    if(n < 0) invalid("n must be >= 0");
    if(n == 0) return GPP_OK;
    if(!p2 || !rho) invalid("NULL argument");
    ensure_device();
    InField in;
    OutField out;
    in.bind(p2, (size_t)n * 7, GPP_MEM_HOST);
    out.bind(rho, (size_t)n, GPP_MEM_HOST);
    corr_launch(s, p1, in.d, in.d + 1, in.d + 2, in.d + 3, in.d + 4, 7, n, background, out.d);
    return finish_call(out);
    GPP_CATCH
}

extern "C" int gpp_structure_corr_points(const gpp_structure* s, const float p1[7], gpp_points* to, int background, float* rho, int mem) {
    GPP_TRY
    if(!s) invalid("structure is NULL");
    if(!p1) invalid("p1 is NULL");
    if(!to) invalid("points is NULL");
    if(to->n == 0) return GPP_OK;
    if(!rho) invalid("NULL argument");
    ensure_device();
    to->to_device();
    OutField out;
    out.bind(rho, (size_t)to->n, mem);
    corr_launch(s, p1, to->d_x.p, to->d_y.p, to->d_z.p, to->d_elev.p, to->d_laf.p, 1, to->n, background, out.d);
    return finish_call(out);   // (a device result is read by the caller's own stream next)
    GPP_CATCH
}
