// The reusable downscaling plan (include/gridpp_hip.h: gpp_downscale_plan_*).  Everything of nearest / bilinear /
// simple_gradient / full_gradient that depends on no value -- the nearest grid point of every output location, its box (Grid::get_box)
// and the weights (s, t) -- is computed ONCE per pair of geometries; an apply is then a gather and, for Bilinear, four products per
// location and field: no search, no box test, no double-precision solve.
//
// Record of an output location:
//   Nearest    int32          the nearest grid point (-1: none)
//   Bilinear   int4, 16 B     .x the nearest grid point; .y the flat index c of corner (Y1, X1) of its box, -1 when it is in no box,
//                             -2 - c when the weights of the box leave [0, 1] (the reference throws there); .z / .w the bits of s / t.
// The planned locator of downscale_loc.h reads a record; d(f), the level loop and the gradient combination are the ones the direct
// calls use, so a kernel here is a few lines around them.  Inside a box the nearest-neighbour fallback of a field with a missing
// corner takes that corner's value from the registers instead of a fifth load (the nearest grid point is one of the four).
//
// The error of a distorted box keeps the condition of the direct calls: a location with bad weights raises in the apply in which one
// of the downscaled fields has four valid corners there (bilinear.cpp:309-313), never at construction.
#include "common.h"
#include "downscale_loc.h"
#include "downscale_call.h"
#include "ensemble_downscale.h"
#include <climits>
#include <memory>

using namespace gpp;

namespace {

__global__ __launch_bounds__(256) void k_plan_build(const float* __restrict__ glat, const float* __restrict__ glon, int nY, int nX,
                                                    const int* __restrict__ nn, const float* __restrict__ qlat,
                                                    const float* __restrict__ qlon, int nq, int4* __restrict__ rec,
                                                    unsigned long long* __restrict__ distorted) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if(q >= nq) return;
    const int n0 = nn[q];
    const float lat = qlat[q], lon = qlon[q];
    int I1, J1, I2, J2;
    int code = -1;
    float s = 0, t = 0;
    if(get_box(glat, glon, nY, nX, n0, lat, lon, I1, J1, I2, J2)) {
        const int i0 = I1 * nX + J1, i1 = I2 * nX + J1, i2 = I1 * nX + J2, i3 = I2 * nX + J2;
        const bool bad = weights(lon, lat, glon[i0], glon[i1], glon[i2], glon[i3], glat[i0], glat[i1], glat[i2], glat[i3], s, t);
        code = bad ? -2 - i0 : i0;
        if(bad) atomicAdd(distorted, 1ull);
    }
    rec[q] = make_int4(n0, code, __float_as_int(s), __float_as_int(t));
}

// values [nt][nG] -> out [nt][nq]: a location per thread, unit-stride writes across lanes per level (as k_bilinear / k_gather_levels)
template <bool BIL>
__global__ __launch_bounds__(256) void k_plan_apply(const int4* __restrict__ rec, const int* __restrict__ nn, const int nq, const int nX,
                                                    const size_t nG, const float* __restrict__ values, const int nt,
                                                    float* __restrict__ out, int* __restrict__ err) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if(q >= nq) return;
    PlannedLoc<BIL> l(rec, nn, q, nX, err);
    down_levels(l, values, nG, nt, out, (size_t)nq, q);
}

// values [nG][E] -> out [nq][E] (gridpp's cube layout, the member index innermost): G lanes per location, 64 / G locations per wave;
// lane j of a group takes V members at V j, V (j + G), ...: every corner is read as runs of V G contiguous floats and the output run is
// written with unit stride across the group.  The four-corner validity test is per member.  V = 2 (one 8-byte access per lane; E even,
// both arrays 8-byte aligned) is the measured winner for Bilinear, V = 1 serves every other case.
// The loads are PlannedLoc::down_members' written out: calling it here costs the Bilinear V = 1 kernels four VGPRs (30 -> 34).  The
// occupancy would stay 8 waves per SIMD; the rule that a refactor leaves every kernel's registers as they were decided it, not a timing.
template <bool BIL, int G, int V>
__global__ __launch_bounds__(256) void k_plan_apply_cube(const int4* __restrict__ rec, const int* __restrict__ nn, const int nq,
                                                         const int nX, const float* __restrict__ values, const int E,
                                                         float* __restrict__ out, int* __restrict__ err) {
    using vec = typename VecOf<V>::type;
    const size_t g = (size_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if(g >= (size_t)nq) return;
    const int q = (int)g, lane = threadIdx.x % G;
    PlannedLoc<BIL> l(rec, nn, q, nX, err);
    float* __restrict__ o = out + (size_t)q * E;
    for(int e = lane * V; e < E; e += G * V) {
        union { vec v; float f[V]; } a0, a1, a2, a3, r;
        if(BIL && l.inside) {
            const float* __restrict__ f = values + (size_t)l.c * E + e;
            a0.v = *reinterpret_cast<const vec*>(f); a1.v = *reinterpret_cast<const vec*>(f + (size_t)nX * E);
            a2.v = *reinterpret_cast<const vec*>(f + E); a3.v = *reinterpret_cast<const vec*>(f + (size_t)(nX + 1) * E);
#pragma unroll
            for(int u = 0; u < V; ++u) r.f[u] = l.in_box(a0.f[u], a1.f[u], a2.f[u], a3.f[u]);
        }
        else if(l.n0 >= 0) r.v = *reinterpret_cast<const vec*>(values + (size_t)l.n0 * E + e);   // outside the domain: nearest neighbour
        else {
#pragma unroll
            for(int u = 0; u < V; ++u) r.f[u] = NAN;
        }
        *reinterpret_cast<vec*>(o + e) = r.v;
    }
}

struct GradientArgs : GradientFields {   // values, egrad, lgrad [nt][n_in], out [nt][nq]
    const int4* rec; const int* nn; int nq, nX;
    int nt; size_t n_in;
};

// k_downscale (downscale.hip) with d(f) read from the record
template <bool BIL>
__global__ __launch_bounds__(256) void k_plan_gradient(const GradientArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if(q >= a.nq) return;
    PlannedLoc<BIL> l(a.rec, a.nn, q, a.nX, a.err);
    gradient_levels(l, a, a.n_in, a.nt, (size_t)a.nq, q);
}

struct GradientCubeArgs : GradientFields {   // values [n_in][E], out [nq][E]; egrad / lgrad [n_in] shared by the members, or [n_in][E]
    const int4* rec; const int* nn; int nq, nX, E;
    int e_members, l_members;                // != 0: that gradient is [n_in][E]
};

// k_plan_gradient on cubes: values [n_in][E] -> out [nq][E] with the lanes of k_plan_apply_cube.  Everything that does not depend on
// the member -- the record, the two terms (gradient_term) and the correction of a gradient shared by the members -- is computed before
// the member loop (every lane of a group reads the same few addresses); with shared gradients the loop is k_plan_apply_cube's plus one
// add.  PM: a gradient has a field per member and adds its four corner runs to the loop.
template <bool BIL, int G, int V, bool PM>
__global__ __launch_bounds__(256) void k_plan_gradient_cube(const GradientCubeArgs a) {
    using vec = typename VecOf<V>::type;
    const size_t g = (size_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if(g >= (size_t)a.nq) return;
    const int q = (int)g, lane = threadIdx.x % G, E = a.E;
    PlannedLoc<BIL> l(a.rec, a.nn, q, a.nX, a.err);
    const bool e_pm = PM && a.e_members, l_pm = PM && a.l_members;
    float elev_corr = 0, laf_corr = 0, corr;
    GradientTerm et, lt;
    if(!a.full) corr = (a.oelev[q] - l.down(a.ielev)) * a.elev_gradient;   // simple_gradient.cpp: no validity test
    else {
        if(a.lgrad) {
            lt = gradient_term(l, a.olaf, a.ilaf, q);
            if(!l_pm) laf_corr = gradient_corr(l, lt, a.lgrad);
        }
        if(a.egrad) {
            et = gradient_term(l, a.oelev, a.ielev, q);
            if(!e_pm) elev_corr = gradient_corr(l, et, a.egrad);
        }
        corr = laf_corr + elev_corr;
    }
    float* __restrict__ o = a.out + (size_t)q * E;
    for(int e = lane * V; e < E; e += G * V) {
        union { vec v; float f[V]; } r;
        float v[V];
        l.template down_members<V>(a.values, E, e, v);
        if(PM) {   // gradient_corr per member
            float lc[V], ec[V], t[V];
#pragma unroll
            for(int u = 0; u < V; ++u) { lc[u] = laf_corr; ec[u] = elev_corr; }
            if(l_pm && (lt.use || l.may_still_raise())) {
                l.template down_members<V>(a.lgrad, E, e, t);
#pragma unroll
                for(int u = 0; u < V; ++u) if(lt.use) lc[u] = t[u] * lt.diff;
            }
            if(e_pm && (et.use || l.may_still_raise())) {
                l.template down_members<V>(a.egrad, E, e, t);
#pragma unroll
                for(int u = 0; u < V; ++u) if(et.use) ec[u] = t[u] * et.diff;
            }
#pragma unroll
            for(int u = 0; u < V; ++u) r.f[u] = v[u] + (lc[u] + ec[u]);
        }
        else {
#pragma unroll
            for(int u = 0; u < V; ++u) r.f[u] = v[u] + corr;
        }
        *reinterpret_cast<vec*>(o + e) = r.v;
    }
}

// .x of the Bilinear records -> a plain index, for the ensemble downscalers
__global__ __launch_bounds__(256) void k_plan_nearest_of_records(const int4* __restrict__ rec, const int nq, int* __restrict__ nn) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if(q < nq) nn[q] = rec[q].x;
}

}   // namespace

struct gpp_downscale_plan {
    int downscaler = 0, nY = 0, nX = 0, nq = 0;
    int itype = 0, otype = 0;                // the coordinate types of the two sets (the ensemble downscalers need them equal)
    bool out_grid = false;                   // the output is a Grid (or holds nothing)
    size_t n_in = 0;
    long long distorted = 0;
    DevBuf<int4> rec;                        // Bilinear
    DevBuf<int> nn;                          // Nearest; for Bilinear .x of the records, extracted by the first ensemble downscaler
    bool nn_ready = false;
    DevBuf<float> ielev, ilaf, oelev, olaf;  // copies of the two sets' elevations and land area fractions (the gradient methods)
    DevBuf<int> err;
    long long bytes() const {
        return (long long)(rec.cap * sizeof(int4) + (nn.cap + err.cap) * sizeof(int) + (ielev.cap + ilaf.cap + oelev.cap + olaf.cap) * sizeof(float));
    }
};

namespace {

void copy_field(DevBuf<float>& dst, const float* src, size_t n) {
    dst.get(n);
    if(n) GPP_HIP(hipMemcpyAsync(dst.p, src, n * sizeof(float), hipMemcpyDeviceToDevice, stream()));
}

void plan_gradient(gpp_downscale_plan* p, const float* values, int nt, const float* egrad, const float* lgrad, float elev_gradient, int full,
                   float* out, int mem) {
    if(!p) invalid("plan handle is NULL");
    if(nt < 0) invalid("negative number of time levels");
    if(p->nq == 0 || nt == 0) return;
    ensure_device();
    mem &= ~GPP_ASYNC;
    DownscaleCall call(p->n_in, values, out, (size_t)nt * p->nq, mem, &p->err);
    if(call.done) return;
    const size_t nin = (size_t)nt * p->n_in;
    InField v, eg, lg;
    v.bind(values, nin, mem);
    eg.bind(egrad, nin, mem);
    lg.bind(lgrad, nin, mem);
    GradientArgs a;
    a.rec = p->rec.p; a.nn = p->nn.p; a.nq = p->nq; a.nX = p->nX;
    a.values = v.d; a.egrad = eg.d; a.lgrad = lg.d;
    a.nt = nt; a.n_in = p->n_in;
    a.ielev = p->ielev.p; a.ilaf = p->ilaf.p; a.oelev = p->oelev.p; a.olaf = p->olaf.p;
    a.elev_gradient = elev_gradient;
    a.full = full;
    a.out = call.o.d; a.err = call.err;
    const dim3 grid(blocks_of(p->nq)), block(256);
    if(p->downscaler == 1) launch(k_plan_gradient<true>, grid, block, 0, a);
    else launch(k_plan_gradient<false>, grid, block, 0, a);
    call.finish();
}

}   // namespace

extern "C" int gpp_downscale_plan_create(gpp_points* igrid, gpp_points* to, int downscaler, gpp_downscale_plan** plan) {
    GPP_TRY
    if(!igrid || !to || !plan) invalid("grid / points / plan handle is NULL");
    if(igrid->n > 0 && igrid->nx <= 0) invalid("the input must be a Grid");
    if(downscaler != 0 && downscaler != 1) invalid("Invalid downscaler");   // downscaling.cpp:16-17
    if(downscaler == 0 && igrid->type != to->type) invalid("Coordinate types must be the same");   // as gpp_nearest_levels
    ensure_device();
    std::unique_ptr<gpp_downscale_plan> p(new gpp_downscale_plan);
    p->downscaler = downscaler; p->nY = igrid->ny; p->nX = igrid->nx; p->nq = to->n; p->n_in = (size_t)igrid->n;
    p->itype = igrid->type; p->otype = to->type; p->out_grid = to->nx > 0 || to->n == 0;
    const int nq = to->n;
    if(nq > 0 && igrid->n > 0) {
        igrid->to_device();
        to->to_device();
        copy_field(p->ielev, igrid->d_elev.p, p->n_in); copy_field(p->ilaf, igrid->d_laf.p, p->n_in);
        copy_field(p->oelev, to->d_elev.p, nq); copy_field(p->olaf, to->d_laf.p, nq);
        if(downscaler == 0) {
            p->nn.get(nq);
            gpp_nearest_device(igrid, to->d_x.p, to->d_y.p, to->d_z.p, nq, 1, p->nn.p);
            p->nn_ready = true;
        }
        else {
            to->latlon_to_device();
            igrid->latlon_to_device();
            DevBuf<int> idx;
            DevBuf<unsigned long long> count;
            idx.get(nq); count.get(1);
            p->rec.get(nq);
            GPP_HIP(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), stream()));
            gpp_nearest_device(igrid, to->d_x.p, to->d_y.p, to->d_z.p, nq, 1, idx.p);
            launch(k_plan_build, blocks_of(nq), 256, 0, igrid->d_lat.p, igrid->d_lon.p, igrid->ny, igrid->nx, idx.p, to->d_lat.p, to->d_lon.p, nq, p->rec.p, count.p);
            unsigned long long h = 0;
            GPP_HIP(hipMemcpyAsync(&h, count.p, sizeof(h), hipMemcpyDeviceToHost, stream()));
            GPP_HIP(hipStreamSynchronize(stream()));
            p->distorted = (long long)h;
        }
        GPP_HIP(hipStreamSynchronize(stream()));
    }
    *plan = p.release();
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_downscale_plan_destroy(gpp_downscale_plan* plan) {
    GPP_TRY
    delete plan;
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_downscale_plan_info(const gpp_downscale_plan* plan, long long* locations, long long* cells, int* downscaler, long long* bytes,
                                       long long* distorted) {
    GPP_TRY
    if(!plan) invalid("plan handle is NULL");
    if(locations) *locations = plan->nq;
    if(cells) *cells = (long long)plan->n_in;
    if(downscaler) *downscaler = plan->downscaler;
    if(bytes) *bytes = plan->bytes();
    if(distorted) *distorted = plan->distorted;
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_downscale_plan_apply(gpp_downscale_plan* plan, const float* values, int nt, float* out, int mem) {
    GPP_TRY
    if(!plan) invalid("plan handle is NULL");
    if(nt < 0) invalid("negative number of time levels");
    if(plan->nq == 0 || nt == 0) return GPP_OK;
    ensure_device();
    mem &= ~GPP_ASYNC;
    DownscaleCall call(plan->n_in, values, out, (size_t)nt * plan->nq, mem, &plan->err);
    if(call.done) return GPP_OK;
    InField v;
    v.bind(values, (size_t)nt * plan->n_in, mem);
    const dim3 grid(blocks_of(plan->nq)), block(256);
    if(plan->downscaler == 1)
        launch(k_plan_apply<true>, grid, block, 0, (const int4*)plan->rec.p, (const int*)nullptr, plan->nq, plan->nX, plan->n_in, v.d, nt, call.o.d, call.err);
    else
        launch(k_plan_apply<false>, grid, block, 0, (const int4*)nullptr, (const int*)plan->nn.p, plan->nq, plan->nX, plan->n_in, v.d, nt, call.o.d, call.err);
    call.finish();
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_downscale_plan_apply_cube(gpp_downscale_plan* plan, const float* values, int ne, float* out, int mem) {
    GPP_TRY
    if(!plan) invalid("plan handle is NULL");
    if(ne < 0) invalid("negative number of members");
    if(plan->nq == 0 || ne == 0) return GPP_OK;
    ensure_device();
    mem &= ~GPP_ASYNC;
    DownscaleCall call(plan->n_in, values, out, (size_t)ne * plan->nq, mem, &plan->err);
    if(call.done) return GPP_OK;
    InField v;
    v.bind(values, (size_t)ne * plan->n_in, mem);
    const bool bil = plan->downscaler == 1;
    // 8-byte accesses where every row of members starts on an 8-byte boundary: measured faster than scalar ones for Bilinear on both
    // geometries of DESIGN.md 4.19, not for Nearest (and 16-byte ones only on one of the two)
    const bool wide = bil && ne % 2 == 0 && ((uintptr_t)v.d | (uintptr_t)call.o.d) % 8 == 0;
    const int G = group_of(wide ? ne / 2 : ne);
    const size_t blocks = ((size_t)plan->nq + 256 / G - 1) / (256 / G);
    if(blocks > (size_t)INT_MAX) invalid("too many output locations for this many members");
    const dim3 grid((unsigned)blocks), block(256);
    const int4* rec = bil ? plan->rec.p : nullptr;
    const int* nn = bil ? nullptr : plan->nn.p;
    dispatch_group(G, [&](auto g_) {
        constexpr int G_ = decltype(g_)::value;
        auto go = [&](auto kernel) { launch(kernel, grid, block, 0, rec, nn, plan->nq, plan->nX, v.d, ne, call.o.d, call.err); };
        if(wide) go(k_plan_apply_cube<true, G_, 2>);
        else if(bil) go(k_plan_apply_cube<true, G_, 1>);
        else go(k_plan_apply_cube<false, G_, 1>);
    });
    call.finish();
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_downscale_plan_simple_gradient(gpp_downscale_plan* plan, const float* values, int nt, float elev_gradient, float* out, int mem) {
    GPP_TRY
    plan_gradient(plan, values, nt, nullptr, nullptr, elev_gradient, 0, out, mem);
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_downscale_plan_full_gradient(gpp_downscale_plan* plan, const float* values, int nt, const float* elev_gradient,
                                                const float* laf_gradient, float* out, int mem) {
    GPP_TRY
    plan_gradient(plan, values, nt, elev_gradient, laf_gradient, 0, 1, out, mem);
    return GPP_OK;
    GPP_CATCH
}

namespace {

// the two cube-layout gradient entries: egrad / lgrad NULL = term absent, e_members / l_members 1 (a field shared by the members) or ne
void plan_gradient_cube(gpp_downscale_plan* p, const float* values, int ne, const float* egrad, int e_members, const float* lgrad, int l_members,
                        float elev_gradient, int full, float* out, int mem) {
    if(!p) invalid("plan handle is NULL");
    if(ne < 0) invalid("negative number of members");
    if(p->nq == 0 || ne == 0) return;
    if((egrad && e_members != 1 && e_members != ne) || (lgrad && l_members != 1 && l_members != ne))
        invalid("a gradient must have 1 or ne members");
    ensure_device();
    mem &= ~GPP_ASYNC;
    DownscaleCall call(p->n_in, values, out, (size_t)ne * p->nq, mem, &p->err);
    if(call.done) return;
    const bool e_pm = egrad && e_members == ne && ne > 1, l_pm = lgrad && l_members == ne && ne > 1;
    InField v, eg, lg;
    v.bind(values, (size_t)ne * p->n_in, mem);
    eg.bind(egrad, (e_pm ? (size_t)ne : 1) * p->n_in, mem);
    lg.bind(lgrad, (l_pm ? (size_t)ne : 1) * p->n_in, mem);
    GradientCubeArgs a;
    a.rec = p->rec.p; a.nn = p->nn.p; a.nq = p->nq; a.nX = p->nX; a.E = ne;
    a.values = v.d; a.egrad = eg.d; a.lgrad = lg.d;
    a.e_members = e_pm; a.l_members = l_pm;
    a.ielev = p->ielev.p; a.ilaf = p->ilaf.p; a.oelev = p->oelev.p; a.olaf = p->olaf.p;
    a.elev_gradient = elev_gradient;
    a.full = full;
    a.out = call.o.d; a.err = call.err;
    const bool bil = p->downscaler == 1, pm = e_pm || l_pm;
    // 8-byte accesses under k_plan_apply_cube's condition (Bilinear, E even), for every array that is read or written in runs of members
    uintptr_t bound = (uintptr_t)v.d | (uintptr_t)call.o.d;
    if(e_pm) bound |= (uintptr_t)eg.d;
    if(l_pm) bound |= (uintptr_t)lg.d;
    const bool wide = bil && ne % 2 == 0 && bound % 8 == 0;
    const int G = group_of(wide ? ne / 2 : ne);
    const size_t blocks = ((size_t)p->nq + 256 / G - 1) / (256 / G);
    if(blocks > (size_t)INT_MAX) invalid("too many output locations for this many members");
    const dim3 grid((unsigned)blocks), block(256);
    dispatch_group(G, [&](auto g_) {
        constexpr int G_ = decltype(g_)::value;
        auto go = [&](auto kernel) { launch(kernel, grid, block, 0, a); };
        if(wide) go(pm ? k_plan_gradient_cube<true, G_, 2, true> : k_plan_gradient_cube<true, G_, 2, false>);
        else if(bil) go(pm ? k_plan_gradient_cube<true, G_, 1, true> : k_plan_gradient_cube<true, G_, 1, false>);
        else go(pm ? k_plan_gradient_cube<false, G_, 1, true> : k_plan_gradient_cube<false, G_, 1, false>);
    });
    call.finish();
}

// what the planned ensemble downscalers check before the shared part of ensemble_downscale.hip; -> the index of the nearest grid points
void check_ensemble_plan(gpp_downscale_plan* p) {
    if(!p) invalid("plan handle is NULL");
    if(!p->out_grid) invalid("the plan's output must be a Grid");
    if(p->itype != p->otype) invalid("Coordinate types must be the same");
}
const int* plan_nearest_index(gpp_downscale_plan* p) {
    if(!p->nn_ready) {   // a Bilinear plan: .x of its records, extracted once and kept (4 bytes per location, counted in bytes())
        p->nn.get(p->nq);
        launch(k_plan_nearest_of_records, blocks_of(p->nq), 256, 0, (const int4*)p->rec.p, p->nq, p->nn.p);
        p->nn_ready = true;
    }
    return p->nn.p;
}

}   // namespace

extern "C" int gpp_downscale_plan_simple_gradient_cube(gpp_downscale_plan* plan, const float* values, int ne, float elev_gradient, float* out,
                                                       int mem) {
    GPP_TRY
    plan_gradient_cube(plan, values, ne, nullptr, 1, nullptr, 1, elev_gradient, 0, out, mem);
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_downscale_plan_full_gradient_cube(gpp_downscale_plan* plan, const float* values, int ne, const float* elev_gradient,
                                                     int elev_members, const float* laf_gradient, int laf_members, float* out, int mem) {
    GPP_TRY
    plan_gradient_cube(plan, values, ne, elev_gradient, elev_members, laf_gradient, laf_members, 0, 1, out, mem);
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_downscale_plan_probability(gpp_downscale_plan* plan, const float* values, int ne, const float* threshold,
                                              int comparison_operator, float* out, int mem) {
    GPP_TRY
    check_ensemble_plan(plan);
    ensemble_probability([&] { return plan_nearest_index(plan); }, plan->n_in, plan->nq, values, ne, threshold, comparison_operator, out,
                         mem & ~GPP_ASYNC);
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_downscale_plan_mask_threshold(gpp_downscale_plan* plan, const float* ivalues_true, const float* ivalues_false,
                                                 const float* threshold_values, int ne, const float* threshold, int comparison_operator,
                                                 int statistic, float quantile, float* out, int mem) {
    GPP_TRY
    check_ensemble_plan(plan);
    ensemble_mask_threshold([&] { return plan_nearest_index(plan); }, plan->n_in, plan->nq, ivalues_true, ivalues_false, threshold_values, ne,
                            threshold, comparison_operator, statistic, quantile, out, mem & ~GPP_ASYNC);
    return GPP_OK;
    GPP_CATCH
}
