// gridpp::simple_gradient (src/api/simple_gradient.cpp) and gridpp::full_gradient (src/api/gradient.cpp:5-274) for gfx950:
// the downscaling of every field they need and the correction that joins them, in one pass.
//
// The reference downscales each field on its own (full_gradient stacks values, gradients, elevations and lafs into one vec3
// and downscales that) and then combines the downscaled fields in a second loop.  Here one thread per output location does
// the time-independent work once: the nearest grid point (gpp_nearest_device, once per call), the box and, lazily, the
// weights (s, t) for Bilinear, the output elevation / laf and the downscaled input elevation / laf; then it loops over the
// T levels, gathers the value and gradient fields of level t and writes out[t][q] with unit stride across lanes.
//
// d(f), the locator that finds it and the combination of the downscaled fields are those of downscale_loc.h, shared with
// k_bilinear and the kernels of a plan; this unit holds the kernel around them and the entry points.  A box whose weights leave
// [0, 1] raises exactly when bilinear would raise on one of the fields the reference downscales: the weights are solved the
// first time any of those fields has four valid corners.
#include "common.h"
#include "downscale_loc.h"
#include "downscale_call.h"

using namespace gpp;

namespace {

struct DownscaleArgs : GradientFields {                  // values, egrad, lgrad [nt][n_in], out [nt][nq]
    const float* glat; const float* glon; int nY, nX;   // input grid, row-major
    const int* nn;                                       // nearest grid point of each output location
    const float* qlat; const float* qlon; int nq;        // output locations
    int nt; size_t n_in;
};

template <bool BIL>
__global__ __launch_bounds__(256) void k_downscale(const DownscaleArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if(q >= a.nq) return;
    DirectLoc<BIL> l(a.glat, a.glon, a.nY, a.nX, a.nn, a.qlat, a.qlon, q, a.err);
    gradient_levels(l, a, a.n_in, a.nt, (size_t)a.nq, q);
}

// values, egrad, lgrad: [nt][igrid->n] following `mem`; egrad / lgrad NULL = absent (simple_gradient: both NULL)
void downscale(gpp_points* igrid, gpp_points* to, const float* values, int nt, const float* egrad, const float* lgrad,
               float elev_gradient, int full, int downscaler, float* out, int mem) {
    ensure_device();
    if(!igrid || !to) invalid("grid / points is NULL");
    if(igrid->n > 0 && igrid->nx <= 0) invalid("the input must be a Grid");
    if(downscaler != 0 && downscaler != 1) invalid("Invalid downscaler");   // downscaling.cpp:16-17
    if(downscaler == 0 && igrid->type != to->type) invalid("Coordinate types must be the same");   // as gpp_nearest_levels
    if(nt < 0) invalid("negative number of time levels");
    const int nq = to->n;
    if(nq == 0 || nt == 0) return;
    DownscaleCall call((size_t)igrid->n, values, out, (size_t)nt * nq, mem);
    if(call.done) return;
    const size_t nin = (size_t)nt * igrid->n;
    InField v, eg, lg;
    v.bind(values, nin, mem);
    eg.bind(egrad, nin, mem);
    lg.bind(lgrad, nin, mem);
    igrid->to_device();
    to->to_device();
    if(downscaler == 1) {
        to->latlon_to_device();
        igrid->latlon_to_device();
    }
    DevBuf<int> idx;
    idx.get(nq);
    gpp_nearest_device(igrid, to->d_x.p, to->d_y.p, to->d_z.p, nq, 1, idx.p);
    DownscaleArgs a;
    a.glat = igrid->d_lat.p; a.glon = igrid->d_lon.p; a.nY = igrid->ny; a.nX = igrid->nx;
    a.nn = idx.p;
    a.qlat = to->d_lat.p; a.qlon = to->d_lon.p; a.nq = nq;
    a.values = v.d; a.egrad = eg.d; a.lgrad = lg.d;
    a.nt = nt; a.n_in = (size_t)igrid->n;
    a.ielev = igrid->d_elev.p; a.ilaf = igrid->d_laf.p;
    a.oelev = to->d_elev.p; a.olaf = to->d_laf.p;
    a.elev_gradient = elev_gradient;
    a.full = full;
    a.out = call.o.d; a.err = call.err;
    const dim3 grid(blocks_of(nq)), block(256);
    if(downscaler == 1) launch(k_downscale<true>, grid, block, 0, a);
    else launch(k_downscale<false>, grid, block, 0, a);
    call.finish();
}

}   // namespace

extern "C" int gpp_simple_gradient(gpp_points* igrid, gpp_points* to, const float* values, int nt, float elev_gradient, int downscaler,
                                   float* out, int mem) {
    GPP_TRY
    downscale(igrid, to, values, nt, nullptr, nullptr, elev_gradient, 0, downscaler, out, mem);
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_full_gradient(gpp_points* igrid, gpp_points* to, const float* values, int nt, const float* elev_gradient,
                                 const float* laf_gradient, int downscaler, float* out, int mem) {
    GPP_TRY
    downscale(igrid, to, values, nt, elev_gradient, laf_gradient, 0, 1, downscaler, out, mem);
    return GPP_OK;
    GPP_CATCH
}
