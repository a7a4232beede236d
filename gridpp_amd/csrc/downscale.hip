// gridpp::simple_gradient (src/api/simple_gradient.cpp) and gridpp::full_gradient (src/api/gradient.cpp:5-274) for gfx950:
// the downscaling of every field they need and the correction that joins them, in one pass.
//
// The reference downscales each field on its own (full_gradient stacks values, gradients, elevations and lafs into one vec3
// and downscales that) and then combines the downscaled fields in a second loop.  Here one thread per output location does
// the time-independent work once: the nearest grid point (gpp_nearest_device, once per call), the box and, lazily, the
// weights (s, t) for Bilinear, the output elevation / laf and the downscaled input elevation / laf; then it loops over the
// T levels, gathers the value and gradient fields of level t and writes out[t][q] with unit stride across lanes.
//
// d(f) at a location is what nearest / bilinear give for field f alone: for Bilinear the field is interpolated with the
// location's weights when its four corners are all valid and takes the nearest grid point's value otherwise
// (bilinear.cpp:322-403), so values, gradients, elevations and lafs may mix the two at one location.  A box whose weights
// leave [0, 1] raises exactly when bilinear would raise on one of the fields the reference downscales: the weights are
// solved the first time any of those fields has four valid corners.
#include "common.h"
#include "bilinear_geom.h"

using namespace gpp;

namespace {

struct DownscaleArgs {
    const float* glat; const float* glon; int nY, nX;   // input grid, row-major
    const int* nn;                                       // nearest grid point of each output location
    const float* qlat; const float* qlon; int nq;        // output locations
    const float* values; const float* egrad; const float* lgrad;   // [nt][n_in]; egrad / lgrad NULL = term absent
    int nt; size_t n_in;
    const float* ielev; const float* ilaf;               // input grid [n_in]
    const float* oelev; const float* olaf;               // output locations [nq]
    float elev_gradient;                                 // simple_gradient's scalar
    int full;                                            // 0: simple_gradient, 1: full_gradient
    float* out;                                          // [nt][nq]
    int* err;                                            // err[0] = 1 when a box is too distorted, err[1..2] = bits of one (s, t)
};

template <bool BIL>
__global__ __launch_bounds__(256) void k_downscale(const DownscaleArgs a) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if(q >= a.nq) return;
    const int n0 = a.nn[q];
    int I1 = -1, J1 = -1, I2 = -1, J2 = -1;
    bool inside = false;
    float lat = 0, lon = 0;
    if(BIL) {
        lat = a.qlat[q]; lon = a.qlon[q];
        inside = get_box(a.glat, a.glon, a.nY, a.nX, n0, lat, lon, I1, J1, I2, J2);
    }
    const int i0 = I1 * a.nX + J1, i1 = I2 * a.nX + J1, i2 = I1 * a.nX + J2, i3 = I2 * a.nX + J2;
    float s = 0, t = 0;
    bool solved = false;
    // d(f): field f downscaled at this location
    auto down = [&](const float* __restrict__ f) -> float {
        if(BIL && inside) {
            const float v0 = f[i0], v1 = f[i1], v2 = f[i2], v3 = f[i3];
            if(dev_valid(v0) && dev_valid(v1) && dev_valid(v2) && dev_valid(v3)) {
                if(!solved) {
                    const bool bad = weights(lon, lat, a.glon[i0], a.glon[i1], a.glon[i2], a.glon[i3], a.glat[i0], a.glat[i1], a.glat[i2],
                                             a.glat[i3], s, t);
                    solved = true;
                    if(bad && atomicCAS(&a.err[0], 0, 1) == 0) { a.err[1] = __float_as_int(s); a.err[2] = __float_as_int(t); }
                }
                return bilinear_value(v0, v1, v2, v3, s, t);
            }
        }
        return n0 >= 0 ? f[n0] : NAN;   // outside the domain or a missing corner: nearest neighbour
    };
    const size_t nq = a.nq;
    if(!a.full) {   // simple_gradient.cpp: out = d(values) + (oelev - d(ielevs)) * elev_gradient, no validity test
        const float elev_corr = (a.oelev[q] - down(a.ielev)) * a.elev_gradient;
        for(int k = 0; k < a.nt; ++k) a.out[(size_t)k * nq + q] = down(a.values + (size_t)k * a.n_in) + elev_corr;
        return;
    }
    // gradient.cpp:56-81: a term counts where the output's and the downscaled input's elevation (laf) are both valid
    float ediff = 0, ldiff = 0;
    bool euse = false, luse = false;
    if(a.egrad) {
        const float oe = a.oelev[q], ie = down(a.ielev);
        euse = dev_valid(oe) && dev_valid(ie);
        ediff = oe - ie;
    }
    if(a.lgrad) {
        const float ol = a.olaf[q], il = down(a.ilaf);
        luse = dev_valid(ol) && dev_valid(il);
        ldiff = ol - il;
    }
    for(int k = 0; k < a.nt; ++k) {
        const size_t off = (size_t)k * a.n_in;
        const float v = down(a.values + off);
        float laf_corr = 0, elev_corr = 0;
        // a gradient that is not used here is still downscaled by the reference: read its corners while the weights are unsolved
        if(a.lgrad) {
            if(luse) laf_corr = down(a.lgrad + off) * ldiff;
            else if(BIL && inside && !solved) (void)down(a.lgrad + off);
        }
        if(a.egrad) {
            if(euse) elev_corr = down(a.egrad + off) * ediff;
            else if(BIL && inside && !solved) (void)down(a.egrad + off);
        }
        a.out[(size_t)k * nq + q] = v + (laf_corr + elev_corr);
    }
}

__global__ void k_downscale_fill_nan(float* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n) out[i] = NAN;
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
    const size_t nout = (size_t)nt * nq;
    OutField o;
    o.bind(out, nout, mem);
    if(igrid->n == 0) {   // nearest.cpp:132-134, bilinear.cpp:37-39: all missing, and so is every sum with them
        hipLaunchKernelGGL(k_downscale_fill_nan, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, stream(), o.d, nout);
        GPP_HIP(hipGetLastError());
        o.finish();
        GPP_HIP(hipStreamSynchronize(stream()));
        return;
    }
    if(!values) invalid("values is NULL");
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
    DevBuf<int> idx, err;
    idx.get(nq);
    err.get(4);
    GPP_HIP(hipMemsetAsync(err.p, 0, 4 * sizeof(int), stream()));
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
    a.out = o.d; a.err = err.p;
    const dim3 grid((nq + 255) / 256), block(256);
    if(downscaler == 1) hipLaunchKernelGGL(k_downscale<true>, grid, block, 0, stream(), a);
    else hipLaunchKernelGGL(k_downscale<false>, grid, block, 0, stream(), a);
    GPP_HIP(hipGetLastError());
    int herr[4];
    GPP_HIP(hipMemcpyAsync(herr, err.p, sizeof(herr), hipMemcpyDeviceToHost, stream()));
    o.finish();
    GPP_HIP(hipStreamSynchronize(stream()));
    bilinear_check_distorted(herr);
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
