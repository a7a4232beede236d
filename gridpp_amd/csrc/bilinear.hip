// gridpp::bilinear (src/api/bilinear.cpp) and the box search it rests on (Grid::get_box, src/api/grid.cpp:149-229;
// point_in_rectangle, src/api/util.cpp:561-582) for gfx950.
//
// One thread per output location: the nearest grid point comes from the bin index (gpp_nearest_device), the four
// quadrants around it are tested in the reference's order, the weights (s, t) are solved once per location (they do not
// depend on the time level) and the T levels are gathered with unit-stride writes across locations: the direct locator and
// the level loop of downscale_loc.h, which the downscalers and the plan share.  All float expressions keep the reference's
// association (the build has -ffp-contract=off and correctly rounded float divide); the quadratic of the general
// quadrilateral is solved in double exactly as bilinear.cpp:159-267 does.
#include "common.h"
#include "downscale_loc.h"
#include "downscale_call.h"

using namespace gpp;

namespace {

// values [nt][nY*nX], out [nt][nq].  err[0] = 1 when a box is too distorted, err[1..2] = bits of one offending (s, t).
__global__ __launch_bounds__(256) void k_bilinear(const float* __restrict__ glat, const float* __restrict__ glon, int nY, int nX,
                                                  const int* __restrict__ nn, const float* __restrict__ qlat,
                                                  const float* __restrict__ qlon, int nq, const float* __restrict__ values, int nt,
                                                  float* __restrict__ out, int* __restrict__ err) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if(q >= nq) return;
    DirectLoc<true> l(glat, glon, nY, nX, nn, qlat, qlon, q, err);
    down_levels(l, values, (size_t)nY * nX, nt, out, (size_t)nq, q);
}

__global__ void k_get_box(const float* __restrict__ glat, const float* __restrict__ glon, int nY, int nX, const int* __restrict__ nn,
                          const float* __restrict__ qlat, const float* __restrict__ qlon, int nq, int* __restrict__ box) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if(q >= nq) return;
    int I1, J1, I2, J2;
    const bool inside = get_box(glat, glon, nY, nX, nn[q], qlat[q], qlon[q], I1, J1, I2, J2);
    box[5 * q + 0] = inside; box[5 * q + 1] = I1; box[5 * q + 2] = J1; box[5 * q + 3] = I2; box[5 * q + 4] = J2;
}

__global__ void k_in_rectangle(const float* p, int* out) {
    out[0] = in_rectangle(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]);
}

}   // namespace

void bilinear_check_distorted(const int herr[4]) {
    if(herr[0]) {   // bilinear.cpp:309-313
        float s, t;
        memcpy(&s, &herr[1], 4); memcpy(&t, &herr[2], 4);
        char msg[256];
        snprintf(msg, sizeof msg, "Problem with bilinear interpolation. Grid is rotated/distorted in a way that is not supported. "
                 "s=%g and t=%g are outside [-0.05,1.05].", s, t);
        runtime(msg);
    }
}

void gpp_points::latlon_to_device() {
    if(latlon_on_device) return;
    ensure_host_fields();
    d_lat.upload(lats.data(), n);
    d_lon.upload(lons.data(), n);
    GPP_HIP(hipStreamSynchronize(stream()));
    latlon_on_device = true;
}

extern "C" int gpp_bilinear(gpp_points* igrid, gpp_points* to, const float* values, int nt, float* out, int mem) {
    GPP_TRY
    ensure_device();
    if(!igrid || !to) invalid("grid / points is NULL");
    if(nt < 0) invalid("negative number of time levels");
    const int nq = to->n;
    if(nq == 0 || nt == 0) return GPP_OK;
    DownscaleCall call((size_t)igrid->n, values, out, (size_t)nt * nq, mem);   // bilinear.cpp:37-39
    if(call.done) return GPP_OK;
    InField v;
    v.bind(values, (size_t)nt * igrid->n, mem);
    to->to_device();
    to->latlon_to_device();
    igrid->latlon_to_device();
    DevBuf<int> idx;
    idx.get(nq);
    gpp_nearest_device(igrid, to->d_x.p, to->d_y.p, to->d_z.p, nq, 1, idx.p);
    launch(k_bilinear, blocks_of(nq), 256, 0, igrid->d_lat.p, igrid->d_lon.p, igrid->ny, igrid->nx, idx.p, to->d_lat.p, to->d_lon.p, nq, v.d, nt, call.o.d, call.err);
    call.finish();
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_grid_get_box(gpp_points* grid, const float* qlats, const float* qlons, int nq, int* inside, int* boxes) {
    GPP_TRY
    ensure_device();
    if(!grid) invalid("grid is NULL");
    if(nq < 0) invalid("nq < 0");
    if(nq == 0) return GPP_OK;
    if(grid->n == 0) {
        for(int i = 0; i < nq; i++) { inside[i] = 0; for(int k = 0; k < 4; k++) boxes[4 * i + k] = -1; }
        return GPP_OK;
    }
    std::vector<float> qx(nq), qy(nq), qz(nq);
    if(gpp_convert_coordinates(qlats, qlons, nq, grid->type, qx.data(), qy.data(), qz.data()) != GPP_OK) return GPP_EINVAL;
    DevBuf<float> dx, dy, dz, dlat, dlon;
    DevBuf<int> idx, box;
    dx.upload(qx.data(), nq); dy.upload(qy.data(), nq); dz.upload(qz.data(), nq);
    dlat.upload(qlats, nq); dlon.upload(qlons, nq);
    idx.get(nq); box.get((size_t)5 * nq);
    grid->latlon_to_device();
    gpp_nearest_device(grid, dx.p, dy.p, dz.p, nq, 1, idx.p);
    launch(k_get_box, blocks_of(nq), 256, 0, grid->d_lat.p, grid->d_lon.p, grid->ny, grid->nx, idx.p, dlat.p, dlon.p, nq, box.p);
    std::vector<int> h((size_t)5 * nq);
    GPP_HIP(hipMemcpyAsync(h.data(), box.p, sizeof(int) * h.size(), hipMemcpyDeviceToHost, stream()));
    GPP_HIP(hipStreamSynchronize(stream()));
    for(int i = 0; i < nq; i++) { inside[i] = h[5 * i]; for(int k = 0; k < 4; k++) boxes[4 * i + k] = h[5 * i + 1 + k]; }
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_point_in_rectangle(const float corners_latlon[8], float lat, float lon, int* inside) {
    GPP_TRY
    ensure_device();
    if(!corners_latlon || !inside) invalid("NULL argument");
    float h[10];
    memcpy(h, corners_latlon, 8 * sizeof(float));
    h[8] = lat; h[9] = lon;
    DevBuf<float> d;
    DevBuf<int> r;
    d.upload(h, 10);
    r.get(1);
    launch(k_in_rectangle, 1, 1, 0, d.p, r.p);
    GPP_HIP(hipMemcpyAsync(inside, r.p, sizeof(int), hipMemcpyDeviceToHost, stream()));
    GPP_HIP(hipStreamSynchronize(stream()));
    return GPP_OK;
    GPP_CATCH
}
