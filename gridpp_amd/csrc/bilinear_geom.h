// The box search and the weights of gridpp::bilinear, shared by the direct locator (downscale_loc.h), k_get_box (bilinear.hip)
// and k_plan_build (downscale_plan.hip): Grid::get_box (src/api/grid.cpp:149-229), point_in_rectangle (src/api/util.cpp:561-582) and the
// weights / interpolation of src/api/bilinear.cpp:137-320.  Every float expression keeps the reference's association
// (the build has -ffp-contract=off and correctly rounded float divide).  Internal linkage: each translation unit has
// its own device code object.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float edge_side(float plat, float plon, float qlat, float qlon, float mlat, float mlon) {
    const float vlon = qlon - plon;
    const float vlat = -1.0f * (qlat - plat);
    const float c = -1.0f * (vlat * plon + vlon * plat);
    return (vlat * mlon + vlon * mlat) + c;
}
// util.cpp:571-582
__device__ __forceinline__ bool in_rectangle(float alat, float alon, float blat, float blon, float clat, float clon, float dlat,
                                             float dlon, float mlat, float mlon) {
    const float d1 = edge_side(alat, alon, blat, blon, mlat, mlon);
    const float d2 = edge_side(alat, alon, dlat, dlon, mlat, mlon);
    const float d3 = edge_side(blat, blon, clat, clon, mlat, mlon);
    const float d4 = edge_side(clat, clon, dlat, dlon, mlat, mlon);
    const bool cw = 0 >= d1 && 0 >= d4 && 0 <= d2 && 0 >= d3;
    const bool ccw = 0 <= d1 && 0 <= d4 && 0 >= d2 && 0 <= d3;
    return cw || ccw;
}

// grid.cpp:149-229; box = (Y1, X1, Y2, X2), all -1 when the point is in none of the four quadrants
__device__ bool get_box(const float* __restrict__ glat, const float* __restrict__ glon, int nY, int nX, int nn, float lat,
                        float lon, int& Y1, int& X1, int& Y2, int& X2) {
    Y1 = Y2 = X1 = X2 = -1;
    if(nn < 0 || nX <= 1 || nY <= 1) return false;
    const int Y = nn / nX, X = nn - Y * nX;
    const float alat = glat[nn], alon = glon[nn];
    for(int it = 0; it < 4; ++it) {
        const int xdir = (it & 1) ? 1 : -1;
        const int ydir = (it < 2) ? 1 : -1;
        if((Y == 0 && ydir == -1) || (Y == nY - 1 && ydir == 1) || (X == 0 && xdir == -1) || (X == nX - 1 && xdir == 1)) continue;
        const int b = (Y + ydir) * nX + X, c = b + xdir, d = nn + xdir;
        if(in_rectangle(alat, alon, glat[b], glon[b], glat[c], glon[c], glat[d], glon[d], lat, lon)) {
            X1 = xdir == 1 ? X : X - 1;
            X2 = X1 + 1;
            Y1 = ydir == 1 ? Y : Y - 1;
            Y2 = Y1 + 1;
            return true;
        }
    }
    return false;
}

__device__ __forceinline__ bool in_range(float v) {   // bilinear.cpp:154-157
    const float tol = 0.01f;
    return v >= -tol && v < 1 + tol;
}

// bilinear.cpp:159-267
__device__ void weights_general(float x, float y, float x0, float x1, float x2, float x3, float y0, float y1, float y2, float y3,
                                float& t_out, float& s_out) {
    const double a = -x0 + x2, b = -x0 + x1, c = x0 - x1 - x2 + x3, d = x - x0;     // differences formed in float
    const double e = -y0 + y2, f = -y0 + y1, g = y0 - y1 - y2 + y3, h = y - y0;
    double alpha = NAN, beta = NAN;
    const double Y1 = y1, Y2 = y3, Y3 = y0, Y4 = y2, X1 = x1, X2 = x3, X3 = x0, X4 = x2;
    const double X31 = X3 - X1, X21 = X2 - X1, Y42 = Y4 - Y2, Y21 = Y2 - Y1, Y31 = Y3 - Y1, Y43 = Y4 - Y3, X42 = X4 - X2,
                 X43 = X4 - X3;
    const double qa = 2 * c * e - 2 * a * g, qb = 2 * c * f - 2 * b * g;
    const double lin1 = b * e - a * f + d * g - c * h, lin2 = b * e - a * f - d * g + c * h;
    const double root = sqrt(-4 * (c * e - a * g) * (d * f - b * h) + lin1 * lin1);
    if(qa != 0 && qb != 0) {
        alpha = -(lin1 + root) / qa;
        beta = (lin2 + root) / qb;
        if(!in_range((float)alpha)) alpha = -(lin1 - root) / qa;
        if(!in_range((float)beta)) beta = (lin2 - root) / qb;
    }
    else if(qb == 0) {
        alpha = -(lin1 + root) / qa;
        if(!in_range((float)alpha)) alpha = -(lin1 - root) / qa;
        const float s = (float)alpha;
        float t;
        if(Y3 + Y43 * s - Y1 - Y21 * s == 0) t = (float)((x - X1 - X21 * s) / (X3 + X43 * s - X1 - X21 * s));
        else t = (float)((y - Y1 - Y21 * s) / (Y3 + Y43 * s - Y1 - Y21 * s));
        beta = 1 - t;
    }
    else {   // qa == 0
        beta = (lin2 + root) / qb;
        const float t = (float)(1 - beta);
        float s;
        if(Y2 + Y42 * t - Y1 - Y31 * t == 0) s = (float)((x - X1 - X31 * t) / (X2 + X42 * t - X1 - X31 * t));
        else s = (float)((y - Y1 - Y31 * t) / (Y2 + Y42 * t - Y1 - Y31 * t));
        alpha = s;
    }
    s_out = (float)alpha;
    t_out = (float)(1 - beta);
}

// bilinear.cpp:269-313: true when (s, t) end up outside [0, 1] (the reference throws there)
__device__ bool weights(float x, float y, float x0, float x1, float x2, float x3, float y0, float y1, float y2, float y3,
                        float& s, float& t) {
    const float Y1 = y1, Y2 = y3, Y3 = y0, Y4 = y2, X1 = x1, X2 = x3, X3 = x0, X4 = x2;
    const bool vertical = (double)fabsf((X3 - X1) * (Y4 - Y2) - (X4 - X2) * (Y3 - Y1)) <= 1e-4;
    const bool horizontal = (double)fabsf((X2 - X1) * (Y4 - Y3) - (X4 - X3) * (Y2 - Y1)) <= 1e-4;
    if(vertical && horizontal) {   // bilinear.cpp:138-153
        const float A = X2 - X1, B = X3 - X1, C = Y2 - Y1, D = Y3 - Y1;
        const float det = 1 / (A * D - B * C);
        s = det * ((x - X1) * (D) + (y - Y1) * (-B));
        t = det * ((x - X1) * (-C) + (y - Y1) * (A));
    }
    else weights_general(x, y, x0, x1, x2, x3, y0, y1, y2, y3, t, s);
    if(t >= 1 && (double)t <= 1.15) t = 1;
    if(t <= 0 && (double)t >= -0.15) t = 0;
    if(s >= 1 && (double)s <= 1.15) s = 1;
    if(s <= 0 && (double)s >= -0.15) s = 0;
    return !(s >= 0 && s <= 1 && t >= 0 && t <= 1);
}

// bilinear.cpp:137-153 with the corners as get_box names them: v0 = (Y1, X1), v1 = (Y2, X1), v2 = (Y1, X2), v3 = (Y2, X2)
__device__ __forceinline__ float bilinear_value(float v0, float v1, float v2, float v3, float s, float t) {
    const float P1 = v1, P2 = v3, P3 = v0, P4 = v2;
    return P1 * (1 - s) * (1 - t) + P2 * s * (1 - t) + P3 * (1 - s) * t + P4 * s * t;
}

}   // namespace
