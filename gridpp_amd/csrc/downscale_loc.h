// An output location of a downscaling call and d(f), "field f downscaled at this location", for gfx950: what nearest / bilinear give
// for field f alone.  For Bilinear the field is interpolated with the location's weights where its four corners are all valid and
// takes the nearest grid point's value otherwise (bilinear.cpp:322-403), so the fields of one call may mix the two at one location;
// a box whose weights leave [0, 1] is flagged in `err` the first time a field has four valid corners there (bilinear.cpp:309-313).
//
// Two locators share one interface, `float down(const float* f)` and `bool may_still_raise() const`:
//   DirectLoc    found in the call itself (bilinear.hip, downscale.hip): the nearest grid point, the box of Grid::get_box and the
//                weights (s, t), solved lazily by the first field that needs them.
//   PlannedLoc   read from the record of a plan (downscale_plan.hip), whose weights were solved at construction.
// and the bodies written against it once: the level loop of bilinear, the combination of simple_gradient / full_gradient and the
// part of it that does not depend on the level or member.  Internal linkage, as bilinear_geom.h.
#pragma once
#include "bilinear_geom.h"

namespace {

// err[0] = 1 when a box is too distorted, err[1..2] = bits of one offending (s, t)
__device__ __forceinline__ void flag_distorted(int* __restrict__ err, const float s, const float t) {
    if(atomicCAS(&err[0], 0, 1) == 0) { err[1] = __float_as_int(s); err[2] = __float_as_int(t); }
}

template <bool BIL>
struct DirectLoc {
    const float* glat; const float* glon;
    int* err;
    int n0, i0, i1, i2, i3;   // the nearest grid point (-1: none) and the corners (Y1, X1), (Y2, X1), (Y1, X2), (Y2, X2) of the box
    float lat = 0, lon = 0, s = 0, t = 0;
    bool inside = false, solved = false;
    // nn: the nearest grid point of every location; the box is searched for Bilinear only
    __device__ __forceinline__ DirectLoc(const float* __restrict__ glat_, const float* __restrict__ glon_, const int nY, const int nX,
                                         const int* __restrict__ nn, const float* __restrict__ qlat, const float* __restrict__ qlon,
                                         const int q, int* __restrict__ err_) : glat(glat_), glon(glon_), err(err_), n0(nn[q]) {
        int I1 = -1, J1 = -1, I2 = -1, J2 = -1;
        if(BIL) {
            lat = qlat[q]; lon = qlon[q];
            inside = get_box(glat, glon, nY, nX, n0, lat, lon, I1, J1, I2, J2);
        }
        i0 = I1 * nX + J1; i1 = I2 * nX + J1; i2 = I1 * nX + J2; i3 = I2 * nX + J2;
    }
    __device__ __forceinline__ float down(const float* __restrict__ f) {
        if(BIL && inside) {
            const float v0 = f[i0], v1 = f[i1], v2 = f[i2], v3 = f[i3];
            if(dev_valid(v0) && dev_valid(v1) && dev_valid(v2) && dev_valid(v3)) {
                if(!solved) {
                    const bool bad = weights(lon, lat, glon[i0], glon[i1], glon[i2], glon[i3], glat[i0], glat[i1], glat[i2], glat[i3], s, t);
                    solved = true;
                    if(bad) flag_distorted(err, s, t);
                }
                return bilinear_value(v0, v1, v2, v3, s, t);
            }
        }
        // outside the domain or a missing corner: nearest neighbour (bilinear.cpp:346-356)
        return n0 >= 0 ? f[n0] : NAN;   // (-1: a location the search cannot rank; Points / Grid refuse NaN coordinates, "Invalid coords")
    }
    // a field not downscaled yet may still be the one that flags this location
    __device__ __forceinline__ bool may_still_raise() const { return BIL && inside && !solved; }
};

// V consecutive members of a cell as one access (down_members and the cube kernels of a plan)
template <int V> struct VecOf;
template <> struct VecOf<1> { using type = float; };
template <> struct VecOf<2> { using type = float2; };

// A record of a plan in registers (downscale_plan.hip describes the records).  c >= 0: corner (Y1, X1) of the box; `bad`: its
// weights leave [0, 1].  get_box always returns Y2 = Y1 + 1 and X2 = X1 + 1, so the other corners are c + nX, c + 1 and c + nX + 1.
template <bool BIL>
struct PlannedLoc {
    int* err;
    int n0, c = -1, nX;
    float s = 0, t = 0;
    bool inside = false, bad = false, flagged = false;
    // rec: the records of a Bilinear plan; nn: the index of a Nearest plan
    __device__ __forceinline__ PlannedLoc(const int4* __restrict__ rec, const int* __restrict__ nn, const int q, const int nX_,
                                          int* __restrict__ err_) : err(err_), nX(nX_) {
        if(BIL) {
            const int4 r = rec[q];
            n0 = r.x;
            inside = r.y != -1;
            bad = r.y < -1;
            c = bad ? -2 - r.y : r.y;
            s = __int_as_float(r.z); t = __int_as_float(r.w);
        }
        else n0 = nn[q];
    }
    // the value of a field with corners v0 = (Y1, X1), v1 = (Y2, X1), v2 = (Y1, X2), v3 = (Y2, X2) at a location inside that box
    __device__ __forceinline__ float in_box(const float v0, const float v1, const float v2, const float v3) {
        if(dev_valid(v0) && dev_valid(v1) && dev_valid(v2) && dev_valid(v3)) {
            if(bad && !flagged) { flag_distorted(err, s, t); flagged = true; }
            return bilinear_value(v0, v1, v2, v3, s, t);
        }
        const int d = n0 - c;   // a missing corner: the nearest grid point, one of the four, from the registers
        return d == 0 ? v0 : d == nX ? v1 : d == 1 ? v2 : v3;
    }
    // a level of (T, Y, X)
    __device__ __forceinline__ float down(const float* __restrict__ f) {
        if(BIL && inside) return in_box(f[c], f[c + nX], f[c + 1], f[c + nX + 1]);
        return n0 >= 0 ? f[n0] : NAN;   // outside the domain: nearest neighbour
    }
    // members e ... e + V - 1 of a cube [n_in][E]: every corner is one V-float access, the four-corner validity test is per member
    template <int V>
    __device__ __forceinline__ void down_members(const float* __restrict__ f, const int E, const int e, float (&r)[V]) {
        using vec = typename VecOf<V>::type;
        union { vec v; float f[V]; } a0, a1, a2, a3;
        if(BIL && inside) {
            const float* __restrict__ p = f + (size_t)c * E + e;
            a0.v = *reinterpret_cast<const vec*>(p); a1.v = *reinterpret_cast<const vec*>(p + (size_t)nX * E);
            a2.v = *reinterpret_cast<const vec*>(p + E); a3.v = *reinterpret_cast<const vec*>(p + (size_t)(nX + 1) * E);
#pragma unroll
            for(int u = 0; u < V; ++u) r[u] = in_box(a0.f[u], a1.f[u], a2.f[u], a3.f[u]);
        }
        else if(n0 >= 0) {   // outside the domain: nearest neighbour
            a0.v = *reinterpret_cast<const vec*>(f + (size_t)n0 * E + e);
#pragma unroll
            for(int u = 0; u < V; ++u) r[u] = a0.f[u];
        }
        else {
#pragma unroll
            for(int u = 0; u < V; ++u) r[u] = NAN;
        }
    }
    __device__ __forceinline__ bool may_still_raise() const { return BIL && bad && !flagged; }
};

// values [nt][n_in] -> out [nt][nq]: the levels of one location, unit-stride writes across the lanes of a wavefront per level
template <class L>
__device__ __forceinline__ void down_levels(L& l, const float* __restrict__ values, const size_t n_in, const int nt,
                                            float* __restrict__ out, const size_t nq, const int q) {
    for(int k = 0; k < nt; ++k) out[(size_t)k * nq + q] = l.down(values + (size_t)k * n_in);
}

// What the gradient kernels share whatever the layout of their fields
struct GradientFields {
    const float* values; const float* egrad; const float* lgrad;   // egrad / lgrad NULL = term absent
    const float* ielev; const float* ilaf;                         // input grid [n_in]
    const float* oelev; const float* olaf;                         // output locations [nq]
    float elev_gradient;                                           // simple_gradient's scalar
    int full;                                                      // 0: simple_gradient, 1: full_gradient
    float* out;
    int* err;
};

// A term of full_gradient at a location, the part that depends on no level or member (gradient.cpp:56-81): the term counts where the
// output's and the downscaled input's elevation (laf) are both valid, and multiplies their difference
struct GradientTerm {
    bool use = false;
    float diff = 0;
};
template <class L>
__device__ __forceinline__ GradientTerm gradient_term(L& l, const float* __restrict__ ofield, const float* __restrict__ ifield, const int q) {
    GradientTerm g;
    const float o = ofield[q], i = l.down(ifield);
    g.use = dev_valid(o) && dev_valid(i);
    g.diff = o - i;
    return g;
}
// ... and its correction from the gradient field.  A gradient whose term is switched off at a location is still downscaled by the
// reference and may raise there: its corners are read only where that could still happen
template <class L>
__device__ __forceinline__ float gradient_corr(L& l, const GradientTerm& g, const float* __restrict__ gradient) {
    if(g.use) return l.down(gradient) * g.diff;
    if(l.may_still_raise()) (void)l.down(gradient);
    return 0;
}

// simple_gradient / full_gradient of the levels of one location: values, egrad, lgrad [nt][n_in] -> out [nt][nq]
template <class L>
__device__ __forceinline__ void gradient_levels(L& l, const GradientFields& a, const size_t n_in, const int nt, const size_t nq, const int q) {
    if(!a.full) {   // simple_gradient.cpp: out = d(values) + (oelev - d(ielevs)) * elev_gradient, no validity test
        const float elev_corr = (a.oelev[q] - l.down(a.ielev)) * a.elev_gradient;
        for(int k = 0; k < nt; ++k) a.out[(size_t)k * nq + q] = l.down(a.values + (size_t)k * n_in) + elev_corr;
        return;
    }
    GradientTerm e, lf;
    if(a.egrad) e = gradient_term(l, a.oelev, a.ielev, q);
    if(a.lgrad) lf = gradient_term(l, a.olaf, a.ilaf, q);
    for(int k = 0; k < nt; ++k) {
        const size_t off = (size_t)k * n_in;
        const float v = l.down(a.values + off);
        float laf_corr = 0, elev_corr = 0;
        if(a.lgrad) laf_corr = gradient_corr(l, lf, a.lgrad + off);
        if(a.egrad) elev_corr = gradient_corr(l, e, a.egrad + off);
        a.out[(size_t)k * nq + q] = v + (laf_corr + elev_corr);
    }
}

}   // namespace
