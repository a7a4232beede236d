// neighbourhood_quantiles_fast and neighbourhood_cdf on libgridpp_hip.so: many levels of neighbourhood_quantile_fast from one pass over the
// cube, and the per-threshold neighbourhood probabilities it interpolates in.
//
// A header of its own, not part of gridpp.hpp: the reference has neither function (it computes the probabilities -- `yarray`,
// src/api/neighbourhood.cpp:490-509 -- per cell and throws them away), so a program written for the reference has to ask for this header by
// name.  Every level plane is, bit for bit, what neighbourhood_quantile_fast of gridpp.hpp returns for that level.
#pragma once
#include "gridpp.hpp"

namespace gridpp {

namespace detail {
inline vec3 nbh_quantiles(const vec& f, size_t Y, size_t X, size_t E, int is3d, const vec& quantiles, int halfwidth, const vec& thresholds) {
    if(halfwidth < 0) throw std::invalid_argument("Half width must be > 0");
    if(Y == 0 || X == 0 || E == 0) return vec3();
    vec out(Y * X * quantiles.size(), MV);
    check(gpp_neighbourhood_quantiles_fast(f.data(), (int)Y, (int)X, (int)E, is3d, quantiles.data(), (int)quantiles.size(), halfwidth, thresholds.data(),
                                           (int)thresholds.size(), out.data(), GPP_MEM_HOST));
    return unflatten(out, Y, X, quantiles.size());
}
inline vec3 nbh_cdf(const vec& f, size_t Y, size_t X, size_t E, int is3d, const vec& thresholds, int halfwidth) {
    if(halfwidth < 0) throw std::invalid_argument("Half width must be > 0");
    if(Y == 0 || X == 0 || E == 0) return vec3();
    vec out(Y * X * thresholds.size(), MV);
    check(gpp_neighbourhood_cdf(f.data(), (int)Y, (int)X, (int)E, is3d, halfwidth, thresholds.data(), (int)thresholds.size(), out.data(), GPP_MEM_HOST));
    return unflatten(out, Y, X, thresholds.size());
}
}   // namespace detail

/** Many levels of neighbourhood_quantile_fast: the member pass and the window sums run once for all of them
 *  @param input Field (Y, X) or cube (Y, X, E)
 *  @param quantiles Scalar levels in [0, 1], in any order, repeats allowed (std::invalid_argument outside; a NaN level gives a NaN plane)
 *  @param halfwidth Neighbourhood halfwidth, >= 0
 *  @param thresholds The thresholds the quantile is interpolated between (none: NaN everywhere)
 *  @return [y][x][level]: neighbourhood_quantile_fast(input, quantiles[j], halfwidth, thresholds), bit for bit */
inline vec3 neighbourhood_quantiles_fast(const vec2& input, const vec& quantiles, int halfwidth, const vec& thresholds) {
    size_t Y, X; const vec f = detail::flatten(input, Y, X);
    return detail::nbh_quantiles(f, Y, X, 1, 0, quantiles, halfwidth, thresholds);
}
inline vec3 neighbourhood_quantiles_fast(const vec3& input, const vec& quantiles, int halfwidth, const vec& thresholds) {
    size_t Y, X, E; const vec f = detail::flatten(input, Y, X, E);
    return detail::nbh_quantiles(f, Y, X, E, 1, quantiles, halfwidth, thresholds);
}

/** P(member <= thresholds[t]) over the window and the members: the curve neighbourhood_quantile_fast interpolates in.  In [0, 1]; NaN where the
 *  window holds no valid cell.  The exceedance probability is 1 - cdf.
 *  @return [y][x][t], for the thresholds as given (unsorted, duplicated and non-finite ones included) */
inline vec3 neighbourhood_cdf(const vec2& input, const vec& thresholds, int halfwidth) {
    size_t Y, X; const vec f = detail::flatten(input, Y, X);
    return detail::nbh_cdf(f, Y, X, 1, 0, thresholds, halfwidth);
}
inline vec3 neighbourhood_cdf(const vec3& input, const vec& thresholds, int halfwidth) {
    size_t Y, X, E; const vec f = detail::flatten(input, Y, X, E);
    return detail::nbh_cdf(f, Y, X, E, 1, thresholds, halfwidth);
}

/** The device-pointer forms: `input` [Y][X][E] (E == 1 and is3d == 0: a 2-D field), `thresholds` [nt] and `out` are in HBM; `quantiles` is a host
 *  array.  out is [Y][X][quantiles.size()] / [Y][X][nt].  The calls return when the result is complete. */
inline void neighbourhood_quantiles_fast_device(const float* input, int Y, int X, int E, bool is3d, const vec& quantiles, int halfwidth,
                                                const float* thresholds, int nt, float* out) {
    detail::check(gpp_neighbourhood_quantiles_fast(input, Y, X, E, is3d ? 1 : 0, quantiles.data(), (int)quantiles.size(), halfwidth, thresholds, nt, out, GPP_MEM_DEVICE));
}
inline void neighbourhood_cdf_device(const float* input, int Y, int X, int E, bool is3d, const float* thresholds, int nt, int halfwidth, float* out) {
    detail::check(gpp_neighbourhood_cdf(input, Y, X, E, is3d ? 1 : 0, halfwidth, thresholds, nt, out, GPP_MEM_DEVICE));
}

}   // namespace gridpp
