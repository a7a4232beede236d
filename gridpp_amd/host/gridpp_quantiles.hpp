// calc_quantiles and quantile_mapping_curves on libgridpp_hip.so: many quantiles of every row from one sort, and one quantile-mapping
// curve per cell for apply_curve(vec2, vec3, vec3, ...).
//
// A header of its own, not part of gridpp.hpp: the reference has neither function (its quantile_mapping_curve is 1-D, and with quantiles it
// indexes into the inputs as given, src/api/quantile_mapping.cpp:41-42), so a program written for the reference has to ask for this header
// by name.  Every value is, bit for bit, what calc_quantile of gridpp.hpp returns for that row and level.
#pragma once
#include "gridpp.hpp"

namespace gridpp {

namespace detail {
inline void check_levels(const vec& quantiles) {   // (NaN passes and gives NaN)
    for(float q : quantiles)
        if(q < 0 || q > 1) throw std::invalid_argument("calc_quantiles: Quantiles must be between 0 and 1 inclusive");
}
// rows x len values -> rows x quantiles.size() results
inline vec rows_quantiles(const vec& f, size_t rows, size_t len, const vec& quantiles) {
    vec out(rows * quantiles.size(), MV);
    if(rows && !quantiles.empty())
        check(gpp_calc_quantiles(f.data(), (long)rows, (int)len, quantiles.data(), (int)quantiles.size(), out.data(), GPP_MEM_HOST));
    return out;
}
}   // namespace detail

/** The quantiles of one vector
 *  @param array Input values (invalid values are skipped)
 *  @param quantiles Levels in [0, 1], in any order, repeats allowed (std::invalid_argument outside; a NaN level gives NaN)
 *  @return One value per level: calc_quantile(array, quantiles[j]) */
inline vec calc_quantiles(const vec& array, const vec& quantiles) {
    detail::check_levels(quantiles);
    return detail::rows_quantiles(array, 1, array.size(), quantiles);
}

/** The quantiles of every row; rows of different lengths are padded with NaN to the longest, as calc_quantile(vec2) does
 *  @return [row][level] */
inline vec2 calc_quantiles(const vec2& array, const vec& quantiles) {
    detail::check_levels(quantiles);
    size_t len;
    const vec f = detail::pad_rows(array, len);
    return detail::unflatten(detail::rows_quantiles(f, array.size(), len, quantiles), array.size(), quantiles.size());
}

/** The quantiles of every cell of a cube (Y, X, N)
 *  @return [y][x][level] */
inline vec3 calc_quantiles(const vec3& array, const vec& quantiles) {
    detail::check_levels(quantiles);
    size_t Y, X, E;
    const vec f = detail::flatten(array, Y, X, E);
    return detail::unflatten(detail::rows_quantiles(f, Y * X, E, quantiles), Y, X, quantiles.size());
}

/** One quantile-mapping curve per cell, ready for apply_curve(vec2, vec3, vec3, ...).  True quantiles of each cell's valid values, unlike
 *  the 1-D quantile_mapping_curve, which indexes into the inputs as given (src/api/quantile_mapping.cpp:41-42).
 *  @param ref Reference values (Y, X, Tr)
 *  @param fcst Forecast values (Y, X, Tf); Tr and Tf may differ
 *  @param output_fcst Output: the forecast curves (Y, X, Q)
 *  @param quantiles Levels in [0, 1], at least one, none of them NaN
 *  @return The reference curves (Y, X, Q) */
inline vec3 quantile_mapping_curves(const vec3& ref, const vec3& fcst, vec3& output_fcst, const vec& quantiles) {
    if(ref.size() != fcst.size() || (ref.size() && ref[0].size() != fcst[0].size()))
        throw std::invalid_argument("quantile_mapping_curves: ref and fcst must have the same first two dimensions");
    if(quantiles.empty()) throw std::invalid_argument("quantile_mapping_curves: empty quantiles: the sorted-rows form is not built");
    for(float q : quantiles)
        if(!(q >= 0 && q <= 1)) throw std::invalid_argument("Quantiles must be >= 0 and <= 1");
    output_fcst = calc_quantiles(fcst, quantiles);
    return calc_quantiles(ref, quantiles);
}

}   // namespace gridpp
