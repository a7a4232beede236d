// neighbourhood_members and calc_gradient_members on libgridpp_hip.so: a spatial filter and the gradient of every member of a (Y, X, E) cube,
// without a permute of the cube.
//
// A header of its own, not part of gridpp.hpp: the reference has neither function (its neighbourhood(vec3) pools the members into one field and
// its calc_gradient takes two 2-D fields), so a program written for the reference has to ask for this header by name.  Plane e of a result is,
// on exact data bit for bit, what neighbourhood / calc_gradient of gridpp.hpp return for plane e.
#pragma once
#include "gridpp.hpp"

namespace gridpp {

namespace detail {
inline void check_members_statistic(Statistic statistic) {
    if(statistic == Quantile) throw std::invalid_argument("Use neighbourhood_quantile for computing neighbourhood quantiles");
    if(statistic == Median) throw std::invalid_argument("neighbourhood_members does not compute the statistic Median: order statistics per member are not supported");
    if(statistic == RandomChoice)
        throw std::invalid_argument("neighbourhood_members does not compute the statistic RandomChoice: order statistics per member are not supported");
}
inline vec3 gradient_members(const vec& b, size_t Yb, size_t Xb, size_t Eb, bool base3d, const vec3& values, GradientType gradient_type, int halfwidth, int min_num,
                             float min_range, float default_gradient) {
    size_t Y, X, E;
    const vec v = flatten(values, Y, X, E);
    if(halfwidth <= 0) throw std::invalid_argument("Halwidth cannot be <= 0; must be positive integer");
    if(is_valid(min_range) && min_range < 0) throw std::invalid_argument("min_range must be >= 0");
    if(min_num < 0) throw std::invalid_argument("num_min must be >= 0");
    if(Yb == 0) throw std::invalid_argument("base input has no size");
    if(Yb != Y || Xb != X || (base3d && Eb != E)) throw std::invalid_argument("base is not the same size as values");
    vec out(v.size(), MV);
    check(gpp_calc_gradient_members(b.data(), base3d ? (int)E : 1, v.data(), (int)Y, (int)X, (int)E, (int)gradient_type, halfwidth, min_num, min_range,
                                    default_gradient, out.data(), GPP_MEM_HOST));
    return unflatten(out, Y, X, E);
}
}   // namespace detail

/** A spatial filter of every member: plane e of the result is neighbourhood(plane e of input, halfwidth, statistic)
 *  @param input Cube (Y, X, E)
 *  @param halfwidth Neighbourhood halfwidth, >= 0 (std::invalid_argument below; windows wider than the field are clipped to it)
 *  @param statistic Mean, Sum, Count, Min, Max, Std or Variance (std::invalid_argument for Median, RandomChoice and Quantile)
 *  @return [y][x][e]; NaN where the window of the member holds no valid value (Count: 0) */
inline vec3 neighbourhood_members(const vec3& input, int halfwidth, Statistic statistic) {
    size_t Y, X, E; const vec f = detail::flatten(input, Y, X, E);
    if(halfwidth < 0) throw std::invalid_argument("Half width must be > 0");
    detail::check_members_statistic(statistic);
    if(Y == 0 || X == 0 || E == 0) return vec3();
    vec out(f.size(), MV);
    detail::check(gpp_neighbourhood_members(f.data(), (int)Y, (int)X, (int)E, halfwidth, (int)statistic, out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, Y, X, E);
}

/** calc_gradient of every member: plane e of the result is calc_gradient(base, plane e of values, ...), base shared by the members
 *  @param base Field (Y, X), e.g. the elevation
 *  @param values Cube (Y, X, E)
 *  @return [y][x][e]; the checks and their messages are calc_gradient's */
inline vec3 calc_gradient_members(const vec2& base, const vec3& values, GradientType gradient_type, int halfwidth, int min_num = 2, float min_range = MV,
                                  float default_gradient = 0) {
    size_t Y, X; const vec b = detail::flatten(base, Y, X);
    return detail::gradient_members(b, Y, X, 1, false, values, gradient_type, halfwidth, min_num, min_range, default_gradient);
}
/** ... with a base field per member: plane e of the result is calc_gradient(plane e of base, plane e of values, ...) */
inline vec3 calc_gradient_members(const vec3& base, const vec3& values, GradientType gradient_type, int halfwidth, int min_num = 2, float min_range = MV,
                                  float default_gradient = 0) {
    size_t Y, X, E; const vec b = detail::flatten(base, Y, X, E);
    return detail::gradient_members(b, Y, X, E, true, values, gradient_type, halfwidth, min_num, min_range, default_gradient);
}

/** The device-pointer forms: `input` / `values` / `out` [Y][X][E] and `base` ([Y][X] where base_members == 1, [Y][X][E] where base_members == E) are
 *  in HBM.  The calls return when the result is complete. */
inline void neighbourhood_members_device(const float* input, int Y, int X, int E, int halfwidth, Statistic statistic, float* out) {
    detail::check(gpp_neighbourhood_members(input, Y, X, E, halfwidth, (int)statistic, out, GPP_MEM_DEVICE));
}
inline void calc_gradient_members_device(const float* base, int base_members, const float* values, int Y, int X, int E, GradientType gradient_type, int halfwidth,
                                         int min_num, float min_range, float default_gradient, float* out) {
    detail::check(gpp_calc_gradient_members(base, base_members, values, Y, X, E, (int)gradient_type, halfwidth, min_num, min_range, default_gradient, out,
                                            GPP_MEM_DEVICE));
}

}   // namespace gridpp
