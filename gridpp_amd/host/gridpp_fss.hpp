// fractions_skill_score on libgridpp_hip.so: the Fractions Skill Score of a field or an ensemble cube against a reference field for a table of
// thresholds x half widths from one call, with the two sums it is formed from so that scores can be pooled over many cases.
//
// A header of its own, not part of gridpp.hpp: the reference has no such function, so a program written for the reference has to ask for this
// header by name.  DESIGN.md 4.22 holds the definition.
#pragma once
#include "gridpp.hpp"

namespace gridpp {

typedef std::vector<double> dvec;
typedef std::vector<dvec> dvec2;

/** What fractions_skill_score returns.  fss, fbs and fbs_worst are [threshold][half width]; cells is [half width]. */
struct FssResult {
    dvec2 fss;         /**< 1 - fbs / fbs_worst; NaN where fbs_worst == 0 (no event in either field) */
    dvec2 fbs;         /**< sum over the contributing cells of (Ff - Fo)^2 */
    dvec2 fbs_worst;   /**< sum over the contributing cells of Ff^2 + Fo^2 */
    std::vector<long long> cells;   /**< cells whose window holds a counting cell; does not depend on the threshold */
};

namespace detail {
inline FssResult fss(const vec& f, size_t Y, size_t X, size_t E, int is3d, const vec2& ref, const vec& thresholds, const ivec& halfwidths,
                     ComparisonOperator comparison_operator) {
    size_t RY, RX; const vec r = flatten(ref, RY, RX);
    if((RY != Y || RX != X) && !(Y * X == 0 && RY * RX == 0)) throw std::invalid_argument("fractions_skill_score: ref must have the shape (Y, X) of fcst");
    for(float t : thresholds) if(std::isnan(t)) throw std::invalid_argument("fractions_skill_score: a threshold is NaN");
    for(int h : halfwidths) if(h < 0) throw std::invalid_argument("Half width must be > 0");
    if(comparison_operator != Lt && comparison_operator != Leq && comparison_operator != Gt && comparison_operator != Geq)
        throw std::invalid_argument("Invalid comparison operator");
    const size_t T = thresholds.size(), H = halfwidths.size();
    dvec fbs(T * H, 0.0), worst(T * H, 0.0);
    FssResult out;
    out.cells.assign(H, 0);
    if(T != 0 && H != 0 && Y * X * E != 0)
        check(gpp_fractions_skill_score(f.data(), r.data(), (int)Y, (int)X, (int)E, is3d, thresholds.data(), (int)T, halfwidths.data(), (int)H,
                                        (int)comparison_operator, fbs.data(), worst.data(), out.cells.data(), GPP_MEM_HOST));
    out.fss.assign(T, dvec(H));
    out.fbs.assign(T, dvec(H));
    out.fbs_worst.assign(T, dvec(H));
    for(size_t t = 0; t < T; t++)
        for(size_t h = 0; h < H; h++) {
            out.fbs[t][h] = fbs[t * H + h];
            out.fbs_worst[t][h] = worst[t * H + h];
            out.fss[t][h] = GPP_FSS_VALUE(fbs[t * H + h], worst[t * H + h]);
        }
    return out;
}
}   // namespace detail

/** The Fractions Skill Score for every threshold and every half width
 *  @param fcst Forecast field (Y, X), or an ensemble cube (Y, X, E) in the second overload
 *  @param ref Reference field (Y, X)
 *  @param thresholds Thresholds (+-Inf allowed; std::invalid_argument for NaN)
 *  @param halfwidths Neighbourhood half widths, >= 0 (std::invalid_argument for a negative one)
 *  @param comparison_operator How a value is compared with a threshold: `value op threshold`
 *  @return fss, fbs and fbs_worst per [threshold][half width] and cells per half width.  A cell counts where ref is valid and fcst has a
 *  valid member; Ff = K / M is the pooled fraction of valid members of the window's counting cells that meet the threshold, Fo = O / n the
 *  fraction of its counting cells whose ref does.  To pool over cases add the sums: 1 - sum(fbs) / sum(fbs_worst). */
inline FssResult fractions_skill_score(const vec2& fcst, const vec2& ref, const vec& thresholds, const ivec& halfwidths,
                                       ComparisonOperator comparison_operator = Gt) {
    size_t Y, X; const vec f = detail::flatten(fcst, Y, X);
    return detail::fss(f, Y, X, 1, 0, ref, thresholds, halfwidths, comparison_operator);
}
inline FssResult fractions_skill_score(const vec3& fcst, const vec2& ref, const vec& thresholds, const ivec& halfwidths,
                                       ComparisonOperator comparison_operator = Gt) {
    size_t Y, X, E; const vec f = detail::flatten(fcst, Y, X, E);
    return detail::fss(f, Y, X, E, 1, ref, thresholds, halfwidths, comparison_operator);
}

}   // namespace gridpp
