// gridpp::get_optimal_threshold and gridpp::metric_optimizer_curve (include/gridpp.h, src/api/metric_optimizer.cpp:105-184 of the
// reference) on libgridpp_hip.so.
//
// A header of its own, not part of gridpp.hpp: the reference minimises with Boost's brent_find_minima and returns whichever point of
// whichever plateau of the piecewise-constant score that search ends on; these return the exact optimum over all plateaus -- the midpoint
// of the lowest run of plateaus with the largest valid score, behind the reference's own filters.  That is never a worse
// score, but it is another number, so a program written for the reference has to ask for this header by name.
#pragma once
#include "gridpp.hpp"

namespace gridpp {

/** Compute the optimal forecast threshold for a given reference threshold
 *  @param ref Reference values (a ref shorter than fcst is read out of bounds by the reference: std::invalid_argument here)
 *  @param fcst Forecast values
 *  @param threshold Threshold for the reference values
 *  @param metric A Metric to optimize for
 *  @return The forecast threshold with the largest score; MV where the reference's filters reject it */
inline float get_optimal_threshold(const vec& ref, const vec& fcst, float threshold, Metric metric) {
    if(ref.size() < fcst.size()) throw std::invalid_argument("ref and fcst not the same size");
    float out = MV;
    detail::check(gpp_get_optimal_threshold(ref.data(), fcst.data(), (long long)fcst.size(), threshold, (int)metric, &out, GPP_MEM_HOST));
    return out;
}

/** Create a calibration curve that optimizes a metric (src/api/metric_optimizer.cpp:105-127)
 *  @param ref Reference values
 *  @param fcst Forecast values
 *  @param thresholds Thresholds for which to optimize
 *  @param metric A Metric to optimize for
 *  @param output_fcst Output: the thresholds with a valid optimum (the reference's naming)
 *  @return The optimal forecast threshold of each of them */
inline vec metric_optimizer_curve(const vec& ref, const vec& fcst, const vec& thresholds, Metric metric, vec& output_fcst) {
    if(ref.size() != fcst.size()) throw std::invalid_argument("ref and fcst not the same size");
    vec output_ref(thresholds.size(), MV);
    output_fcst.assign(thresholds.size(), MV);
    int count = 0;
    detail::check(gpp_metric_optimizer_curve(ref.data(), fcst.data(), (long long)fcst.size(), thresholds.data(), (int)thresholds.size(), (int)metric,
                                             output_ref.data(), output_fcst.data(), &count, GPP_MEM_HOST));
    output_ref.resize((size_t)count);
    output_fcst.resize((size_t)count);
    return output_ref;
}

}   // namespace gridpp
