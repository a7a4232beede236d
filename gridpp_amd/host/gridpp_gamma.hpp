// gridpp::gamma_inv and gridpp::Gamma (include/gridpp.h:573,2438-2455 of the reference, minus the Boost members) on libgridpp_hip.so.
//
// A header of its own, not part of gridpp.hpp: where the reference raises through Boost's error policies (a level of 1, a value below
// -tolerance, a cdf that rounds to 0 or 1 in float32) these return IEEE values -- +inf, NaN, -inf / +inf.  A program
// written for the reference that relies on those exceptions does not get them, so it has to ask for this header by name.
#pragma once
#include "gridpp.hpp"

namespace gridpp {

/** Extract quantiles from a gamma distribution (src/api/distribution.cpp:5-33)
 *  @param levels Quantile levels to retrieve, on [0, 1]
 *  @param shape Shape parameter of each distribution, > 0
 *  @param scale Scale parameter of each distribution, > 0
 *  The reference reads levels[i] and scale[i] up to shape.size() without comparing the sizes; here unequal sizes are an
 *  std::invalid_argument. */
inline vec gamma_inv(const vec& levels, const vec& shape, const vec& scale) {
    if(levels.size() != shape.size() || scale.size() != shape.size()) throw std::invalid_argument("gamma_inv: levels, shape and scale must be of the same size");
    vec out(shape.size(), MV);
    detail::check(gpp_gamma_inv(levels.data(), shape.data(), scale.data(), (long long)out.size(), out.data(), GPP_MEM_HOST));
    return out;
}

/** Gamma transformation. Transforms values to cdf from a gamma distribution and subsequantly extracts the cdf from a standard normal
 *  distribution (src/api/transform.cpp:155-179). */
class Gamma : public Transform {
    public:
        Gamma(float shape, float scale, float tolerance = 0.01) : m_shape(shape), m_scale(scale), m_tolerance(tolerance) {   // transform.cpp:155-165
            if(!is_valid(shape) || shape <= 0) throw std::invalid_argument("Shape parameter must be > 0 in the gamma distribution");
            if(!is_valid(scale) || scale <= 0) throw std::invalid_argument("Scale parameter must be > 0 in the gamma distribution");
            if(!is_valid(tolerance) || tolerance < 0) throw std::invalid_argument("Tolerance must be >= 0 in the gamma distribution");
        }
        using Transform::forward;
        using Transform::backward;
        float forward(float value) const { return scalar(value, 0); }
        float backward(float value) const { return scalar(value, 1); }
    protected:
        vec apply(const vec& input, int backward) const {
            vec out(input.size(), MV);
            detail::check(gpp_gamma_transform(input.data(), (long long)input.size(), backward, m_shape, m_scale, m_tolerance, out.data(), GPP_MEM_HOST));
            return out;
        }
    private:
        float m_shape, m_scale, m_tolerance;
        float scalar(float value, int backward) const {
            float out = MV;
            detail::check(gpp_gamma_transform_scalar(value, backward, m_shape, m_scale, m_tolerance, &out));
            return out;
        }
};

}   // namespace gridpp
