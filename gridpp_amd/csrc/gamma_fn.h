// The gamma distribution's quantile function (gridpp::gamma_inv, src/api/distribution.cpp:5-33) and the Gamma transform
// (src/api/transform.cpp:155-179) for ONE value, written once for the host and the device: the kernels of gamma.hip and the host-only
// scalar entry points (gpp_gamma_inv_scalar, gpp_gamma_transform_scalar) compile this same text.
//
// The reference evaluates boost::math::cdf / quantile of gamma_distribution<> and normal in double and stores the result in a float.
// Away from the edges those are mathematical functions, computed here in double from the published algorithms:
//
//   log_tail      ln of ONE tail of the regularised incomplete gamma function, whichever the method at hand computes directly: the
//                 power series of P(a, x) for x < a + 1, the continued fraction of Q(a, x) by the modified Lentz recurrence otherwise
//                 (Abramowitz & Stegun 6.5.29 / 6.5.31; Lentz 1976, Thompson & Barnett 1986).  The other tail is 1 - exp(ln tail).
//                 Kept as a logarithm so that a tail of 1e-400 still steers the inverse.
//   p_inverse     x with P(a, x) = p.  Guess: Wilson & Hilferty (1931) for a > 1, the two-branch guess of DiDonato & Morris (1986) /
//                 Best & Roberts AS 91 for a <= 1, never below the solution of the series' leading term, which is a lower bound of x
//                 and IS the answer (to 1e-17 relative) where it is below SMALL_X.  Refinement: Newton steps inside a bracket, for
//                 p <= 0.5 (and for a <= 1 with x below about 1) on ln P against ln x (concave and increasing: a power law is solved
//                 in one step), otherwise on ln Q against x with Q's target 1 - p, which is exact in double for a float32 p.  A step
//                 that would leave the bracket is replaced by its midpoint (twice x + 1 while there is no upper end yet).
//   ndtri         the standard normal quantile: Wichura, Algorithm AS 241 (1988), PPND16.
//   ncdf          0.5 * erfc(-z / sqrt 2)
//
// Every loop counts: SERIES_MAX_TERMS, FRACTION_MAX_STEPS, INVERSE_MAX_STEPS.  A loop that reaches its bound leaves with the value it
// has; nothing here can trap, and no input makes it run on.  `work`, where given, receives the trip counts (tools/gamma_trip_counts.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace gpp {
namespace gamma_fn {

#define GPP_GM_HD __host__ __device__ __forceinline__   // (p_inverse as a real call would cost its kernels a stack frame)

// ---- the bounds (DESIGN.md 4.12 derives them for shape <= 1e3, the tested domain) ---------------------------------------------------
constexpr int SERIES_MAX_TERMS = 2048;     // terms of the series of P: sqrt(75 * shape) near x = shape + 1, 272 at shape 1e3
constexpr int FRACTION_MAX_STEPS = 2048;   // steps of the fraction of Q: 108 at most (x near 1, small shapes), fewer at large ones
constexpr int INVERSE_MAX_STEPS = 32;      // Newton / midpoint steps of p_inverse; 5 at most on the tested domain
constexpr double TERM_EPS = 5.5511151231257827e-17;   // 2^-54: a term below this share of the sum ends the series / the fraction
constexpr double LENTZ_TINY = 1e-300;      // a denominator of the Lentz recurrence that vanishes is replaced by this
constexpr double INVERSE_TOL = 1e-10;      // a Newton step below this (relative) is the last: the step after it would be ~1e-20
constexpr double LOG_SMALL_X = -39.14394658089878;    // ln 1e-17 (SMALL_X): below it P(a, x) = x^a / Gamma(a + 1) to 1e-17 relative
constexpr double HUGE_X = 1e300;           // from here on Q(a, x) is 0 for every float32 shape

struct Work {
    int evaluations = 0, terms = 0, steps = 0;   // log_tail calls, series terms + fraction steps, inverse steps
    int most_series = 0, most_fraction = 0;      // the longest series / fraction of one log_tail call
};

GPP_GM_HD bool valid(float v) { return v == v && fabsf(v) < INFINITY; }   // util.cpp:16-18

// ---- AS 241, PPND16 -------------------------------------------------------------------------------------------------------------------
// p in (0, 1); 1 - p is exact wherever p comes from a float32 (the callers' case), so the upper tail loses nothing
GPP_GM_HD double ndtri(double p) {
    const double q = p - 0.5;
    if(fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r +
                               1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r + 1.3314166789178437745e+2) * r + 3.3871328727963666080e0);
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r +
                               5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r + 4.2313330701600911252e+1) * r + 1.0);
        return q * num / den;
    }
    double r = q < 0 ? p : 1 - p;
    if(!(r > 0)) return q < 0 ? -INFINITY : INFINITY;
    r = sqrt(-log(r));
    double v;
    if(r <= 5) {
        r -= 1.6;
        const double num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r + 1.27045825245236838258e0) * r +
                               3.64784832476320460504e0) * r + 5.76949722146069140550e0) * r + 4.63033784615654529590e0) * r + 1.42343711074968357734e0);
        const double den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r +
                               6.89767334985100004550e-1) * r + 1.67638483018380384940e0) * r + 2.05319162663775882187e0) * r + 1.0);
        v = num / den;
    }
    else {
        r -= 5;
        const double num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r +
                               2.96560571828504891230e-1) * r + 1.78482653991729133580e0) * r + 5.46378491116411436990e0) * r + 6.65790464350110377720e0);
        const double den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r +
                               1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r + 5.99832206555887937690e-1) * r + 1.0);
        v = num / den;
    }
    return q < 0 ? -v : v;
}

GPP_GM_HD double ncdf(double z) { return 0.5 * erfc(-z * 0.70710678118654752440); }

// ---- the incomplete gamma function -------------------------------------------------------------------------------------------------------
struct Tail {
    double lg;    // ln P(a, x) (upper = false) or ln Q(a, x) (upper = true)
    bool upper;
};
GPP_GM_HD double p_of(const Tail& t) { return t.upper ? -expm1(t.lg) : exp(t.lg); }
GPP_GM_HD double q_of(const Tail& t) { return t.upper ? exp(t.lg) : -expm1(t.lg); }
GPP_GM_HD double log_q_of(const Tail& t) { return t.upper ? t.lg : log(-expm1(t.lg)); }

// a > 0, x >= 0, lga = lgamma(a).  The prefactor x^a e^-x / Gamma(a) is formed as a logarithm: at a = 1e3 its three terms are near
// 7e3 each, so the tail carries up to 1e-12 relative error from there.
GPP_GM_HD Tail log_tail(double a, double x, double lga, Work* work = nullptr) {
    if(work) work->evaluations++;
    if(!(x > 0)) return {-INFINITY, false};
    if(!(x < HUGE_X)) return {-INFINITY, true};
    const double front = a * log(x) - x - lga;
    int n = 0;
    Tail out;
    if(x < a + 1) {   // P(a, x) = x^a e^-x / Gamma(a + 1) * (1 + x / (a + 1) + x^2 / ((a + 1)(a + 2)) + ...)
        double term = 1, sum = 1;
        for(n = 1; n <= SERIES_MAX_TERMS; n++) {
            term *= x / (a + n);
            sum += term;
            if(term < sum * TERM_EPS) break;
        }
        out = {front - log(a) + log(sum), false};
    }
    else {            // Q(a, x) = x^a e^-x / Gamma(a) * 1 / (x + 1 - a - 1 (1 - a) / (x + 3 - a - 2 (2 - a) / (x + 5 - a - ...)))
        double b = x + 1 - a, c = 1 / LENTZ_TINY, d = 1 / b, h = d;
        for(n = 1; n <= FRACTION_MAX_STEPS; n++) {
            const double an = -(double)n * ((double)n - a);
            b += 2;
            d = an * d + b;
            if(fabs(d) < LENTZ_TINY) d = LENTZ_TINY;
            c = b + an / c;
            if(fabs(c) < LENTZ_TINY) c = LENTZ_TINY;
            d = 1 / d;
            const double del = d * c;
            h *= del;
            if(fabs(del - 1) < TERM_EPS) break;
        }
        out = {front + log(h), true};
    }
    if(work) {
        work->terms += n;
        int& most = out.upper ? work->most_fraction : work->most_series;
        most = n > most ? n : most;
    }
    return out;
}

// x with P(a, x) = p for 0 <= p <= 1; lga = lgamma(a)
GPP_GM_HD double p_inverse(double a, double p, double lga, Work* work = nullptr) {
    if(!(p > 0)) return 0;
    if(!(p < 1)) return INFINITY;
    const double lnp = log(p);
    // P(a, x) <= x^a / Gamma(a + 1), with equality to a x / (a + 1) relative: ln of the x that solves the right-hand side
    const double us = (lnp + lga + log(a)) / a;
    if(us < LOG_SMALL_X) return exp(us);
    const double q = 1 - p;
    double x0;
    bool small = false;   // a <= 1 and p below t, which is P(a, 1) to 1e-3: x is below about 1, where P is a power law times a slow factor
    if(a > 1) {
        const double w = 1 - 1 / (9 * a) + ndtri(p) / (3 * sqrt(a));
        x0 = w > 0 ? a * w * w * w : 0;
    }
    else {
        const double t = 1 - a * (0.253 + a * 0.12);
        small = p < t;
        x0 = small ? exp((lnp - log(t)) / a) : 1 - log(q / (1 - t));
    }
    int n = 0;
    double x;
    // The median is below the mean a, so for p <= 0.5 us <= ln x < ln a; for `small`, x < a + 1 by a wide margin.  Either way the series
    // is the method all the way and P itself is computed: against a float32 p > 0.5 its 1e-16 of absolute error is at most 2e-9 of 1 - p.
    if(p <= 0.5 || small) {
        double lo = us, hi = p <= 0.5 ? log(a) : log(a + 1), u = log(x0);
        if(!(u > lo && u < hi)) u = !(u > lo) ? lo : hi;
        for(n = 1; n <= INVERSE_MAX_STEPS; n++) {
            const double xu = exp(u);
            const double lnP = log_tail(a, xu, lga, work).lg;
            const double g = lnP - lnp;
            if(g == 0) break;
            if(g < 0) lo = u;
            else hi = u;
            double un = u - g / exp(a * u - xu - lga - lnP);   // d ln P / d ln x = x pdf(x) / P
            if(un < lo && un >= lo - INVERSE_TOL) un = lo;   // (past an end by less than the tolerance: that end, e.g. the exact lower bound us)
            else if(un > hi && un <= hi + INVERSE_TOL) un = hi;
            if(!(un >= lo && un <= hi)) un = 0.5 * (lo + hi);
            const double step = fabs(un - u);
            u = un;
            if(step <= INVERSE_TOL) break;
        }
        x = exp(u);
    }
    else {
        const double lnq = log(q);
        double lo = exp(us), hi = INFINITY;
        x = x0 > lo ? x0 : lo;
        for(n = 1; n <= INVERSE_MAX_STEPS; n++) {
            const double lnQ = log_q_of(log_tail(a, x, lga, work));
            const double h = lnQ - lnq;
            if(h == 0) break;
            if(h > 0) lo = x;
            else hi = x;
            double xn = x + h / exp((a - 1) * log(x) - x - lga - lnQ);   // d ln Q / dx = -pdf(x) / Q
            if(xn < lo && xn >= lo - INVERSE_TOL * lo) xn = lo;
            else if(xn > hi && xn <= hi + INVERSE_TOL * hi) xn = hi;
            if(!(xn >= lo && xn <= hi)) xn = hi < INFINITY ? 0.5 * (lo + hi) : 2 * x + 1;
            const double step = fabs(xn - x);
            x = xn;
            if(step <= INVERSE_TOL * x) break;
        }
    }
    if(work) work->steps += n;
    return x;
}

// ---- distribution.cpp:5-33 -------------------------------------------------------------------------------------------------------------
enum { GAMMA_OK = 0, GAMMA_LEVEL = 1, GAMMA_SHAPE = 2, GAMMA_SCALE = 3 };
// *code receives which of the three exceptions the reference throws (:8-22, in that order); the value is NaN then.  level 1 gives +inf
// (the reference raises through Boost's overflow policy).
GPP_GM_HD float gamma_inv(float level, float shape, float scale, int* code, Work* work = nullptr) {
    *code = GAMMA_OK;
    if(level < 0 || level > 1 || !valid(level)) { *code = GAMMA_LEVEL; return NAN; }
    if(shape <= 0 || !valid(shape)) { *code = GAMMA_SHAPE; return NAN; }
    if(scale <= 0 || !valid(scale)) { *code = GAMMA_SCALE; return NAN; }
    return (float)((double)scale * p_inverse((double)shape, (double)level, lgamma((double)shape), work));
}

// ---- transform.cpp:155-179 --------------------------------------------------------------------------------------------------------------
// The parameters have been checked by the caller (:158-163); lga = lgamma((double)shape), computed once per call.
struct GammaParams {
    float shape, scale, tolerance;
    double lga;
};
// :166-172.  `float cdf` is a float32 store, and so is value + m_tolerance (two floats).  x < 0 -> NaN and cdf 0 / 1 -> -inf / +inf
// where the reference raises (Boost's domain / overflow policy).
GPP_GM_HD float transform_forward(float value, const GammaParams& g, Work* work = nullptr) {
    if(!valid(value)) return NAN;
    const float x = value + g.tolerance;
    if(x < 0) return NAN;
    const float cdf = (float)p_of(log_tail((double)g.shape, (double)x / (double)g.scale, g.lga, work));
    if(cdf == 0) return -INFINITY;
    if(cdf == 1) return INFINITY;
    return (float)ndtri((double)cdf);
}
// :173-179.  cdf 1 -> +inf where the reference raises; cdf 0 gives -tolerance.
GPP_GM_HD float transform_backward(float value, const GammaParams& g, Work* work = nullptr) {
    if(!valid(value)) return NAN;
    const float cdf = (float)ncdf((double)value);
    if(cdf == 1) return INFINITY;
    return (float)((double)g.scale * p_inverse((double)g.shape, (double)cdf, g.lga, work) - (double)g.tolerance);
}

}   // namespace gamma_fn
}   // namespace gpp
