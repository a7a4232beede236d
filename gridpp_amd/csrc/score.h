// gridpp::calc_score(a, b, c, d, metric) (src/api/metric_optimizer.cpp:207-244) as ONE function for the host scalar
// (gpp_calc_score_table), the vector form (after its count reduction) and the finish step of both neighbourhood_score paths, so that the
// three cannot drift apart.  The reference's promotions are kept operation for operation: every `/ 1.0`, `* 1.0` and `2.0 *` lifts that
// operation (and what follows it in the expression) to double, sums such as a + b + c stay float, the result is rounded to float once.
// No contraction: a * d - b * c is two products and a difference (the library is built with -ffp-contract=off; the pragma below says
// it again for whoever includes this elsewhere).
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPP_SCORE_HD __host__ __device__
#else
#define GPP_SCORE_HD
#endif

#define GPP_SCORE_ETS 0    /* GPP_METRIC_* of include/gridpp_hip.h (include/gridpp.h:103-110) */
#define GPP_SCORE_TS 1
#define GPP_SCORE_KSS 20
#define GPP_SCORE_PC 30
#define GPP_SCORE_BIAS 40
#define GPP_SCORE_HSS 50

GPP_SCORE_HD inline bool gpp_score_metric_known(int metric) {
    return metric == GPP_SCORE_ETS || metric == GPP_SCORE_TS || metric == GPP_SCORE_KSS || metric == GPP_SCORE_PC || metric == GPP_SCORE_BIAS ||
           metric == GPP_SCORE_HSS;
}

// an unknown metric gives NaN here: the callers refuse it before they get this far
GPP_SCORE_HD inline float gpp_score_value(float a, float b, float c, float d, int metric) {
#pragma clang fp contract(off)
    const float missing = NAN;
    if(metric == GPP_SCORE_ETS) {                                   // :208-214
        const float N = a + b + c + d;
        const float ar = (float)((double)(a + b) / 1.0 / (double)N * (double)(a + c));
        if(a + b + c - ar == 0) return missing;
        return (float)((double)(a - ar) / 1.0 / (double)(a + b + c - ar));
    }
    if(metric == GPP_SCORE_TS) return (float)((double)a / 1.0 / (double)(a + b + c));   // :215-218, no guard: 0 / 0 is NaN
    if(metric == GPP_SCORE_PC) {                                    // :219-222, float, no guard
        const float N = a + b + c + d;
        return (a + d) / N;
    }
    if(metric == GPP_SCORE_KSS) {                                   // :223-227
        if((a + c) * (b + d) == 0) return missing;
        return (float)((double)(a * d - b * c) * 1.0 / (double)((a + c) * (b + d)));
    }
    if(metric == GPP_SCORE_BIAS) {                                  // :228-234
        if(b == c) return 1.0f;
        return 1.0f - fabsf(b - c) / (b + c);
    }
    if(metric == GPP_SCORE_HSS) {                                   // :235-240
        const float denom = (a + c) * (c + d) + (a + b) * (b + d);
        if(denom == 0) return missing;
        return (float)(2.0 * (double)(a * d - b * c) / (double)denom);
    }
    return missing;
}
