// The weather diagnostics (src/api/humidity.cpp, pressure.cpp, qnh.cpp, wind.cpp) and the value transforms (src/api/transform.cpp) for
// ONE value, written once for the host and the device: the kernels of pointwise.hip and the host-only scalar entry points
// (gpp_diagnostic_scalar, gpp_transform_scalar) compile this same text, so a CPU test of the scalar forms exercises the source the GPU
// runs.
//
// Promotions.  Every function follows the reference line by line.  An intermediate the reference stores in a `float` is rounded to
// float32 at that store; an expression that a `double` literal promotes (273.15, 17.63, 0.611, 0.2, 0.00066, -1.0 / mThreshold, 10.,
// 0.5 * a * altitude, ...) is evaluated in double up to the next store; `float g0 = 9.80665` is a float32 constant and gridpp::pi is
// 3.14159265f.  The library is built with -ffp-contract=off and correctly rounded division and square root, so the plain operations
// are the same IEEE operations on both sides.
//
// Transcendentals.  Whether the reference's unqualified exp / log / pow bind to the float or to the double overload depends on which
// headers reach each file (gridpp.h pulls <cmath> in only through Boost), which its text does not settle.  The choice made here, once
// for all of them: the function is evaluated in DOUBLE from its already-rounded arguments, its value stays a double inside the
// expression it stands in, and the expression is rounded to float32 where the reference stores a float.  Such a value is within half
// a float32 ulp (plus the double evaluation's own error) of the exactly rounded one: at least as close to either reading as two
// conforming libms are to each other.  The one qualified call, std::atan2 on two floats (wind.cpp:21), IS the float overload: its
// double value is rounded to float32 before the multiplication.  sqrt of a float32 sum through double and back is the float32 square
// root (wind.cpp:7).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/gridpp_hip.h"

namespace gpp {
namespace pointwise {

#define GPP_PW_HD __host__ __device__ inline

GPP_PW_HD bool valid(float v) { return v == v && fabsf(v) < INFINITY; }   // util.cpp:16-18

// ---- humidity.cpp ---------------------------------------------------------------------------------------------------------------
// humidity.cpp:5-21.  td <= temperature ? td : temperature: a NaN td (rh = 0 gives log 0, rh < 0 log of a negative) fails the
// comparison and returns the temperature -- not fmin.
GPP_PW_HD float dewpoint(float temperature, float relative_humidity) {
    if(!(valid(temperature) && valid(relative_humidity))) return NAN;
    const float tempC = (float)((double)temperature - 273.15);                                                              // :8
    const float e = (float)((double)relative_humidity * 0.611 * exp((17.63 * (double)tempC) / ((double)tempC + 243.04)));   // :9
    const double le = log((double)e);
    const float tdC = (float)((116.9 + 243.04 * le) / (16.78 - le));                                                        // :10
    const float td = (float)((double)tdC + 273.15);                                                                         // :11
    return td <= temperature ? td : temperature;                                                                            // :12
}

// humidity.cpp:49-57 / :59-67: the saturation pressure table at x, x already clamped to [0, 39]; x = 39 reads entries 39 and 40
GPP_PW_HD float ewt_at(float x) {
    static constexpr float mEwt[41] = {(float).000034, (float).000089, (float).000220, (float).000517, (float).001155, (float).002472,
                                       (float).005080, (float).01005,  (float).01921,  (float).03553,  (float).06356,  (float).1111,
                                       (float).1891,   (float).3139,   (float).5088,   (float).8070,   (float)1.2540,  (float)1.9118,
                                       (float)2.8627,  (float)4.2148,  (float)6.1078,  (float)8.7192,  (float)12.272,  (float)17.044,
                                       (float)23.373,  (float)31.671,  (float)42.430,  (float)56.236,  (float)73.777,  (float)95.855,
                                       (float)123.40,  (float)157.46,  (float)199.26,  (float)250.16,  (float)311.69,  (float)385.56,
                                       (float)473.67,  (float)578.09,  (float)701.13,  (float)845.28,  (float)1013.25};   // :34-40
    const int l = (int)x;
    return mEwt[l] + (mEwt[l + 1] - mEwt[l]) * (x - (float)l);
}
GPP_PW_HD float ewt_index(float kelvin) {   // :49-53
    float x = (float)(((double)kelvin - 173.16) * 0.2);
    if(x < 0) x = 0;
    else if(x > 39) x = 39;
    return x;
}
// humidity.cpp:33-79
GPP_PW_HD float relative_humidity(float temperature, float dewpoint) {
    if(!(valid(temperature) && valid(dewpoint))) return NAN;
    if(temperature <= dewpoint) return 1;                  // :43-44, before anything else
    const float et = ewt_at(ewt_index(temperature));       // :49-57
    const float etd = ewt_at(ewt_index(dewpoint));         // :59-67
    float rh = etd / et;
    if(rh < 0) rh = 0;
    if(rh > 1) rh = 1;
    return rh;
}

// humidity.cpp:91-109.  The two tests of :93 come before the validity test: a NaN fails both and falls through to it.
GPP_PW_HD float wetbulb(float temperature, float pressure, float relative_humidity) {
    const float temperatureC = (float)((double)temperature - 273.15);                                                             // :92
    if((double)temperatureC <= -243.04 || relative_humidity <= 0) return NAN;                                                     // :93
    if(!(valid(temperatureC) && valid(pressure) && valid(relative_humidity))) return NAN;
    const float e = (float)((double)relative_humidity * 0.611 * exp((17.63 * (double)temperatureC) / ((double)temperatureC + 243.04)));   // :96
    const double le = log((double)e);
    const float Td = (float)((116.9 + 243.04 * le) / (16.78 - le));                                                               // :97
    const float gamma = (float)(0.00066 * (double)pressure / 1000);                                                               // :98
    const float delta = (float)((double)(4098 * e) / pow((double)Td + 243.04, 2.0));                                              // :99 (4098 * e is a float product)
    if(gamma + delta == 0) return NAN;                                                                                            // :100
    const float wetbulbTemperature = (gamma * temperatureC + delta * Td) / (gamma + delta);                                       // :102
    return (float)((double)wetbulbTemperature + 273.15);                                                                          // :103
}

// ---- pressure.cpp ---------------------------------------------------------------------------------------------------------------
// pressure.cpp:5-13.  No guard on a zero temperature: IEEE arithmetic gives the reference's answers.
GPP_PW_HD float pressure(float ielev, float oelev, float ipressure, float itemperature) {
    const float g0 = 9.80665f, M = 0.0289644f, R = 8.3144598f;
    if(!(valid(ielev) && valid(oelev) && valid(ipressure) && valid(itemperature))) return NAN;
    const float arg = -g0 * M * (oelev - ielev) / (R * itemperature);
    return (float)((double)ipressure * exp((double)arg));                                                                         // :11
}

enum { SLP_OK = 0, SLP_ALTITUDE = 1, SLP_TEMPERATURE = 2, SLP_UNPHYSICAL = 3 };
// pressure.cpp:28-80.  *code receives which of the three exceptions the reference throws (:32-38, in that order, on the inputs as
// given; NaNs pass the third test); the value is NaN then.
GPP_PW_HD float sea_level_pressure(float ps, float altitude, float temperature, float rh, float dewpoint, int* code) {
    *code = SLP_OK;
    if(!valid(altitude)) { *code = SLP_ALTITUDE; return NAN; }
    if(!valid(temperature)) { *code = SLP_TEMPERATURE; return NAN; }
    if(ps < 0 || temperature < 0 || rh < 0 || rh > 1 || dewpoint < 0) { *code = SLP_UNPHYSICAL; return NAN; }
    const float T = (float)((double)temperature - 273.15);                                                                        // :42
    const float Ts = (float)(273.15 + (double)T);                                                                                 // :43
    const float g = 9.80665f, R = 287.05f, a = 0.0065f, Ch = 0.12f;   // gridpp::gravit, gridpp::gas_constant_si, :48-49
    float e = 0, slp = 0;
    ps = (float)((double)ps * 0.01);                                                                                              // :50
    if(valid(rh)) {
        const float es = (float)(6.11 * pow(10., (7.5 * (double)T) / (237.3 + (double)T)));                                       // :53
        e = rh * es;
        const float A = 17.625f, B = 243.04f, C = 6.1094f;
        const double l = log((double)(e / C));
        dewpoint = (float)(((double)B * l) / ((double)A - l));                                                                    // :59
    }
    else if(valid(dewpoint)) {
        dewpoint = (float)((double)dewpoint - 273.15);                                                                            // :61
        e = (float)(6.11 * pow(10., (7.5 * (double)dewpoint) / (237.3 + (double)dewpoint)));                                      // :62
    }
    else dewpoint = (float)((double)T - 3.);                                                                                      // :66
    if(altitude >= 50) {
        const float num = g * altitude / R;
        slp = (float)((double)ps * exp((double)num / ((double)Ts + 0.5 * (double)a * (double)altitude + (double)(e * Ch))));      // :70
    }
    else if(altitude < 50) {
        const float Tv = (float)((273.15 + (double)T) /
                                 (1 - 0.379 * (6.11 * pow(10., (7.5 * (double)dewpoint) / (237.7 + (double)dewpoint)) / (double)ps)));   // :72
        const float Ck = (float)((double)(ps * altitude) / (29.27 * (double)Tv));                                                 // :73
        slp = ps + Ck;
    }
    return (float)((double)slp * 100.);                                                                                           // :77
}

// ---- qnh.cpp ---------------------------------------------------------------------------------------------------------------------
// qnh.cpp:6-30.  pressure == 0 gives 0 before the validity test, whatever the altitude; a negative pressure gives NaN through pow.
GPP_PW_HD float qnh(float pressure, float altitude) {
    if(pressure == 0) return 0;
    if(!(valid(altitude) && valid(pressure))) return NAN;
    const float g = 9.80665f, T0 = 288.15f, L = 0.0065f, CRGas = 287.053f, p0 = 101325;
    const double inner = pow((double)(pressure / p0), (double)((CRGas * L) / g));
    return (float)((double)p0 * pow(inner + (double)((altitude * L) / T0), (double)(g / (CRGas * L))));                           // :24
}

// ---- wind.cpp --------------------------------------------------------------------------------------------------------------------
GPP_PW_HD float wind_speed(float xwind, float ywind) { return sqrtf(xwind * xwind + ywind * ywind); }   // wind.cpp:6-8, no validity test
// wind.cpp:20-26.  (0, 0): atan2(-0, -0) = -pi -> -180 -> 180; a -0.0 is not < 0 and stays.
GPP_PW_HD float wind_direction(float xwind, float ywind) {
    const float pi = 3.14159265f;
    float dir = (float)atan2((double)-xwind, (double)-ywind) * 180 / pi;
    if(dir < 0) dir += 360;
    return dir;
}

// ---- transform.cpp ---------------------------------------------------------------------------------------------------------------
// kind: GPP_TRANSFORM_*; p0 = mThreshold, p1 = mScaling.  The parameters of StartedBoxCox have been checked by the caller
// (transform.cpp:128-131).
GPP_PW_HD float transform_forward(float value, int kind, float p0, float p1) {
    switch(kind) {
        case GPP_TRANSFORM_IDENTITY: return value;                                                           // :180-182
        case GPP_TRANSFORM_LOG: return valid(value) ? (float)log((double)value) : NAN;                       // :85-90: forward(0) = -inf
        case GPP_TRANSFORM_BOXCOX:                                                                           // :100-109
            if(!valid(value)) return NAN;
            if(value <= 0) value = 0;
            if(p0 == 0) return (float)log((double)value);
            return (float)((pow((double)value, (double)p0) - 1) / (double)p0);
        case GPP_TRANSFORM_STARTED_BOXCOX:                                                                   // :133-142
            if(!valid(value) || p0 <= 0) return NAN;
            if(value < 0) value = 0;
            if(value <= p1) return value;
            return (float)((double)p1 * (1 + ((pow((double)(value / p1), (double)p0) - 1) / (double)p0)));
    }
    return NAN;
}
GPP_PW_HD float transform_backward(float value, int kind, float p0, float p1) {
    float rValue = 0;
    switch(kind) {
        case GPP_TRANSFORM_IDENTITY: return value;                                                           // :183-185
        case GPP_TRANSFORM_LOG: return valid(value) ? (float)exp((double)value) : NAN;                       // :91-96
        case GPP_TRANSFORM_BOXCOX:                                                                           // :110-125
            if(!valid(value)) return NAN;
            if(p0 == 0) rValue = (float)exp((double)value);
            else {
                if((double)value < -1.0 / (double)p0) value = (float)(-1.0 / (double)p0);
                rValue = (float)pow((double)(1 + p0 * value), (double)(1 / p0));
            }
            if(rValue <= 0) rValue = 0;
            return rValue;
        case GPP_TRANSFORM_STARTED_BOXCOX:                                                                   // :143-154
            if(!valid(value) || p0 <= 0) return NAN;
            if(value <= p1) rValue = value;
            else rValue = (float)((double)p1 * pow((double)(1 + p0 / p1 * (value - p1)), (double)(1 / p0)));
            if(rValue < 0) rValue = 0;
            return rValue;
    }
    return NAN;
}

}   // namespace pointwise
}   // namespace gpp
