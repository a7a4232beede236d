// gridpp::interpolate (src/api/util.cpp:339-414) and gridpp::apply_curve (src/api/curve.cpp:6-77) for ONE value, written once for
// the host and the device: the kernels of curve.hip and the host-only entry points (gpp_apply_curve_scalar,
// gpp_interpolate_scalar) compile this same text, so a CPU test of the scalar forms exercises the source the GPU runs.
// Plain float32 arithmetic in the reference's order; the library is built with -ffp-contract=off and correctly rounded division.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/gridpp_hip.h"

namespace gpp {
namespace curve {

#define GPP_HD __host__ __device__ inline

GPP_HD bool valid(float v) { return v == v && fabsf(v) < INFINITY; }   // util.cpp:16-18

// util.cpp:339-357: invalid entries are skipped; the first valid entry equal to x, else the last valid entry < x seen before the
// first valid entry > x.  -1 where the reference's index stays undefined (its (int) NaN).
GPP_HD int lower_index(float x, const float* v, int n) {
    int index = -1;
    for(int i = 0; i < n; i++) {
        const float c = v[i];
        if(valid(c)) {
            if(c < x) index = i;
            else if(c == x) { index = i; break; }
            else if(c > x) break;
        }
    }
    return index;
}
// util.cpp:358-376: the mirror image from the back
GPP_HD int upper_index(float x, const float* v, int n) {
    int index = -1;
    for(int i = n - 1; i >= 0; i--) {
        const float c = v[i];
        if(valid(c)) {
            if(c > x) index = i;
            else if(c == x) { index = i; break; }
            else if(c < x) break;
        }
    }
    return index;
}

// true where a bisection finds the indices of the two scans: every entry valid, the curve non-decreasing
inline bool valid_and_sorted(const float* v, int n) {
    for(int i = 0; i < n; i++)
        if(!valid(v[i]) || (i > 0 && v[i] < v[i - 1])) return false;
    return true;
}
// The two scan indices of a valid_and_sorted curve for v[0] <= x <= v[n-1], by bisection: lb = first entry >= x, ub = first entry
// > x.  Where an entry equals x the scans stop at the first (from the front) and the last (from the back) of them: lb and ub - 1;
// otherwise at the neighbours of the gap: lb - 1 and lb.
GPP_HD void sorted_indices(float x, const float* v, int n, int& i0, int& i1) {
    int lo = 0, hi = n;
    while(lo < hi) {
        const int mid = (lo + hi) >> 1;
        if(v[mid] < x) lo = mid + 1; else hi = mid;
    }
    const int lb = lo;
    hi = n;
    while(lo < hi) {
        const int mid = (lo + hi) >> 1;
        if(v[mid] <= x) lo = mid + 1; else hi = mid;
    }
    const int ub = lo;
    if(lb < ub) { i0 = lb; i1 = ub - 1; }
    else { i0 = lb - 1; i1 = lb < n ? lb : -1; }
}

// util.cpp:393-411 from the two indices and the four values they select; NaN where an index is undefined
GPP_HD float between(float x, int i0, int i1, int n, float x0, float x1, float y0, float y1) {
    if(i0 < 0 || i1 < 0) return NAN;
    if(x0 == x1) {
        if(i0 == 0 && i1 == n - 1) return (y0 + y1) / 2;
        if(i0 == 0) return y1;
        if(i1 == n - 1) return y0;
        return (y0 + y1) / 2;
    }
    return y0 + (y1 - y0) * (x - x0) / (x1 - x0);
}

// util.cpp:377-414 (sizes already checked).  sorted: iX is valid_and_sorted
GPP_HD float interpolate(float x, const float* iX, const float* iY, int n, bool sorted) {
    if(!valid(x)) return NAN;
    if(n == 0) return NAN;
    if(x > iX[n - 1]) return iY[n - 1];
    if(x < iX[0]) return iY[0];
    int i0, i1;
    if(sorted) sorted_indices(x, iX, n, i0, i1);
    else { i0 = lower_index(x, iX, n); i1 = upper_index(x, iX, n); }
    if(i0 < 0 || i1 < 0) return NAN;
    return between(x, i0, i1, n, iX[i0], iX[i1], iY[i0], iY[i1]);
}

GPP_HD bool known_policy(int p) {   // include/gridpp.h:79-85
    return p == GPP_ONE_TO_ONE || p == GPP_MEAN_SLOPE || p == GPP_NEAREST_SLOPE || p == GPP_ZERO || p == GPP_UNCHANGED;
}

// curve.cpp:26-74: the input lies outside [curve_fcst[0], curve_fcst[C-1]] (or does not compare: NaN).  *unknown (if given) is set
// where the reference throws "Unknown extrapolation policy"; the array forms have checked the policies before.
GPP_HD float extrapolate(float input, const float* curve_ref, const float* curve_fcst, int C, int policy_below, int policy_above,
                         bool* unknown) {
    const float smallestObs = curve_ref[0], smallestFcst = curve_fcst[0];
    const float largestObs = curve_ref[C - 1], largestFcst = curve_fcst[C - 1];
    const bool below = input <= smallestFcst;
    const float nearestObs = below ? smallestObs : largestObs;
    const float nearestFcst = below ? smallestFcst : largestFcst;
    const int policy = below ? policy_below : policy_above;
    if(policy == GPP_UNCHANGED) return input;
    float slope = 1;
    if(policy == GPP_ZERO) slope = 0;
    else if(policy == GPP_ONE_TO_ONE || C <= 1) slope = 1;
    else if(policy == GPP_MEAN_SLOPE) {
        const float dObs = largestObs - smallestObs;
        const float dFcst = largestFcst - smallestFcst;
        slope = dObs / dFcst;
    }
    else if(policy == GPP_NEAREST_SLOPE) {
        float dObs, dFcst;
        if(below) { dObs = curve_ref[1] - curve_ref[0]; dFcst = curve_fcst[1] - curve_fcst[0]; }
        else { dObs = curve_ref[C - 1] - curve_ref[C - 2]; dFcst = curve_fcst[C - 1] - curve_fcst[C - 2]; }
        slope = dObs / dFcst;
    }
    else {
        if(unknown) *unknown = true;
        return NAN;
    }
    return nearestObs + slope * (input - nearestFcst);
}

// curve.cpp:6-77 (sizes already checked, C >= 1).  sorted: curve_fcst is valid_and_sorted
GPP_HD float apply(float input, const float* curve_ref, const float* curve_fcst, int C, int policy_below, int policy_above, bool sorted,
                   bool* unknown) {
    if(input >= curve_fcst[0] && input <= curve_fcst[C - 1]) return interpolate(input, curve_fcst, curve_ref, C, sorted);
    return extrapolate(input, curve_ref, curve_fcst, C, policy_below, policy_above, unknown);
}

}   // namespace curve
}   // namespace gpp
