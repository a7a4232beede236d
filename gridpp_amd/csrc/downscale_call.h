// What the levels-style downscaling entries (bilinear, simple_gradient / full_gradient, the applies of a plan) share once their own
// checks have passed: the output, the all-NaN result of an empty input grid (nearest.cpp:132-134, bilinear.cpp:37-39: all missing,
// and so is every sum with them), the `err` words of the kernel and, after it, the error of a distorted box.
#pragma once
#include "common.h"

// bilinear.hip: the reference's std::runtime_error "Problem with bilinear interpolation..." when a kernel flagged a box
// whose weights leave [0, 1]: err[0] = 1, err[1..2] = bits of the offending (s, t) (bilinear.cpp:309-313)
void bilinear_check_distorted(const int herr[4]);

namespace gpp {

struct DownscaleCall {
    OutField o;
    DevBuf<int> own_err;
    int* err = nullptr;   // zeroed, for the kernel
    bool done = false;    // an empty input grid: the result is complete
    // n_in: cells of the input grid; values: the first input field; plan_err: the buffer of a plan, NULL = one of this call
    DownscaleCall(size_t n_in, const float* values, float* out, size_t nout, int mem, DevBuf<int>* plan_err = nullptr) {
        if(!out) invalid("out is NULL");
        o.bind(out, nout, mem);
        if(n_in == 0) {
            fill_f32(o.d, nout, NAN);
            finish_call(o);
            done = true;
            return;
        }
        if(!values) invalid("values is NULL");
        err = (plan_err ? *plan_err : own_err).get(4);
        GPP_HIP(hipMemsetAsync(err, 0, 4 * sizeof(int), stream()));
    }
    void finish() {   // after the launch
        int herr[4];
        GPP_HIP(hipMemcpyAsync(herr, err, sizeof(herr), hipMemcpyDeviceToHost, stream()));
        finish_call(o);
        bilinear_check_distorted(herr);
    }
};

}   // namespace gpp
