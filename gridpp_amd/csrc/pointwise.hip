// The weather diagnostics (src/api/humidity.cpp, pressure.cpp, qnh.cpp, wind.cpp) and the value transforms (src/api/transform.cpp)
// for gfx950: element-wise over n values.  The per-value arithmetic is pointwise.h, shared by the kernel and the host-only scalar entry
// points (gpp_diagnostic_scalar, gpp_transform_scalar).
//
//   k_pointwise<Op, NIN, VEC, IN64>   NIN input arrays of n values, one output.  VEC = 4: a lane loads four consecutive values of every
//                                     input and stores four, as single 16-byte accesses -- taken when every pointer of the call is
//                                     16-byte aligned, with a VEC = 1 launch for the n mod 4 tail; any unaligned pointer sends the
//                                     whole call to VEC = 1 (the pattern of k_curve_shared).  GPP_POINTWISE_BLOCK lanes per workgroup,
//                                     at most GPP_POINTWISE_MAX_BLOCKS workgroups (8 per compute unit), a grid stride beyond that.
//                                     IN64: the staged inputs of a GPP_HOST_F64 call are doubles and are rounded to float32 as the
//                                     first operation (the typemap's rounding, swig/vector.i:42-55).  No LDS.  The parameters of an
//                                     operation (threshold, scaling) travel by value inside Op.
//   Errors of sea_level_pressure      the kernel never traps: for an offending element it does a global atomicMin of
//                                     (index << 2) | code on one 64-bit status word (all ones before the launch) and writes NaN; the
//                                     host reads the word after the stream has run and reports the lowest offending index.
#include "common.h"
#include "pointwise.h"
#include <cstdint>

using namespace gpp;

namespace {

namespace pw = gpp::pointwise;

// ---- the operations: NIN, whether they report through the status word, and the per-value call ------------------------------------
struct OpDewpoint {
    static constexpr int NIN = 2; static constexpr bool REPORTS = false;
    GPP_PW_HD float operator()(const float* v, int*) const { return pw::dewpoint(v[0], v[1]); }
};
struct OpRelativeHumidity {
    static constexpr int NIN = 2; static constexpr bool REPORTS = false;
    GPP_PW_HD float operator()(const float* v, int*) const { return pw::relative_humidity(v[0], v[1]); }
};
struct OpWetbulb {
    static constexpr int NIN = 3; static constexpr bool REPORTS = false;
    GPP_PW_HD float operator()(const float* v, int*) const { return pw::wetbulb(v[0], v[1], v[2]); }
};
struct OpPressure {
    static constexpr int NIN = 4; static constexpr bool REPORTS = false;
    GPP_PW_HD float operator()(const float* v, int*) const { return pw::pressure(v[0], v[1], v[2], v[3]); }
};
struct OpSeaLevelPressure {
    static constexpr int NIN = 5; static constexpr bool REPORTS = true;
    GPP_PW_HD float operator()(const float* v, int* code) const { return pw::sea_level_pressure(v[0], v[1], v[2], v[3], v[4], code); }
};
struct OpQnh {
    static constexpr int NIN = 2; static constexpr bool REPORTS = false;
    GPP_PW_HD float operator()(const float* v, int*) const { return pw::qnh(v[0], v[1]); }
};
struct OpWindSpeed {
    static constexpr int NIN = 2; static constexpr bool REPORTS = false;
    GPP_PW_HD float operator()(const float* v, int*) const { return pw::wind_speed(v[0], v[1]); }
};
struct OpWindDirection {
    static constexpr int NIN = 2; static constexpr bool REPORTS = false;
    GPP_PW_HD float operator()(const float* v, int*) const { return pw::wind_direction(v[0], v[1]); }
};
template <int KIND, bool BACKWARD>
struct OpTransform {
    static constexpr int NIN = 1; static constexpr bool REPORTS = false;
    float p0, p1;
    GPP_PW_HD float operator()(const float* v, int*) const {
        return BACKWARD ? pw::transform_backward(v[0], KIND, p0, p1) : pw::transform_forward(v[0], KIND, p0, p1);
    }
};

template <int NIN>
struct Inputs {
    const void* p[NIN];
};

// nvec steps of VEC values each; `first` is the index of in[.][0] within the call's arrays (the tail launch starts behind the wide one)
template <class Op, int NIN, int VEC, bool IN64>
__global__ __launch_bounds__(GPP_POINTWISE_BLOCK) void k_pointwise(Op op, Inputs<NIN> in, long long nvec, long long first, float* __restrict__ out,
                                                                   unsigned long long* __restrict__ status) {
    static_assert(VEC == 1 || VEC == 4, "one value or one 16-byte access per lane and step");
    const long long stride = (long long)gridDim.x * GPP_POINTWISE_BLOCK;
    for(long long i = (long long)blockIdx.x * GPP_POINTWISE_BLOCK + threadIdx.x; i < nvec; i += stride) {
        float v[VEC][NIN], o[VEC];
#pragma unroll
        for(int a = 0; a < NIN; a++) {
            if(IN64) {   // float64 staged by the host: the cast is the typemap's rounding
                const double* src = static_cast<const double*>(in.p[a]);
                if(VEC == 4) {
                    const double2 q0 = reinterpret_cast<const double2*>(src)[2 * i], q1 = reinterpret_cast<const double2*>(src)[2 * i + 1];
                    v[0][a] = (float)q0.x; v[1 % VEC][a] = (float)q0.y; v[2 % VEC][a] = (float)q1.x; v[3 % VEC][a] = (float)q1.y;
                }
                else v[0][a] = (float)src[i];
            }
            else {
                const float* src = static_cast<const float*>(in.p[a]);
                if(VEC == 4) {
                    const float4 q = reinterpret_cast<const float4*>(src)[i];
                    v[0][a] = q.x; v[1 % VEC][a] = q.y; v[2 % VEC][a] = q.z; v[3 % VEC][a] = q.w;
                }
                else v[0][a] = src[i];
            }
        }
#pragma unroll
        for(int k = 0; k < VEC; k++) {
            int code = 0;
            o[k] = op(v[k], &code);
            if(Op::REPORTS && code != 0) {
                atomicMin(status, ((unsigned long long)(first + i * VEC + k) << 2) | (unsigned long long)code);
                o[k] = NAN;
            }
        }
        if(VEC == 4) reinterpret_cast<float4*>(out)[i] = make_float4(o[0], o[1 % VEC], o[2 % VEC], o[3 % VEC]);
        else out[i] = o[0];
    }
}

struct PointwiseWorkspace {
    DevBuf<unsigned long long> status;   // the one status word of a reporting call
};
thread_local PointwiseWorkspace g_pw;

template <class Op, int VEC, bool IN64>
void launch_vec(const Op& op, const Inputs<Op::NIN>& in, long long nvec, long long first, float* out, unsigned long long* status) {
    if(nvec <= 0) return;
    launch(k_pointwise<Op, Op::NIN, VEC, IN64>, grid_capped(blocks_of(nvec, GPP_POINTWISE_BLOCK), GPP_POINTWISE_MAX_BLOCKS), GPP_POINTWISE_BLOCK, 0, op, in, nvec, first, out, status);
}

// the wide launch over the first 4 * (n / 4) values where every pointer is 16-byte aligned, one value per lane for the rest
template <class Op, bool IN64>
void launch_both(const Op& op, const Inputs<Op::NIN>& in, long long n, float* out, unsigned long long* status) {
    uintptr_t bits = (uintptr_t)out;
    for(int a = 0; a < Op::NIN; a++) bits |= (uintptr_t)in.p[a];
    const long long n4 = (bits & 15) == 0 ? n / 4 : 0;
    launch_vec<Op, 4, IN64>(op, in, n4, 0, out, status);
    Inputs<Op::NIN> tail;
    for(int a = 0; a < Op::NIN; a++)
        tail.p[a] = IN64 ? (const void*)(static_cast<const double*>(in.p[a]) + 4 * n4) : (const void*)(static_cast<const float*>(in.p[a]) + 4 * n4);
    launch_vec<Op, 1, IN64>(op, tail, n - 4 * n4, 4 * n4, out + 4 * n4, status);
}

const char* slp_message(int code) {   // pressure.cpp:32-38
    switch(code) {
        case pw::SLP_ALTITUDE: return "sea_level_pressure: altitude is NAN";
        case pw::SLP_TEMPERATURE: return "sea_level_pressure: temperature is NAN";
        default: return "sea_level_pressure: unphysical values in input";
    }
}

// the NIN arrays of a call (`mem`) through Op
template <class Op>
void run(const Op& op, const float* const* arrays, long long n, float* out, int mem) {
    constexpr int NIN = Op::NIN;
    if(n < 0) invalid("negative number of values");
    if(n == 0) return;
    for(int a = 0; a < NIN; a++)
        if(!arrays[a]) invalid("an input array is NULL");
    if(!out) invalid("out is NULL");
    ensure_device();
    const bool f64 = !(mem & GPP_MEM_DEVICE) && (mem & GPP_HOST_F64);
    Staged<float> narrow[NIN];
    Staged<double> wide[NIN];
    Inputs<NIN> in;
    for(int a = 0; a < NIN; a++) {
        if(mem & GPP_MEM_DEVICE) in.p[a] = arrays[a];
        else if(f64) { wide[a].upload(reinterpret_cast<const double*>(arrays[a]), (size_t)n); in.p[a] = wide[a].p; }
        else { narrow[a].upload(arrays[a], (size_t)n); in.p[a] = narrow[a].p; }
    }
    OutField o;
    o.bind(out, (size_t)n, mem);
    unsigned long long* status = nullptr;
    if(Op::REPORTS) {
        status = g_pw.status.get(1);
        GPP_HIP(hipMemsetAsync(status, 0xFF, sizeof(unsigned long long), stream()));
    }
    if(f64) launch_both<Op, true>(op, in, n, o.d, status);
    else launch_both<Op, false>(op, in, n, o.d, status);
    o.finish();
    unsigned long long word = ~0ull;
    if(Op::REPORTS) GPP_HIP(hipMemcpyAsync(&word, status, sizeof(word), hipMemcpyDeviceToHost, stream()));
    GPP_HIP(hipStreamSynchronize(stream()));
    if(word != ~0ull) runtime(slp_message((int)(word & 3)));
}

void check_started_boxcox(float threshold, float scaling_factor) {   // transform.cpp:128-131
    if(!pw::valid(threshold) || threshold <= 0) invalid("threshold parameter must be > 0 in the started Box-Cox distribution");
    if(!pw::valid(scaling_factor) || scaling_factor <= 0) invalid("Scaling factor parameter must be > 0 in the started Box-Cox distribution");
}
void check_transform(int kind, float p0, float p1) {
    if(kind != GPP_TRANSFORM_IDENTITY && kind != GPP_TRANSFORM_LOG && kind != GPP_TRANSFORM_BOXCOX && kind != GPP_TRANSFORM_STARTED_BOXCOX)
        invalid("Unknown transform");
    if(kind == GPP_TRANSFORM_STARTED_BOXCOX) check_started_boxcox(p0, p1);
}

template <int KIND>
void run_transform(const float* in, long long n, int backward, float p0, float p1, float* out, int mem) {
    const float* arrays[1] = {in};
    if(backward) run(OpTransform<KIND, true>{p0, p1}, arrays, n, out, mem);
    else run(OpTransform<KIND, false>{p0, p1}, arrays, n, out, mem);
}

}   // namespace

extern "C" int gpp_dewpoint(const float* temperature, const float* relative_humidity, long long n, float* out, int mem) {
    GPP_TRY
    const float* arrays[] = {temperature, relative_humidity};
    run(OpDewpoint(), arrays, n, out, mem);
    return GPP_OK;
    GPP_CATCH
}
extern "C" int gpp_relative_humidity(const float* temperature, const float* dewpoint, long long n, float* out, int mem) {
    GPP_TRY
    const float* arrays[] = {temperature, dewpoint};
    run(OpRelativeHumidity(), arrays, n, out, mem);
    return GPP_OK;
    GPP_CATCH
}
extern "C" int gpp_wetbulb(const float* temperature, const float* pressure, const float* relative_humidity, long long n, float* out, int mem) {
    GPP_TRY
    const float* arrays[] = {temperature, pressure, relative_humidity};
    run(OpWetbulb(), arrays, n, out, mem);
    return GPP_OK;
    GPP_CATCH
}
extern "C" int gpp_pressure(const float* ielev, const float* oelev, const float* ipressure, const float* itemperature, long long n, float* out, int mem) {
    GPP_TRY
    const float* arrays[] = {ielev, oelev, ipressure, itemperature};
    run(OpPressure(), arrays, n, out, mem);
    return GPP_OK;
    GPP_CATCH
}
extern "C" int gpp_sea_level_pressure(const float* ps, const float* altitude, const float* temperature, const float* rh, const float* dewpoint,
                                      long long n, float* out, int mem) {
    GPP_TRY
    const float* arrays[] = {ps, altitude, temperature, rh, dewpoint};
    run(OpSeaLevelPressure(), arrays, n, out, mem);
    return GPP_OK;
    GPP_CATCH
}
extern "C" int gpp_qnh(const float* pressure, const float* altitude, long long n, float* out, int mem) {
    GPP_TRY
    const float* arrays[] = {pressure, altitude};
    run(OpQnh(), arrays, n, out, mem);
    return GPP_OK;
    GPP_CATCH
}
extern "C" int gpp_wind_speed(const float* xwind, const float* ywind, long long n, float* out, int mem) {
    GPP_TRY
    const float* arrays[] = {xwind, ywind};
    run(OpWindSpeed(), arrays, n, out, mem);
    return GPP_OK;
    GPP_CATCH
}
extern "C" int gpp_wind_direction(const float* xwind, const float* ywind, long long n, float* out, int mem) {
    GPP_TRY
    const float* arrays[] = {xwind, ywind};
    run(OpWindDirection(), arrays, n, out, mem);
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_transform(const float* in, long long n, int kind, int backward, float p0, float p1, float* out, int mem) {
    GPP_TRY
    check_transform(kind, p0, p1);
    switch(kind) {
        case GPP_TRANSFORM_IDENTITY: run_transform<GPP_TRANSFORM_IDENTITY>(in, n, backward, p0, p1, out, mem); break;
        case GPP_TRANSFORM_LOG: run_transform<GPP_TRANSFORM_LOG>(in, n, backward, p0, p1, out, mem); break;
        case GPP_TRANSFORM_BOXCOX: run_transform<GPP_TRANSFORM_BOXCOX>(in, n, backward, p0, p1, out, mem); break;
        default: run_transform<GPP_TRANSFORM_STARTED_BOXCOX>(in, n, backward, p0, p1, out, mem); break;
    }
    return GPP_OK;
    GPP_CATCH
}

// ---- host-only forms ----------------------------------------------------------------------------------------------------------
extern "C" int gpp_diagnostic_scalar(int which, const float* args, int nargs, float* out) {
    GPP_TRY
    static const int nin[] = {OpDewpoint::NIN, OpRelativeHumidity::NIN, OpWetbulb::NIN, OpPressure::NIN, OpSeaLevelPressure::NIN, OpQnh::NIN,
                              OpWindSpeed::NIN, OpWindDirection::NIN};
    if(which < 0 || which > GPP_DIAG_WIND_DIRECTION) invalid("Unknown diagnostic");
    if(nargs != nin[which]) invalid("wrong number of arguments for the diagnostic");
    if(!args || !out) invalid("args / out is NULL");
    int code = 0;
    float y = NAN;
    switch(which) {
        case GPP_DIAG_DEWPOINT: y = OpDewpoint()(args, &code); break;
        case GPP_DIAG_RELATIVE_HUMIDITY: y = OpRelativeHumidity()(args, &code); break;
        case GPP_DIAG_WETBULB: y = OpWetbulb()(args, &code); break;
        case GPP_DIAG_PRESSURE: y = OpPressure()(args, &code); break;
        case GPP_DIAG_SEA_LEVEL_PRESSURE: y = OpSeaLevelPressure()(args, &code); break;
        case GPP_DIAG_QNH: y = OpQnh()(args, &code); break;
        case GPP_DIAG_WIND_SPEED: y = OpWindSpeed()(args, &code); break;
        default: y = OpWindDirection()(args, &code); break;
    }
    if(code != 0) runtime(slp_message(code));
    *out = y;
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_transform_scalar(float value, int kind, int backward, float p0, float p1, float* out) {
    GPP_TRY
    check_transform(kind, p0, p1);
    if(!out) invalid("out is NULL");
    *out = backward ? pw::transform_backward(value, kind, p0, p1) : pw::transform_forward(value, kind, p0, p1);
    return GPP_OK;
    GPP_CATCH
}
