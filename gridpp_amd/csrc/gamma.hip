// gridpp::gamma_inv (src/api/distribution.cpp:5-33) and gridpp::Gamma::forward / backward (src/api/transform.cpp:155-179) for gfx950:
// element-wise over n values.  The per-value arithmetic is gamma_fn.h, shared by the kernels and the host-only scalar entry points
// (gpp_gamma_inv_scalar, gpp_gamma_transform_scalar).
//
//   k_gamma_inv<IN64>                   three input arrays, one value per lane and step; GPP_GAMMA_BLOCK lanes per workgroup, at most
//                                       GPP_GAMMA_MAX_BLOCKS workgroups, a grid stride beyond that.  An offending element does a global
//                                       atomicMin of (index << 2) | code on one 64-bit status word (all ones before the launch) and
//                                       gets NaN; the host reads the word after the stream has run, fetches that one value and reports
//                                       it with the reference's text.  The kernel never traps.
//   k_gamma_transform<BACKWARD, IN64>   one input array; shape, scale, tolerance and lgamma(shape) travel by value.
//
// IN64: the staged inputs of a GPP_HOST_F64 call are doubles and are rounded to float32 as the first operation.  No LDS.  One value
// per lane and 4-byte accesses: these kernels are bound by double arithmetic and by the slowest lane of a wave (the lanes of a wave
// need different numbers of series terms and of Newton steps), not by bytes, so there is no 16-byte path.
#include "common.h"
#include "gamma_fn.h"
#include <cstdint>
#include <sstream>

using namespace gpp;

namespace {

namespace gm = gpp::gamma_fn;

template <bool IN64>
__device__ inline float load(const void* p, long long i) {
    return IN64 ? (float)static_cast<const double*>(p)[i] : static_cast<const float*>(p)[i];   // the cast is the typemap's rounding
}

template <bool IN64>
__global__ __launch_bounds__(GPP_GAMMA_BLOCK) void k_gamma_inv(const void* __restrict__ levels, const void* __restrict__ shape, const void* __restrict__ scale,
                                                               long long n, float* __restrict__ out, unsigned long long* __restrict__ status) {
    const long long stride = (long long)gridDim.x * GPP_GAMMA_BLOCK;
    for(long long i = (long long)blockIdx.x * GPP_GAMMA_BLOCK + threadIdx.x; i < n; i += stride) {
        int code = 0;
        const float v = gm::gamma_inv(load<IN64>(levels, i), load<IN64>(shape, i), load<IN64>(scale, i), &code);
        if(code != 0) atomicMin(status, ((unsigned long long)i << 2) | (unsigned long long)code);
        out[i] = v;   // NaN for an offending element
    }
}

template <bool BACKWARD, bool IN64>
__global__ __launch_bounds__(GPP_GAMMA_BLOCK) void k_gamma_transform(const void* __restrict__ in, long long n, gm::GammaParams g, float* __restrict__ out) {
    const long long stride = (long long)gridDim.x * GPP_GAMMA_BLOCK;
    for(long long i = (long long)blockIdx.x * GPP_GAMMA_BLOCK + threadIdx.x; i < n; i += stride) {
        const float v = load<IN64>(in, i);
        out[i] = BACKWARD ? gm::transform_backward(v, g) : gm::transform_forward(v, g);
    }
}

struct GammaWorkspace {
    DevBuf<unsigned long long> status;   // the one status word of a gamma_inv call
};
thread_local GammaWorkspace g_gamma;

// the inputs of a call (`mem`) as device pointers: the caller's, or staged float32 / float64 copies
template <int NIN>
struct DeviceInputs {
    Staged<float> narrow[NIN];
    Staged<double> wide[NIN];
    const void* p[NIN];
    bool f64;
    DeviceInputs(const float* const* arrays, long long n, int mem) : f64(!(mem & GPP_MEM_DEVICE) && (mem & GPP_HOST_F64)) {
        for(int a = 0; a < NIN; a++) {
            if(mem & GPP_MEM_DEVICE) p[a] = arrays[a];
            else if(f64) { wide[a].upload(reinterpret_cast<const double*>(arrays[a]), (size_t)n); p[a] = wide[a].p; }
            else { narrow[a].upload(arrays[a], (size_t)n); p[a] = narrow[a].p; }
        }
    }
};

template <int NIN>
void check_arrays(const float* const* arrays, long long n, const float* out) {
    if(n < 0) invalid("negative number of values");
    if(n == 0) return;
    for(int a = 0; a < NIN; a++)
        if(!arrays[a]) invalid("an input array is NULL");
    if(!out) invalid("out is NULL");
}

// distribution.cpp:9-21: `ss << value` of a float
std::string gamma_inv_message(int code, float value) {
    std::stringstream ss;
    switch(code) {
        case gm::GAMMA_LEVEL: ss << "Invalid level '" << value << "'. Levels must be on the interval [0, 1]."; break;
        case gm::GAMMA_SHAPE: ss << "Invalid shape '" << value << "'. Shapes must be > 0."; break;
        default: ss << "Invalid scale '" << value << "'. Scale must be > 0."; break;
    }
    return ss.str();
}

// element i of an input of the call, as the kernel saw it
float fetch(const float* array, long long i, int mem) {
    if(mem & GPP_MEM_DEVICE) {
        float v = NAN;
        GPP_HIP(hipMemcpyAsync(&v, array + i, sizeof(float), hipMemcpyDeviceToHost, stream()));
        GPP_HIP(hipStreamSynchronize(stream()));
        return v;
    }
    return (mem & GPP_HOST_F64) ? (float)reinterpret_cast<const double*>(array)[i] : array[i];
}

// transform.cpp:158-163
gm::GammaParams gamma_params(float shape, float scale, float tolerance) {
    if(!gm::valid(shape) || shape <= 0) invalid("Shape parameter must be > 0 in the gamma distribution");
    if(!gm::valid(scale) || scale <= 0) invalid("Scale parameter must be > 0 in the gamma distribution");
    if(!gm::valid(tolerance) || tolerance < 0) invalid("Tolerance must be >= 0 in the gamma distribution");
    return gm::GammaParams{shape, scale, tolerance, std::lgamma((double)shape)};
}

}   // namespace

extern "C" int gpp_gamma_inv(const float* levels, const float* shape, const float* scale, long long n, float* out, int mem) {
    GPP_TRY
    const float* arrays[3] = {levels, shape, scale};
    check_arrays<3>(arrays, n, out);
    if(n == 0) return GPP_OK;
    ensure_device();
    DeviceInputs<3> in(arrays, n, mem);
    OutField o;
    o.bind(out, (size_t)n, mem);
    unsigned long long* status = g_gamma.status.get(1);
    GPP_HIP(hipMemsetAsync(status, 0xFF, sizeof(unsigned long long), stream()));
    const unsigned grid = grid_capped(blocks_of(n, GPP_GAMMA_BLOCK), GPP_GAMMA_MAX_BLOCKS);
    if(in.f64) launch(k_gamma_inv<true>, grid, GPP_GAMMA_BLOCK, 0, in.p[0], in.p[1], in.p[2], n, o.d, status);
    else launch(k_gamma_inv<false>, grid, GPP_GAMMA_BLOCK, 0, in.p[0], in.p[1], in.p[2], n, o.d, status);
    o.finish();
    unsigned long long word = ~0ull;
    GPP_HIP(hipMemcpyAsync(&word, status, sizeof(word), hipMemcpyDeviceToHost, stream()));
    GPP_HIP(hipStreamSynchronize(stream()));
    if(word != ~0ull) {
        const int code = (int)(word & 3);
        invalid(gamma_inv_message(code, fetch(arrays[code - 1], (long long)(word >> 2), mem)));
    }
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_gamma_transform(const float* in, long long n, int backward, float shape, float scale, float tolerance, float* out, int mem) {
    GPP_TRY
    const gm::GammaParams g = gamma_params(shape, scale, tolerance);
    const float* arrays[1] = {in};
    check_arrays<1>(arrays, n, out);
    if(n == 0) return GPP_OK;
    ensure_device();
    DeviceInputs<1> src(arrays, n, mem);
    OutField o;
    o.bind(out, (size_t)n, mem);
    const dim3 grid(grid_capped(blocks_of(n, GPP_GAMMA_BLOCK), GPP_GAMMA_MAX_BLOCKS)), block(GPP_GAMMA_BLOCK);
    if(backward) {
        if(src.f64) launch(k_gamma_transform<true, true>, grid, block, 0, src.p[0], n, g, o.d);
        else launch(k_gamma_transform<true, false>, grid, block, 0, src.p[0], n, g, o.d);
    }
    else {
        if(src.f64) launch(k_gamma_transform<false, true>, grid, block, 0, src.p[0], n, g, o.d);
        else launch(k_gamma_transform<false, false>, grid, block, 0, src.p[0], n, g, o.d);
    }
    return finish_call(o);
    GPP_CATCH
}

// ---- host-only forms ----------------------------------------------------------------------------------------------------------
extern "C" int gpp_gamma_inv_scalar(float level, float shape, float scale, float* out) {
    GPP_TRY
    if(!out) invalid("out is NULL");
    int code = 0;
    const float y = gm::gamma_inv(level, shape, scale, &code);
    if(code != 0) invalid(gamma_inv_message(code, code == gm::GAMMA_LEVEL ? level : code == gm::GAMMA_SHAPE ? shape : scale));
    *out = y;
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_gamma_transform_scalar(float value, int backward, float shape, float scale, float tolerance, float* out) {
    GPP_TRY
    const gm::GammaParams g = gamma_params(shape, scale, tolerance);
    if(!out) invalid("out is NULL");
    *out = backward ? gm::transform_backward(value, g) : gm::transform_forward(value, g);
    return GPP_OK;
    GPP_CATCH
}
