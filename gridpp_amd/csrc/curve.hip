// gridpp::apply_curve (src/api/curve.cpp:6-133), gridpp::interpolate (src/api/util.cpp:339-426), gridpp::monotonize_curve
// (curve.cpp:134-250) and gridpp::quantile_mapping_curve (src/api/quantile_mapping.cpp:5-46) for gfx950.
//
// The per-value arithmetic is curve.h, shared by the kernels and the host-only scalar entry points.
//
//   k_curve_shared<LDS, VEC>   one curve for all values (apply_curve with a vec curve, interpolate): element-wise, VEC = 4 values
//                              per lane and step through 16-byte loads and stores.  The curve is staged in LDS while both halves fit
//                              CURVE_LDS_FLOATS, read through the caches beyond that.  The host tests the curve once per call: sorted
//                              and free of invalid entries -> bisection, anything else -> the reference's two linear scans.
//   k_apply_curve_field<G, W>  one curve per cell, curves (Y, X, C) with C contiguous.  A group of G lanes owns a cell (64 / G cells
//                              per wavefront) and reads curve_fcst's run with unit stride, W entries per lane and step (8- and
//                              16-byte loads where 4 C and the slab's address allow).  The two scan indices come from group ballots
//                              instead of a serial walk: with S = the first valid entry >= x, the lower index is S where it equals
//                              x, else the last valid entry before S; with T = the last valid entry <= x, the upper index is T where
//                              it equals x, else the first valid entry after T.  Every lane of the group holds the same state, the
//                              four values the indices select are a second, cache-hot load; curve_ref is read only there.
#include "common.h"
#include "curve.h"
#include <algorithm>
#include <cstdint>

using namespace gpp;

namespace {

constexpr int CURVE_LDS_FLOATS = 8192;   // both halves of a staged curve: 32 KiB per workgroup
constexpr int SHARED_BLOCK = 1024;

template <bool LDS, int VEC>
__global__ __launch_bounds__(SHARED_BLOCK) void k_curve_shared(const float* __restrict__ in, long long nvec, const float* __restrict__ cx,
                                                               const float* __restrict__ cy, int nc, int policy_below, int policy_above,
                                                               int sorted, int interp, float* __restrict__ out) {
    extern __shared__ float staged[];
    const float *X = cx, *Y = cy;
    if(LDS) {
        for(int i = threadIdx.x; i < nc; i += blockDim.x) {
            staged[i] = cx[i];
            staged[nc + i] = cy[i];
        }
        __syncthreads();
        X = staged;
        Y = staged + nc;
    }
    const long long stride = (long long)gridDim.x * blockDim.x;
    for(long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        float v[VEC], o[VEC];
        if(VEC == 4) {
            const float4 q = reinterpret_cast<const float4*>(in)[i];
            v[0] = q.x; v[1 % VEC] = q.y; v[2 % VEC] = q.z; v[3 % VEC] = q.w;
        }
        else v[0] = in[i];
#pragma unroll
        for(int k = 0; k < VEC; k++)
            o[k] = interp ? curve::interpolate(v[k], X, Y, nc, sorted != 0)
                          : curve::apply(v[k], Y, X, nc, policy_below, policy_above, sorted != 0, nullptr);
        if(VEC == 4) reinterpret_cast<float4*>(out)[i] = make_float4(o[0], o[1 % VEC], o[2 % VEC], o[3 % VEC]);
        else out[i] = o[0];
    }
}

// masks of one lane's W entries, packed: valid | valid and >= x | valid and <= x | valid and == x, four bits each
template <int W>
__device__ __forceinline__ unsigned entry_masks(const float (&v)[W], float x) {
    unsigned p = 0;
#pragma unroll
    for(int c = 0; c < W; c++) {
        const bool ok = curve::valid(v[c]);
        p |= (ok ? 1u : 0u) << c;
        p |= ((ok && v[c] >= x) ? 1u : 0u) << (4 + c);
        p |= ((ok && v[c] <= x) ? 1u : 0u) << (8 + c);
        p |= ((ok && v[c] == x) ? 1u : 0u) << (12 + c);
    }
    return p;
}
__device__ __forceinline__ int low_bit(unsigned m) { return __ffs(m) - 1; }
__device__ __forceinline__ int high_bit(unsigned m) { return 31 - __clz(m); }
__device__ __forceinline__ int low_bit64(unsigned long long m) { return __ffsll(m) - 1; }
__device__ __forceinline__ int high_bit64(unsigned long long m) { return 63 - __clzll(m); }

template <int G, int W>
__global__ __launch_bounds__(256) void k_apply_curve_field(const float* __restrict__ in, const float* __restrict__ curve_ref,
                                                           const float* __restrict__ curve_fcst, long long ncell, int nc, int policy_below,
                                                           int policy_above, float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long cell = t / G;
    const int lane = (int)(t % G);
    const bool active = cell < ncell;
    const int gshift = (threadIdx.x & 63) & ~(G - 1);   // the group's first lane within its wavefront
    const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << (G % 64)) - 1);
    const float* f = curve_fcst + (active ? (size_t)cell * nc : 0);
    const float* r = curve_ref + (active ? (size_t)cell * nc : 0);
    const float x = active ? in[cell] : NAN;
    const float f0 = active ? f[0] : NAN, fl = active ? f[nc - 1] : NAN;
    const bool inrange = x >= f0 && x <= fl;       // curve.cpp:22
    const bool scan = inrange && curve::valid(x);  // util.cpp:378
    // group-uniform scan state: S / T as above (-1: none yet), s_eq / t_eq: that entry equals x, prev: the last valid entry before S
    // (while S is missing: so far), next: the first valid entry after T (-1: none yet)
    int S = -1, prev = -1, T = -1, next = -1;
    bool s_eq = false, t_eq = false;
    for(int b0 = 0; b0 < nc; b0 += G * W) {
        const int e0 = b0 + lane * W;
        float v[W];
#pragma unroll
        for(int c = 0; c < W; c++) v[c] = NAN;
        if(scan && e0 < nc) {   // nc is a multiple of W (the launcher's business): the lane's W entries are all inside
            if(W == 4) {
                const float4 q = *reinterpret_cast<const float4*>(f + e0);
                v[0] = q.x; v[1 % W] = q.y; v[2 % W] = q.z; v[3 % W] = q.w;
            }
            else if(W == 2) {
                const float2 q = *reinterpret_cast<const float2*>(f + e0);
                v[0] = q.x; v[1 % W] = q.y;
            }
            else v[0] = f[e0];
        }
        const unsigned p = entry_masks<W>(v, x);
        const unsigned long long BV = (__ballot((p & 15u) != 0) >> gshift) & gmask;
        const unsigned long long BGE = (__ballot(((p >> 4) & 15u) != 0) >> gshift) & gmask;
        const unsigned long long BLE = (__ballot(((p >> 8) & 15u) != 0) >> gshift) & gmask;
        if(S < 0) {
            if(BGE) {
                const int L = low_bit64(BGE);
                const unsigned pl = (unsigned)__shfl((int)p, L, G);
                const int c = low_bit((pl >> 4) & 15u);
                S = b0 + L * W + c;
                s_eq = ((pl >> (12 + c)) & 1u) != 0;
                const unsigned before = (pl & 15u) & ((1u << c) - 1);
                if(before) prev = b0 + L * W + high_bit(before);
                else {
                    const unsigned long long lanes_before = BV & ((1ull << L) - 1);
                    if(lanes_before) {
                        const int L2 = high_bit64(lanes_before);
                        prev = b0 + L2 * W + high_bit((unsigned)__shfl((int)p, L2, G) & 15u);
                    }
                }
            }
            else if(BV) {
                const int L2 = high_bit64(BV);
                prev = b0 + L2 * W + high_bit((unsigned)__shfl((int)p, L2, G) & 15u);
            }
        }
        if(BLE) {
            const int L = high_bit64(BLE);
            const unsigned pl = (unsigned)__shfl((int)p, L, G);
            const int c = high_bit((pl >> 8) & 15u);
            T = b0 + L * W + c;
            t_eq = ((pl >> (12 + c)) & 1u) != 0;
            const unsigned after = (pl & 15u) & ~((2u << c) - 1);
            next = -1;
            if(after) next = b0 + L * W + low_bit(after);
            else {
                const unsigned long long lanes_after = L >= 63 ? 0ull : (BV & ~((2ull << L) - 1));
                if(lanes_after) {
                    const int L2 = low_bit64(lanes_after);
                    next = b0 + L2 * W + low_bit((unsigned)__shfl((int)p, L2, G) & 15u);
                }
            }
        }
        else if(next < 0 && BV) {
            const int L2 = low_bit64(BV);
            next = b0 + L2 * W + low_bit((unsigned)__shfl((int)p, L2, G) & 15u);
        }
    }
    if(!active) return;
    float y;
    if(scan) {
        const int i0 = s_eq ? S : prev, i1 = t_eq ? T : next;
        y = NAN;
        if(i0 >= 0 && i1 >= 0) y = curve::between(x, i0, i1, nc, f[i0], f[i1], r[i0], r[i1]);
    }
    else if(inrange) y = NAN;   // an infinite input between infinite ends: util.cpp:378
    else y = curve::extrapolate(x, r, f, nc, policy_below, policy_above, nullptr);
    if(lane == 0) out[cell] = y;
}

void check_policies(int policy_below, int policy_above) {
    if(!curve::known_policy(policy_below) || !curve::known_policy(policy_above)) invalid("Unknown extrapolation policy");
}
void check_curve_sizes(int nc_ref, int nc_fcst) {   // curve.cpp:7-10
    if(nc_ref != nc_fcst) invalid("curve_ref and curve_fcst must be the same size");
    if(nc_ref <= 0) invalid("curve_ref and curve_fcst cannot have size 0");
}

int compute_units() {
    static int cus = 0;
    if(cus == 0) {
        int dev = 0, n = 0;
        GPP_HIP(hipGetDevice(&dev));
        GPP_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        cus = n > 0 ? n : 256;
    }
    return cus;
}

template <bool LDS, int VEC>
void launch_shared(const float* in, long long nvec, const float* cx, const float* cy, int nc, int pb, int pa, int sorted, int interp, float* out) {
    if(nvec <= 0) return;
    // a staged curve is loaded once per workgroup: two resident workgroups per compute unit walk the values with a grid stride
    const unsigned blocks = grid_capped(blocks_of(nvec, SHARED_BLOCK), (size_t)compute_units() * 2);
    const size_t lds = LDS ? (size_t)2 * nc * sizeof(float) : 0;
    launch(k_curve_shared<LDS, VEC>, blocks, SHARED_BLOCK, lds, in, nvec, cx, cy, nc, pb, pa, sorted, interp, out);
}

// values `in` (n of them, `mem`) through the host curve (cx -> cy): apply_curve (interp = 0: cx = curve_fcst, cy = curve_ref) or interpolate
void run_shared(const float* in, long long n, const float* cx, const float* cy, int nc, int pb, int pa, int interp, float* out, int mem) {
    ensure_device();
    InField v;
    OutField o;
    v.bind(in, (size_t)n, mem);
    o.bind(out, (size_t)n, mem);
    Staged<float> c;
    c.get((size_t)2 * std::max(nc, 1));
    if(nc > 0) {
        GPP_HIP(hipMemcpyAsync(c.p, cx, (size_t)nc * sizeof(float), hipMemcpyHostToDevice, stream()));
        GPP_HIP(hipMemcpyAsync(c.p + nc, cy, (size_t)nc * sizeof(float), hipMemcpyHostToDevice, stream()));
    }
    const int sorted = curve::valid_and_sorted(cx, nc) ? 1 : 0;
    const bool lds = 2 * (long long)nc <= CURVE_LDS_FLOATS;
    const bool wide = (((uintptr_t)v.d | (uintptr_t)o.d) & 15) == 0;
    const long long n4 = wide ? n / 4 : 0;
    if(lds) {
        launch_shared<true, 4>(v.d, n4, c.p, c.p + nc, nc, pb, pa, sorted, interp, o.d);
        launch_shared<true, 1>(v.d + 4 * n4, n - 4 * n4, c.p, c.p + nc, nc, pb, pa, sorted, interp, o.d + 4 * n4);
    }
    else {
        launch_shared<false, 4>(v.d, n4, c.p, c.p + nc, nc, pb, pa, sorted, interp, o.d);
        launch_shared<false, 1>(v.d + 4 * n4, n - 4 * n4, c.p, c.p + nc, nc, pb, pa, sorted, interp, o.d + 4 * n4);
    }
    finish_call(o);
}

template <int G, int W>
void launch_field(const float* in, const float* ref, const float* fcst, long long ncell, int nc, int pb, int pa, float* out) {
    const long long blocks = blocks_of(ncell * G);
    launch(k_apply_curve_field<G, W>, (unsigned)blocks, 256, 0, in, ref, fcst, ncell, nc, pb, pa, out);
}
template <int W>
void launch_field_w(const float* in, const float* ref, const float* fcst, long long ncell, int nc, int pb, int pa, float* out) {
    // lanes per cell: the smallest group that covers the run in one step, 64 beyond that (a chunked loop)
    int g = 4;
    while(g < 64 && g * W < nc) g *= 2;
    switch(g) {
        case 4: launch_field<4, W>(in, ref, fcst, ncell, nc, pb, pa, out); break;
        case 8: launch_field<8, W>(in, ref, fcst, ncell, nc, pb, pa, out); break;
        case 16: launch_field<16, W>(in, ref, fcst, ncell, nc, pb, pa, out); break;
        case 32: launch_field<32, W>(in, ref, fcst, ncell, nc, pb, pa, out); break;
        default: launch_field<64, W>(in, ref, fcst, ncell, nc, pb, pa, out); break;
    }
}

}   // namespace

extern "C" int gpp_apply_curve(const float* fcst, long long n, const float* curve_ref, int nc_ref, const float* curve_fcst, int nc_fcst,
                               int policy_below, int policy_above, float* out, int mem) {
    GPP_TRY
    check_curve_sizes(nc_ref, nc_fcst);
    check_policies(policy_below, policy_above);
    if(!curve_ref || !curve_fcst) invalid("curve is NULL");
    if(n < 0) invalid("negative number of values");
    if(n == 0) return GPP_OK;
    if(!fcst || !out) invalid("fcst / out is NULL");
    run_shared(fcst, n, curve_fcst, curve_ref, nc_ref, policy_below, policy_above, 0, out, mem);
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_interpolate(const float* x, long long n, const float* ix, int nc_x, const float* iy, int nc_y, float* out, int mem) {
    GPP_TRY
    if(nc_x != nc_y) invalid("Dimension mismatch. Cannot interpolate.");   // util.cpp:416-417
    if(nc_x < 0) invalid("negative curve size");
    if(nc_x > 0 && (!ix || !iy)) invalid("curve is NULL");
    if(n < 0) invalid("negative number of values");
    if(n == 0) return GPP_OK;
    if(!x || !out) invalid("x / out is NULL");
    run_shared(x, n, ix, iy, nc_x, GPP_ONE_TO_ONE, GPP_ONE_TO_ONE, 1, out, mem);
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_apply_curve_field(const float* fcst, const float* curve_ref, const float* curve_fcst, int ny, int nx, int nc_ref, int nc_fcst,
                                     int policy_below, int policy_above, float* out, int mem) {
    GPP_TRY
    if(nc_ref != nc_fcst) invalid("curve_ref and curve_fcst dimension sizes mismatch");   // curve.cpp:111-112
    if(nc_ref <= 0) invalid("curve_ref and curve_fcst cannot have size 0");
    check_policies(policy_below, policy_above);
    if(ny < 0 || nx < 0) invalid("negative field size");
    const long long ncell = (long long)ny * nx;
    if(ncell == 0) return GPP_OK;
    if(!fcst || !curve_ref || !curve_fcst || !out) invalid("a field is NULL");
    ensure_device();
    const int nc = nc_ref;
    InField v, r, f;
    OutField o;
    v.bind(fcst, (size_t)ncell, mem);
    r.bind(curve_ref, (size_t)ncell * nc, mem);
    f.bind(curve_fcst, (size_t)ncell * nc, mem);
    o.bind(out, (size_t)ncell, mem);
    // entries per lane and load: the widest that divides the run and keeps every cell's run aligned
    const uintptr_t a = (uintptr_t)f.d;
    if(nc % 4 == 0 && a % 16 == 0) launch_field_w<4>(v.d, r.d, f.d, ncell, nc, policy_below, policy_above, o.d);
    else if(nc % 2 == 0 && a % 8 == 0) launch_field_w<2>(v.d, r.d, f.d, ncell, nc, policy_below, policy_above, o.d);
    else launch_field_w<1>(v.d, r.d, f.d, ncell, nc, policy_below, policy_above, o.d);
    return finish_call(o);
    GPP_CATCH
}

// ---- host-only forms ----------------------------------------------------------------------------------------------------------
extern "C" int gpp_apply_curve_scalar(float input, const float* curve_ref, int nc_ref, const float* curve_fcst, int nc_fcst, int policy_below,
                                      int policy_above, float* out) {
    GPP_TRY
    check_curve_sizes(nc_ref, nc_fcst);
    if(!curve_ref || !curve_fcst || !out) invalid("curve / out is NULL");
    bool unknown = false;
    const float y = curve::apply(input, curve_ref, curve_fcst, nc_ref, policy_below, policy_above, curve::valid_and_sorted(curve_fcst, nc_fcst),
                                 &unknown);
    if(unknown) invalid("Unknown extrapolation policy");   // curve.cpp:70-72: only where the input extrapolates with it
    *out = y;
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_interpolate_scalar(float x, const float* ix, int nc_x, const float* iy, int nc_y, float* out) {
    GPP_TRY
    if(!out) invalid("out is NULL");
    if(!curve::valid(x)) { *out = NAN; return GPP_OK; }   // util.cpp:378-379, before the sizes are compared
    if(nc_x != nc_y) invalid("Dimension mismatch. Cannot interpolate.");
    if(nc_x < 0) invalid("negative curve size");
    if(nc_x > 0 && (!ix || !iy)) invalid("curve is NULL");
    *out = curve::interpolate(x, ix, iy, nc_x, curve::valid_and_sorted(ix, nc_x));
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_monotonize_curve(const float* curve_ref_in, int nc_ref, const float* curve_fcst_in, int nc_fcst, float* out_ref, float* out_fcst,
                                    int* count) {
    GPP_TRY
    check_curve_sizes(nc_ref, nc_fcst);
    if(!curve_ref_in || !curve_fcst_in || !out_ref || !out_fcst || !count) invalid("an argument is NULL");
    // curve.cpp:142-161: pairs with a missing member are dropped
    std::vector<float> curve_ref, curve_fcst;
    for(int i = 0; i < nc_ref; i++)
        if(curve::valid(curve_fcst_in[i]) && curve::valid(curve_ref_in[i])) {
            curve_ref.push_back(curve_ref_in[i]);
            curve_fcst.push_back(curve_fcst_in[i]);
        }
    const int N = (int)curve_ref.size();
    *count = 0;
    if(N == 0) return GPP_OK;   // (the reference reads curve_fcst[0] of an empty vector here)
    // curve.cpp:163-238: a deviation is a stretch whose x values do not increase; every point inside one is removed
    std::vector<int> new_indices;
    new_indices.reserve(N);
    float prev = curve_fcst[0];
    bool deviation = false;
    float x_min = curve_fcst[0], x_max = curve_fcst[0];
    new_indices.push_back(0);
    const float tol = 0.1f;
    for(int i = 1; i < N; i++) {
        const float x = curve_fcst[i];
        if(deviation) {
            if(x < x_min) x_min = x;
            if(x > x_max + tol) {   // past the deviation: remove the kept points inside it, that is all points above x_min
                x_max = x;
                for(int j = (int)new_indices.size() - 1; j >= 0; j--) {
                    if(curve_fcst[new_indices[j]] < x_min - tol) break;
                    new_indices.pop_back();
                }
                new_indices.push_back(i);
                deviation = false;
                prev = x;
                x_max = x;
            }
        }
        else {
            if(x <= prev + tol) {
                deviation = true;
                x_min = x;
            }
            else {
                new_indices.push_back(i);
                prev = x;
                x_max = x;
            }
        }
    }
    if(deviation) {   // finished inside a deviation (:227-238; the loop pops the LAST entry for every kept point >= x_min, as there)
        for(int j = (int)new_indices.size() - 1; j >= 0; j--) {
            if(curve_fcst[new_indices[j]] >= x_min) new_indices.pop_back();
        }
    }
    for(size_t i = 0; i < new_indices.size(); i++) {
        out_ref[i] = curve_ref[new_indices[i]];
        out_fcst[i] = curve_fcst[new_indices[i]];
    }
    *count = (int)new_indices.size();
    return GPP_OK;
    GPP_CATCH
}

extern "C" int gpp_quantile_mapping_curve(const float* ref, int n_ref, const float* fcst, int n_fcst, const float* quantiles, int nq, float* out_ref,
                                          float* out_fcst, int* count) {
    GPP_TRY
    if(n_ref != n_fcst) invalid("ref and fcst must be of the same size");
    if(n_ref < 0 || nq < 0) invalid("negative size");
    if(nq > 0 && !quantiles) invalid("quantiles is NULL");
    for(int i = 0; i < nq; i++) {
        const float q = quantiles[i];
        if(!curve::valid(q) || q > 1 || q < 0) invalid("Quantiles must be >= 0 and <= 1");
    }
    if(!count) invalid("count is NULL");
    *count = 0;
    if(n_ref == 0) return GPP_OK;
    if(!ref || !fcst || !out_ref || !out_fcst) invalid("an argument is NULL");
    const int S = n_ref;
    if(S == 1 || nq == 0) {
        std::copy(ref, ref + S, out_ref);
        std::copy(fcst, fcst + S, out_fcst);
        if(S > 1) {   // NaN (no order in the reference's std::sort) goes last
            auto less = [](float a, float b) { return a < b || (a == a && b != b); };
            std::sort(out_ref, out_ref + S, less);
            std::sort(out_fcst, out_fcst + S, less);
        }
        *count = S;
        return GPP_OK;
    }
    for(int i = 0; i < nq; i++) {
        const int index = (int)(quantiles[i] * (float)(S - 1));   // quantile_mapping.cpp:40-42: indexes the inputs as given, not the sorted copies
        out_fcst[i] = fcst[index];
        out_ref[i] = ref[index];
    }
    *count = nq;
    return GPP_OK;
    GPP_CATCH
}
