// ensemble_downscale.hip without its nearest-neighbour search: what gpp_downscale_probability / gpp_mask_threshold_downscale do once
// the nearest input cell of every output cell is known -- the checks of operator, statistic and quantile, the NaN / Count fills of an
// empty input grid or an empty ensemble, the LDS path and the slab path of rows beyond GPP_ENSEMBLE_ROW_CAP.  The direct entry points
// pass the index they compute, the planned ones (downscale_plan.hip) the index a plan holds.
#pragma once
#include <cstddef>
#include <functional>
#include <type_traits>

namespace gpp {

// The kernels that read a run of E members per cell (the ensemble downscalers here, the cube-layout kernels of a plan) do it with a
// group of G lanes, 64 / G cells per wavefront: the smallest G of 4 ... 64 whose lanes read at most four members each
inline int group_of(int E) {
    for(int g = 4; g < 64; g *= 2) if(E <= 4 * g) return g;
    return 64;
}
// f(std::integral_constant<int, G>{}) for the G that group_of returned: the template argument of such a kernel
template <class F>
void dispatch_group(int G, F&& f) {
    switch(G) {
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        case 16: f(std::integral_constant<int, 16>{}); break;
        case 32: f(std::integral_constant<int, 32>{}); break;
        default: f(std::integral_constant<int, 64>{}); break;
    }
}

// -> a device pointer to the nearest input cell of each of the nq output cells; called at most once, and only when the index is read
// (n_in > 0, ne > 0, after every check has passed)
using NearestIndex = std::function<const int*()>;

// n_in: cells of the input grid; values [n_in][ne]; threshold, out [nq]
void ensemble_probability(const NearestIndex& index, size_t n_in, int nq, const float* values, int ne, const float* threshold,
                          int comparison_operator, float* out, int mem);
void ensemble_mask_threshold(const NearestIndex& index, size_t n_in, int nq, const float* ivalues_true, const float* ivalues_false,
                             const float* threshold_values, int ne, const float* threshold, int comparison_operator, int statistic,
                             float quantile, float* out, int mem);

}   // namespace gpp
