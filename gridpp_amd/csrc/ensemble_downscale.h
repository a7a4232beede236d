// ensemble_downscale.hip without its nearest-neighbour search: what gpp_downscale_probability / gpp_mask_threshold_downscale do once
// the nearest input cell of every output cell is known -- the checks of operator, statistic and quantile, the NaN / Count fills of an
// empty input grid or an empty ensemble, the LDS path and the slab path of rows beyond GPP_ENSEMBLE_ROW_CAP.  The direct entry points
// pass the index they compute, the planned ones (downscale_plan.hip) the index a plan holds.
#pragma once
#include <cstddef>
#include <functional>

namespace gpp {

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
