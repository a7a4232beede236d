// Exact quantiles of the rows of a device-resident [rows][len] array (rows_select.hip): the selection behind gpp_calc_quantile,
// the Median of gpp_calc_statistic and the member Median of gpp_neighbourhood.
#pragma once

namespace gpp {

// d_out[r] = calc_quantile(row r, q_r) (src/api/util.cpp:111-178) with the bits of row_quantile (row_stats.h).  q_r = d_q[r] when
// q_per_row, d_q[0] otherwise; d_q == nullptr asks for the median (q = 0.5).  The levels are expected in [0, 1] or NaN (the callers
// check).  Launches on the library stream and returns without waiting for it.
void rows_quantile(const float* d_in, long rows, int len, const float* d_q, int q_per_row, float* d_out);

// true when a device-resident quantile field holds a value below 0 or above 1 (NaN passes): one flag is read back, not the field
bool quantile_out_of_range(const float* d_q, long nq);

}   // namespace gpp
