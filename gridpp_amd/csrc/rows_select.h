// Exact quantiles of the rows of a device-resident [rows][len] array (rows_select.hip): the selection behind gpp_calc_quantile,
// the Median of gpp_calc_statistic and the member Median of gpp_neighbourhood; and many levels per row at once (rows_quantiles.hip):
// the sort behind gpp_calc_quantiles.
#pragma once

namespace gpp {

// d_out[r] = calc_quantile(row r, q_r) (src/api/util.cpp:111-178) with the bits of row_quantile (row_stats.h).  q_r = d_q[r] when
// q_per_row, d_q[0] otherwise; d_q == nullptr asks for the median (q = 0.5).  The levels are expected in [0, 1] or NaN (the callers
// check).  Launches on the library stream and returns without waiting for it.
void rows_quantile(const float* d_in, long rows, int len, const float* d_q, int q_per_row, float* d_out);

// true when a device-resident quantile field holds a value below 0 or above 1 (NaN passes): one flag is read back, not the field
bool quantile_out_of_range(const float* d_q, long nq);

// d_out[r * nq + j] = what rows_quantile gives for row r at the level h_levels[j], bit for bit, for nq levels on the HOST (in [0, 1] or
// NaN, in any order, repeats allowed: the callers check the range): rows_quantiles.hip sorts every row once in LDS and picks the levels
// out of it where that pays, and calls rows_quantile once per level otherwise.  Launches on the library stream and returns without
// waiting for it: h_levels stays readable until the caller has synchronised the stream.
void rows_quantiles(const float* d_in, long rows, int len, const float* h_levels, int nq, float* d_out);

}   // namespace gpp

// ---- device helpers shared by rows_select.hip and rows_quantiles.hip ------------------------------------------------------------------
#include "row_stats.h"

#define RS_TILE_MAXLEN 160        // (MEMBER_EC of neighbourhood.hip: rows up to this length are selected out of LDS)
#define RS_INV 0xFFFFFFFFu        // key of an invalid value: no finite float maps to it

__device__ __forceinline__ unsigned rs_key(float v) { return dev_valid(v) ? f2ord(v) : RS_INV; }
__device__ __forceinline__ void rs_indices(float q, int N, int& lo, int& up) {   // util.cpp:152-157
    const float pos = q * (float)(N - 1);
    lo = (int)floorf(pos); up = (int)ceilf(pos);
}
// -0.0 and +0.0 compare equal in row_statistic's Min / Max: one key for both, so that the index decides between them
__device__ __forceinline__ unsigned rs_canon(unsigned k) { return k == 0x7FFFFFFFu ? 0x80000000u : k; }
