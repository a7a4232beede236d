// The pair table of an observation index (round 13): rho(observation a, observation b) of a scalar Barnes structure for every pair that can
// meet in one union of k_oi_union, computed once per (point set, structure, window) instead of once per tile.  The value of a pair depends
// on the two positions, elevations and land fractions and on the structure's scalars only -- not on the tile, the grid or the observation
// values -- and the headline evaluates every pair a few hundred times per call.
//
// Layout, on what the index already has (observations sorted by bin, bin_start): for the observation at sorted position a, in bin (bx, by),
// and every dy in [-W, W] the sorted positions of the bins (bx - W .. bx + W, by + dy), clamped at the domain edge, form ONE contiguous range.
// Per observation 2 W + 1 row descriptors {first sorted position, length, offset of the row's values, 0}; the float32 values of every b in
// those ranges, (a, a) included; the bin row of every sorted position.  A lookup is one descriptor load and one value load, no search.  Both
// directions are stored: d_barnes_corr_flat takes the chord and the elevation / land-fraction differences through squares only, so it is
// bitwise symmetric.  The values come from that very helper on the sorted records (k_pair_values, oi.hip): the bits of the P build's own loop.
//
// The table is a cache: a pair it does not hold (window too small, row clamped away) makes the work item redo its P build by evaluation, so
// no result depends on the table being present or complete.  It lives with the index (gpp_obs_index::pair) and is freed with it.
#pragma once
#include "common.h"

constexpr size_t GPP_PAIR_TABLE_CAP = (size_t)128 << 20;   // bytes: half of the 256 MiB Infinity Cache, so that the gathers stay on the chip

struct PairTabArgs {       // what a kernel takes for its lookups; W == 0: no table
    const int4* desc;      // [sorted position][2 W + 1]
    const float* vals;
    const int* brow;       // [sorted position]: bin row
    int W;                 // half-width of the window, in bins
    unsigned ndesc, nvals; // entries of desc / vals (the lookups clamp their addresses against them)
};

struct gpp_pair_table {
    // the key: the resolved scalar structure and the window asked for
    bool built = false;
    int kh = -1, kv = -1, kw = -1, W_asked = 0;
    float h = 0, v = 0, w = 0, R = 0;
    // what that gave (W == 0: nothing fits under the cap, or the allocation failed -- not an error)
    int W = 0;
    size_t bytes = 0;
    unsigned ndesc = 0, nvals = 0;
    gpp::DevBuf<int4> d_desc;
    gpp::DevBuf<float> d_vals;
    gpp::DevBuf<int> d_brow, d_bin_base;
    PairTabArgs args() const { return PairTabArgs{d_desc.p, d_vals.p, d_brow.p, W, ndesc, nvals}; }
};

#ifdef __HIPCC__
// Entry (row i, row p) of a union's P, for the lane that builds it.  ai = (sorted position of row i) * (2 W + 1) and ri / rp = the bin rows
// of the two observations, as their row lanes hold them.  The descriptor index is clamped into the table whatever the inputs; `in` says
// whether row p's bin row lies inside row i's window.
__device__ __forceinline__ unsigned d_pair_desc_index(const PairTabArgs& t, const int ai, const int ri, const int rp, bool& in) {
    const int dy = rp - ri + t.W;
    in = (unsigned)dy <= (unsigned)(2 * t.W);
    return min((unsigned)(ai + max(0, min(dy, 2 * t.W))), t.ndesc - 1u);
}
// ... and the index of the value behind that descriptor for the observation at sorted position pp, clamped likewise; `hit`: the row holds it
__device__ __forceinline__ unsigned d_pair_value_index(const PairTabArgs& t, const int4 d, const int pp, bool& hit) {
    const unsigned k = (unsigned)(pp - d.x);
    hit = k < (unsigned)d.y;
    return min((unsigned)d.z + k, t.nvals - 1u);
}
#endif
