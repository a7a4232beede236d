// Two small pieces of oi_common.h that a plain host compiler can include as well (tools/ubench/oi_small_check.cpp checks them on the
// CPU): the triangle-index table of the P build and the float32 minimum without NaN handling.
#pragma once

// entry e of a lower triangle stored row by row -> (row i) << 8 | (column p <= i), e = i (i + 1) / 2 + p: the encoding of d_tritab, for
// every union the tile kernels can hold (U_MAXU = 40, 56, 62 rows: 820, 1 596, 1 953 entries).  Generated at compile time; oi_union.h puts it in
// device memory (3.9 KB per translation unit; the 820 entries of the 32-column form are 1.6 KB and stay in cache).
constexpr int TRI_ROWS = 62;
constexpr int TRI_N = TRI_ROWS * (TRI_ROWS + 1) / 2;
struct TriTab { unsigned short v[TRI_N]; };
constexpr TriTab make_tri_tab() {
    TriTab t{};
    int e = 0;
    for(int i = 0; i < TRI_ROWS; ++i)
        for(int p = 0; p <= i; ++p) t.v[e++] = (unsigned short)((i << 8) | p);
    return t;
}

// min(a, b) and min(a, b, c) of float32 numbers without the NaN handling of fminf.  PRECONDITION: no operand is a NaN and none has its
// sign bit set (every operand is +0, a positive subnormal or normal number, or +inf).  fminf has to return the other operand when one is
// a NaN, and for values the compiler cannot prove quiet (anything loaded from memory) it first canonicalises every operand with
// v_max_f32 v, v, v -- three instructions for a minimum of two.  Floats without a sign bit are ordered like their bit patterns read as
// integers, so the minimum is the INTEGER minimum of the patterns (v_min_i32 / v_min3_i32, which the compiler forms itself): the smaller
// operand as it stands, bit for bit what fminf returns for such operands.
// (Round 12 built this first as inline v_min_f32 / v_min3_f32: 131 vector instructions fewer per tile and 2.3 % SLOWER -- the scheduler
//  knows no latency for an inline statement and put every LDS read directly in front of its use, one s_waitcnt lgkmcnt(0) per read, where
//  the reads of a pass issue back to back otherwise.  profiles/oi_union_selection_ab.txt.)
#if defined(__HIPCC__)
#define GPP_SMALL_FN __device__ __forceinline__
#else
#define GPP_SMALL_FN inline
#endif
GPP_SMALL_FN int d_small_bits(float a) { return __builtin_bit_cast(int, a); }
GPP_SMALL_FN float d_small_float(int i) { return __builtin_bit_cast(float, i); }
GPP_SMALL_FN float d_min_pos(float a, float b) {
    const int x = d_small_bits(a), y = d_small_bits(b);
    return d_small_float(y < x ? y : x);
}
GPP_SMALL_FN float d_min3_pos(float a, float b, float c) { return d_min_pos(d_min_pos(a, b), c); }
