// calc_ranks, sort_rows, reorder_by_ranks and calc_crps on libgridpp_hip.so: the rank of every value within its row (the last axis), the
// sorted rows, ensemble copula coupling and the CRPS of an ensemble.
//
// A header of its own, not part of gridpp.hpp: the reference has none of the four, so a program written for the reference has to ask for
// this header by name.  Valid means finite; valid values compare numerically (-0.0 == +0.0) and equal values are ordered by position, lower
// index first.
#pragma once
#include "gridpp.hpp"

namespace gridpp {

namespace detail {
inline void rows_ranks(const vec& f, size_t rows, size_t len, ivec* ranks, vec* sorted) {
    if(ranks) ranks->assign(rows * len, -1);
    if(sorted) sorted->assign(rows * len, MV);
    if(rows * len)
        check(gpp_calc_ranks(f.data(), (long)rows, (int)len, ranks ? ranks->data() : nullptr, sorted ? sorted->data() : nullptr, GPP_MEM_HOST));
}
inline vec rows_reorder(const vec& v, const vec& t, size_t rows, size_t len) {
    vec out(rows * len, MV);
    if(rows * len) check(gpp_reorder_by_ranks(v.data(), t.data(), (long)rows, (int)len, out.data(), GPP_MEM_HOST));
    return out;
}
inline vec rows_crps(const vec& e, const vec& ref, size_t rows, size_t len) {
    vec out(rows, MV);
    if(rows) check(gpp_calc_crps(e.data(), ref.data(), (long)rows, (int)len, out.data(), GPP_MEM_HOST));
    return out;
}
// row n of a padded [rows][len] result cut back to the length of the ragged row it came from
template <class T>
inline std::vector<std::vector<T>> cut_rows(const std::vector<T>& f, const vec2& like, size_t len) {
    std::vector<std::vector<T>> o(like.size());
    for(size_t n = 0; n < like.size(); n++) o[n].assign(f.begin() + n * len, f.begin() + n * len + like[n].size());
    return o;
}
inline ivec3 unflatten_i(const ivec& f, size_t Y, size_t X, size_t E) {
    ivec3 o(Y, ivec2(X));
    for(size_t y = 0; y < Y; y++)
        for(size_t x = 0; x < X; x++) o[y][x].assign(f.begin() + (y * X + x) * E, f.begin() + (y * X + x + 1) * E);
    return o;
}
inline void same_shape(const vec2& a, const vec2& b) {
    bool same = a.size() == b.size();
    for(size_t n = 0; same && n < a.size(); n++) same = a[n].size() == b[n].size();
    if(!same) throw std::invalid_argument("reorder_by_ranks: values and template must have the same shape");
}
}   // namespace detail

/** The rank of every value of a vector among its valid values: #{valid j : a[j] < a[i]} + #{valid j < i : a[j] == a[i]}; -1 for an invalid value */
inline ivec calc_ranks(const vec& array) {
    ivec r;
    detail::rows_ranks(array, 1, array.size(), &r, nullptr);
    return r;
}
/** The ranks within every row; rows of different lengths are padded with NaN to the longest for the call and come back at their own length */
inline ivec2 calc_ranks(const vec2& array) {
    size_t len;
    const vec f = detail::pad_rows(array, len);
    ivec r;
    detail::rows_ranks(f, array.size(), len, &r, nullptr);
    return detail::cut_rows(r, array, len);
}
/** The ranks within every cell of a cube (Y, X, N) */
inline ivec3 calc_ranks(const vec3& array) {
    size_t Y, X, E;
    const vec f = detail::flatten(array, Y, X, E);
    ivec r;
    detail::rows_ranks(f, Y * X, E, &r, nullptr);
    return detail::unflatten_i(r, Y, X, E);
}

/** A vector in the order of calc_ranks: out[calc_ranks(a)[i]] = a[i] with its bits kept; NaN from the number of valid values on */
inline vec sort_rows(const vec& array) {
    vec s;
    detail::rows_ranks(array, 1, array.size(), nullptr, &s);
    return s;
}
/** Every row sorted; rows of different lengths are padded with NaN to the longest for the call and come back at their own length */
inline vec2 sort_rows(const vec2& array) {
    size_t len;
    const vec f = detail::pad_rows(array, len);
    vec s;
    detail::rows_ranks(f, array.size(), len, nullptr, &s);
    return detail::cut_rows(s, array, len);
}
/** Every cell of a cube (Y, X, N) sorted */
inline vec3 sort_rows(const vec3& array) {
    size_t Y, X, E;
    const vec f = detail::flatten(array, Y, X, E);
    vec s;
    detail::rows_ranks(f, Y * X, E, nullptr, &s);
    return detail::unflatten(s, Y, X, E);
}

/** Ensemble copula coupling (ECC-Q; the Schaake shuffle with a historical template): out[i] = sort_rows(values)[calc_ranks(templ)[i]], NaN
 *  where templ[i] is invalid or its rank is not below the number of valid values.  Ties in the template are broken by position, not at random.
 *  @param values Calibrated values in any order
 *  @param templ The member order to restore; same shape as values (std::invalid_argument otherwise) */
inline vec reorder_by_ranks(const vec& values, const vec& templ) {
    if(values.size() != templ.size()) throw std::invalid_argument("reorder_by_ranks: values and template must have the same shape");
    return detail::rows_reorder(values, templ, 1, values.size());
}
inline vec2 reorder_by_ranks(const vec2& values, const vec2& templ) {
    detail::same_shape(values, templ);
    size_t len, tlen;
    const vec v = detail::pad_rows(values, len), t = detail::pad_rows(templ, tlen);
    return detail::cut_rows(detail::rows_reorder(v, t, values.size(), len), values, len);
}
inline vec3 reorder_by_ranks(const vec3& values, const vec3& templ) {
    if(values.size() != templ.size()) throw std::invalid_argument("reorder_by_ranks: values and template must have the same shape");
    for(size_t y = 0; y < values.size(); y++) detail::same_shape(values[y], templ[y]);
    size_t Y, X, E, Y2, X2, E2;
    const vec v = detail::flatten(values, Y, X, E), t = detail::flatten(templ, Y2, X2, E2);
    return detail::unflatten(detail::rows_reorder(v, t, Y * X, E), Y, X, E);
}

/** The CRPS of an ensemble against one value: (1/N) sum |x_i - y| - (1/(2 N^2)) sum sum |x_i - x_j| over the N valid members, summed in
 *  double in its rank form; NaN when there is no valid member or ref is not finite */
inline float calc_crps(const vec& ensemble, float ref) {
    return detail::rows_crps(ensemble, vec(1, ref), 1, ensemble.size())[0];
}
/** One CRPS per row; ref holds one value per row (std::invalid_argument otherwise); shorter rows are padded with NaN */
inline vec calc_crps(const vec2& ensemble, const vec& ref) {
    if(ref.size() != ensemble.size()) throw std::invalid_argument("calc_crps: ref must have the shape of ensemble without its last axis");
    size_t len;
    const vec f = detail::pad_rows(ensemble, len);
    return detail::rows_crps(f, ref, ensemble.size(), len);
}
/** One CRPS per cell of a cube (Y, X, N); ref is (Y, X) */
inline vec2 calc_crps(const vec3& ensemble, const vec2& ref) {
    bool same = ref.size() == ensemble.size();
    for(size_t y = 0; same && y < ref.size(); y++) same = ref[y].size() == ensemble[y].size();
    if(!same) throw std::invalid_argument("calc_crps: ref must have the shape of ensemble without its last axis");
    size_t Y, X, E, Y2, X2;
    const vec f = detail::flatten(ensemble, Y, X, E), r = detail::flatten(ref, Y2, X2);
    return detail::unflatten(detail::rows_crps(f, r, Y * X, E), Y, X);
}

}   // namespace gridpp
