// gridpp::DownscalingPlan -- the reusable plan of the downscalers (include/gridpp_hip.h: gpp_downscale_plan_*).  No
// counterpart in the reference's gridpp.h, hence a header of its own beside gridpp.hpp (which it includes): everything of downscaling,
// simple_gradient and full_gradient that depends on no value -- the nearest grid point of every output location and, for Bilinear, its box
// and weights -- is computed once by the constructor, and the methods downscale any number of fields with it, each result bit for bit
// that of the direct call.
//
//     gridpp::DownscalingPlan plan(igrid, ogrid, gridpp::Bilinear);
//     vec2 out = plan.apply(values);              // = downscaling(igrid, ogrid, values, Bilinear)
//     vec3 ens = plan.apply_cube(values_yxe);     // an ensemble in gridpp's cube layout, the member index innermost
//     vec2 t2m = plan.full_gradient(values, elev_gradient, laf_gradient);
//
// A plan built for a Grid output answers apply / apply_cube / simple_gradient / full_gradient, one built for a Points output the same
// names with the suffix _points (C++ cannot overload on the result alone).  The plan holds 4 (Nearest) or 16 (Bilinear) bytes of HBM per
// output location and copies of both sets' elevations and land area fractions (nbytes()) until it is destroyed; the Grid / Points it was
// built from may be destroyed first.  A box whose weights leave [0, 1] does not fail the constructor (distorted() counts them): the
// methods throw std::runtime_error where the direct calls do.
#pragma once
#include "gridpp.hpp"

namespace gridpp {
class DownscalingPlan {
  public:
    DownscalingPlan(const Grid& igrid, const Grid& ogrid, Downscaler downscaler = Nearest)
        : mGrid(true), mY(igrid.size()[0]), mX(igrid.size()[1]), mOY(ogrid.size()[0]), mOX(ogrid.size()[1]) {
        create(igrid, ogrid.handle(), ogrid.get_coordinate_type(), downscaler);
    }
    DownscalingPlan(const Grid& igrid, const Points& opoints, Downscaler downscaler = Nearest)
        : mGrid(false), mY(igrid.size()[0]), mX(igrid.size()[1]), mOY(opoints.size()), mOX(1) {
        create(igrid, opoints.handle(), opoints.get_coordinate_type(), downscaler);
    }
    ~DownscalingPlan() { release(); }
    DownscalingPlan(const DownscalingPlan&) = delete;
    DownscalingPlan& operator=(const DownscalingPlan&) = delete;
    DownscalingPlan(DownscalingPlan&& o) noexcept : mGrid(o.mGrid), mY(o.mY), mX(o.mX), mOY(o.mOY), mOX(o.mOX), mP(o.mP) { o.mP = nullptr; }
    DownscalingPlan& operator=(DownscalingPlan&& o) noexcept {
        if(this != &o) {
            release();
            mGrid = o.mGrid; mY = o.mY; mX = o.mX; mOY = o.mOY; mOX = o.mOX; mP = o.mP;
            o.mP = nullptr;
        }
        return *this;
    }

    // ---- a Grid output ----
    vec2 apply(const vec2& ivalues) const { need_grid(true); return detail::unflatten(level(0, ivalues, nullptr, nullptr, 0), mOY, mOX); }
    vec3 apply(const vec3& ivalues) const { need_grid(true); size_t T; vec o = levels(0, ivalues, nullptr, nullptr, 0, T); return detail::unflatten(o, T, mOY, mOX); }
    vec3 apply_cube(const vec3& ivalues) const { need_grid(true); size_t E; vec o = cube(ivalues, E); return detail::unflatten(o, mOY, mOX, E); }
    vec2 simple_gradient(const vec2& ivalues, float elev_gradient) const {
        need_grid(true);
        return detail::unflatten(level(1, ivalues, nullptr, nullptr, elev_gradient), mOY, mOX);
    }
    vec3 simple_gradient(const vec3& ivalues, float elev_gradient) const {
        need_grid(true);
        size_t T;
        vec o = levels(1, ivalues, nullptr, nullptr, elev_gradient, T);
        return detail::unflatten(o, T, mOY, mOX);
    }
    vec2 full_gradient(const vec2& ivalues, const vec2& elev_gradient, const vec2& laf_gradient = vec2()) const {
        need_grid(true);
        if(ivalues.size() != mY || (ivalues.size() ? ivalues[0].size() : 0) != mX) throw std::invalid_argument("Values is the wrong size");   // gradient.cpp:10-11
        return detail::unflatten(level(2, ivalues, &elev_gradient, &laf_gradient, 0), mOY, mOX);
    }
    vec3 full_gradient(const vec3& ivalues, const vec3& elev_gradient, const vec3& laf_gradient) const {
        need_grid(true);
        size_t T;
        vec o = levels(2, ivalues, &elev_gradient, &laf_gradient, 0, T);
        return detail::unflatten(o, T, mOY, mOX);
    }
    // ---- a Points output ----
    vec apply_points(const vec2& ivalues) const { need_grid(false); return level(0, ivalues, nullptr, nullptr, 0); }
    vec2 apply_points(const vec3& ivalues) const { need_grid(false); size_t T; vec o = levels(0, ivalues, nullptr, nullptr, 0, T); return detail::unflatten(o, T, mOY); }
    vec2 apply_cube_points(const vec3& ivalues) const { need_grid(false); size_t E; vec o = cube(ivalues, E); return detail::unflatten(o, mOY, E); }
    vec simple_gradient_points(const vec2& ivalues, float elev_gradient) const { need_grid(false); return level(1, ivalues, nullptr, nullptr, elev_gradient); }
    vec2 simple_gradient_points(const vec3& ivalues, float elev_gradient) const {
        need_grid(false);
        size_t T;
        vec o = levels(1, ivalues, nullptr, nullptr, elev_gradient, T);
        return detail::unflatten(o, T, mOY);
    }
    vec full_gradient_points(const vec2& ivalues, const vec2& elev_gradient, const vec2& laf_gradient) const {
        need_grid(false);
        return level(2, ivalues, &elev_gradient, &laf_gradient, 0);
    }
    vec2 full_gradient_points(const vec3& ivalues, const vec3& elev_gradient, const vec3& laf_gradient) const {
        need_grid(false);
        size_t T;
        vec o = levels(2, ivalues, &elev_gradient, &laf_gradient, 0, T);
        return detail::unflatten(o, T, mOY);
    }

    Downscaler downscaler() const { int d = 0; detail::check(gpp_downscale_plan_info(mP, nullptr, nullptr, &d, nullptr, nullptr)); return (Downscaler)d; }
    long long nbytes() const { long long b = 0; detail::check(gpp_downscale_plan_info(mP, nullptr, nullptr, nullptr, &b, nullptr)); return b; }   // HBM held now
    long long distorted() const { long long d = 0; detail::check(gpp_downscale_plan_info(mP, nullptr, nullptr, nullptr, nullptr, &d)); return d; }

  private:
    void create(const Grid& igrid, gpp_points* to, CoordinateType otype, Downscaler downscaler) {
        detail::check_downscaler(downscaler);
        if(downscaler == Nearest && igrid.get_coordinate_type() != otype) throw std::invalid_argument("Coordinate types must be the same");
        detail::check(gpp_downscale_plan_create(igrid.handle(), to, (int)downscaler, &mP));
    }
    void release() {
        if(mP) gpp_downscale_plan_destroy(mP);
        mP = nullptr;
    }
    void need_grid(bool grid) const {
        if(grid != mGrid) throw std::invalid_argument(mGrid ? "this plan was built for a Grid output" : "this plan was built for a Points output");
    }
    size_t locations() const { return mOY * mOX; }
    // which: 0 apply, 1 simple_gradient, 2 full_gradient; v [T][Y * X]; empty: the values passed the size rule without holding a field
    vec run(int which, const vec& v, size_t T, bool empty, const vec* eg, const vec* lg, float elev_gradient) const {
        vec out(T * locations(), MV);
        if(out.empty()) return out;
        if(mY && mX && empty) throw std::invalid_argument(detail::GRID_MISMATCH);
        if(which == 0) detail::check(gpp_downscale_plan_apply(mP, v.data(), (int)T, out.data(), GPP_MEM_HOST));
        else if(which == 1) detail::check(gpp_downscale_plan_simple_gradient(mP, v.data(), (int)T, elev_gradient, out.data(), GPP_MEM_HOST));
        else detail::check(gpp_downscale_plan_full_gradient(mP, v.data(), (int)T, eg ? eg->data() : nullptr, lg ? lg->data() : nullptr, out.data(), GPP_MEM_HOST));
        return out;
    }
    vec level(int which, const vec2& ivalues, const vec2* egrad, const vec2* lgrad, float elev_gradient) const {
        if(ivalues.size() != 0 && (ivalues.size() != mY || ivalues[0].size() != mX)) throw std::invalid_argument(detail::GRID_MISMATCH);   // util.cpp:427-429
        size_t Y, X;
        vec v = detail::flatten(ivalues, Y, X), lf, ef;
        const vec* lg = lgrad ? detail::gradient_field(*lgrad, lf, Y, X, detail::LAF_MISMATCH) : nullptr;
        const vec* eg = egrad ? detail::gradient_field(*egrad, ef, Y, X, detail::ELEV_MISMATCH) : nullptr;
        return run(which, v, 1, Y == 0, eg, lg, elev_gradient);
    }
    vec levels(int which, const vec3& ivalues, const vec3* egrad, const vec3* lgrad, float elev_gradient, size_t& T) const {
        if(ivalues.size() != 0 && ivalues[0].size() != 0 && (ivalues[0].size() != mY || ivalues[0][0].size() != mX))   // util.cpp:430-432
            throw std::invalid_argument(detail::GRID_MISMATCH);
        size_t Y, X;
        vec v = detail::flatten(ivalues, T, Y, X), lf, ef;
        const vec* lg = lgrad ? detail::gradient_field(*lgrad, lf, T, Y, X, detail::LAF_MISMATCH) : nullptr;
        const vec* eg = egrad ? detail::gradient_field(*egrad, ef, T, Y, X, detail::ELEV_MISMATCH) : nullptr;
        return run(which, v, T, T == 0 || Y == 0, eg, lg, elev_gradient);
    }
    vec cube(const vec3& ivalues, size_t& E) const {
        size_t Y, X;
        vec v = detail::flatten(ivalues, Y, X, E);
        if(Y != mY || (Y && X != mX)) throw std::invalid_argument(detail::GRID_MISMATCH);
        vec out(locations() * E, MV);
        if(!out.empty()) detail::check(gpp_downscale_plan_apply_cube(mP, v.data(), (int)E, out.data(), GPP_MEM_HOST));
        return out;
    }
    bool mGrid;
    size_t mY, mX, mOY, mOX;
    gpp_downscale_plan* mP = nullptr;
};
}   // namespace gridpp
