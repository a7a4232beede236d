// gridpp::OiGain -- the reusable gain of optimal interpolation (include/gridpp_hip.h: gpp_oi_gain_*).  No counterpart in
// the reference's gridpp.h, hence a header of its own beside gridpp.hpp (which it includes): everything of optimal_interpolation that
// depends on no value -- which observations every background point selects and their weights -- is computed once by the constructor,
// and apply() analyses a field, or a stack of fields in gridpp's cube layout (the field index innermost), with it.
//
//     gridpp::OiGain gain(grid, points, pratios, structure, 30);
//     vec2 out = gain.apply(background, pobs, pbackground);        // = optimal_interpolation(grid, background, points, pobs, pratios, pbackground, structure, 30)
//     vec3 outs = gain.apply(background_yxe, pobs, pbackground_se);   // E fields in one call
//
// pratios is optimal_interpolation's (a caller of optimal_interpolation_full passes obs_variance / bvariance_at_points, divided in
// float32).  usable (empty: every station) names the stations to leave out at construction -- the reference drops a station with a
// missing value per call; apply() throws std::invalid_argument when a usable station has one.  1 <= max_points <= max_points_cap.
// The gain holds about cells * max_points * 12 bytes of HBM (nbytes()) until it is destroyed; the Grid, Points and structure it was
// built from may be destroyed first.
#pragma once
#include "gridpp.hpp"

namespace gridpp {
class OiGain {
  public:
    static const int max_points_cap = GPP_OI_GAIN_MAX_POINTS;
    OiGain(const Grid& bgrid, const Points& points, const vec& pratios, const StructureFunction& structure, int max_points, const ivec& usable = ivec())
        : mGrid(true), mY(bgrid.size()[0]), mX(bgrid.size()[1]) {
        if(bgrid.get_coordinate_type() != points.get_coordinate_type())
            throw std::invalid_argument("Both background and observations points must be of same coordinate type (lat/lon or x/y)");
        create(bgrid.handle(), points, pratios, structure, max_points, usable);
    }
    OiGain(const Points& bpoints, const Points& points, const vec& pratios, const StructureFunction& structure, int max_points, const ivec& usable = ivec())
        : mGrid(false), mY(bpoints.size()), mX(1) {
        if(bpoints.get_coordinate_type() != points.get_coordinate_type())
            throw std::invalid_argument("Both background and observations points must be of same coordinate type (lat/lon or x/y)");
        create(bpoints.handle(), points, pratios, structure, max_points, usable);
    }
    // a Grid background: one field, or (Y, X, E) with pbackground (S, E)
    vec2 apply(const vec2& background, const vec& pobs, const vec& pbackground, bool allow_extrapolation = true) const {
        need_grid(true);
        size_t Y, X;
        const vec bg = detail::flatten(background, Y, X);
        if(Y != mY || X != mX) throw std::invalid_argument("input field is not the same size as the grid");
        return detail::unflatten(run(bg, 1, pobs, false, pbackground, allow_extrapolation), Y, X);
    }
    vec3 apply(const vec3& background, const vec& pobs, const vec2& pbackground, bool allow_extrapolation = true) const {
        need_grid(true);
        size_t Y, X, E, S, E2;
        const vec bg = detail::flatten(background, Y, X, E);
        const vec pbg = detail::flatten(pbackground, S, E2);
        if(Y != mY || X != mX) throw std::invalid_argument("input field is not the same size as the grid");
        if(E2 != E) throw std::invalid_argument("Fields in the gridded background is not the same as in the point background");
        return detail::unflatten(run(bg, E, pobs, false, pbg, allow_extrapolation), Y, X, E);
    }
    // a Points background: one field, or (N, E) with pbackground (S, E)
    vec apply(const vec& background, const vec& pobs, const vec& pbackground, bool allow_extrapolation = true) const {
        need_grid(false);
        if(background.size() != mY) throw std::invalid_argument("Input field is not the same size as the grid");
        return run(background, 1, pobs, false, pbackground, allow_extrapolation);
    }
    vec2 apply(const vec2& background, const vec& pobs, const vec2& pbackground, bool allow_extrapolation = true) const {
        need_grid(false);
        size_t N, E, S, E2;
        const vec bg = detail::flatten(background, N, E);
        const vec pbg = detail::flatten(pbackground, S, E2);
        if(N != mY) throw std::invalid_argument("Input field is not the same size as the grid");
        if(E2 != E) throw std::invalid_argument("Fields in the background is not the same as in the point background");
        return detail::unflatten(run(bg, E, pobs, false, pbg, allow_extrapolation), N, E);
    }
    // the analysis variance of optimal_interpolation_full: bvariance (1 - w . g) where the point has a selection
    vec2 analysis_variance(const vec2& bvariance) const {
        need_grid(true);
        size_t Y, X;
        const vec bv = detail::flatten(bvariance, Y, X);
        if(Y != mY || X != mX) throw std::invalid_argument("Input bvariance is not the same size as the grid");
        return detail::unflatten(variance(bv), Y, X);
    }
    vec analysis_variance(const vec& bvariance) const {
        need_grid(false);
        if(bvariance.size() != mY) throw std::invalid_argument("Input bvariance is not the same size as the grid");
        return variance(bvariance);
    }
    // per background point (flat, row-major for a Grid): the number of selected observations, their indices into the observation arrays
    // (ascending, -1 behind the selection) and their weights (0 behind the selection), max_points() columns each
    ivec counts() const {
        ivec c(mY * mX);
        if(!c.empty()) detail::check(gpp_oi_gain_selection(mH->g, c.data(), nullptr, nullptr, GPP_MEM_HOST));
        return c;
    }
    ivec2 indices() const {
        std::vector<int> f(mY * mX * (size_t)mK);
        if(!f.empty()) detail::check(gpp_oi_gain_selection(mH->g, nullptr, f.data(), nullptr, GPP_MEM_HOST));
        ivec2 o(mY * mX);
        for(size_t i = 0; i < o.size(); i++) o[i].assign(f.begin() + i * mK, f.begin() + (i + 1) * mK);
        return o;
    }
    std::vector<std::vector<double> > weights() const {
        std::vector<double> f(mY * mX * (size_t)mK);
        if(!f.empty()) detail::check(gpp_oi_gain_selection(mH->g, nullptr, nullptr, f.data(), GPP_MEM_HOST));
        std::vector<std::vector<double> > o(mY * mX);
        for(size_t i = 0; i < o.size(); i++) o[i].assign(f.begin() + i * mK, f.begin() + (i + 1) * mK);
        return o;
    }
    int max_points() const { return mK; }
    long long nbytes() const {   // HBM held now; returned when the last copy of the gain is destroyed
        long long b = 0;
        detail::check(gpp_oi_gain_info(mH->g, nullptr, nullptr, nullptr, &b, nullptr));
        return b;
    }
    int largest_selection() const {
        int l = 0;
        detail::check(gpp_oi_gain_info(mH->g, nullptr, nullptr, nullptr, nullptr, &l));
        return l;
    }

  private:
    struct Handle {
        gpp_oi_gain* g = nullptr;
        ~Handle() { if(g) gpp_oi_gain_destroy(g); }
    };
    void create(gpp_points* bg, const Points& points, const vec& pratios, const StructureFunction& structure, int max_points, const ivec& usable) {
        if(max_points < 1) throw std::invalid_argument("max_points must be >= 1: a gain holds max_points columns per background point");
        if(max_points > max_points_cap) throw std::invalid_argument("max_points must be <= " + std::to_string(max_points_cap) + " (GPP_OI_GAIN_MAX_POINTS)");
        if((int)pratios.size() != points.size()) throw std::invalid_argument("Ratios and points size mismatch");
        if(!usable.empty() && (int)usable.size() != points.size()) throw std::invalid_argument("usable and points size mismatch");
        std::vector<unsigned char> u(usable.size());
        for(size_t i = 0; i < u.size(); i++) u[i] = usable[i] ? 1 : 0;
        mS = (size_t)points.size();
        mK = max_points;
        mH = std::make_shared<Handle>();
        detail::check(gpp_oi_gain_create(bg, points.handle(), pratios.data(), usable.empty() ? nullptr : u.data(), structure.c_struct(), max_points, &mH->g));
    }
    void need_grid(bool grid) const {
        if(grid != mGrid) throw std::invalid_argument(mGrid ? "this gain was built for a Grid background" : "this gain was built for a Points background");
    }
    vec run(const vec& bg, size_t E, const vec& pobs, bool per_field, const vec& pbg, bool allow_extrapolation) const {
        if(E < 1) throw std::invalid_argument("background holds no fields");
        if(pobs.size() != mS) throw std::invalid_argument("Observations and points size mismatch");
        if(pbg.size() != mS * E) throw std::invalid_argument("Background and points size mismatch");
        vec out(bg.size());
        if(!bg.empty())
            detail::check(gpp_oi_gain_apply(mH->g, bg.data(), (int)E, pobs.data(), per_field ? 1 : 0, pbg.data(), allow_extrapolation ? 1 : 0, out.data(), GPP_MEM_HOST));
        return out;
    }
    vec variance(const vec& bv) const {
        vec out(bv.size());
        if(!bv.empty()) detail::check(gpp_oi_gain_variance(mH->g, bv.data(), out.data(), GPP_MEM_HOST));
        return out;
    }
    bool mGrid;
    size_t mY, mX, mS = 0;
    int mK = 0;
    std::shared_ptr<Handle> mH;
};
}   // namespace gridpp
