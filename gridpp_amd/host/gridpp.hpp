// gridpp.hpp -- C++ host mirror of the reference's public API (include/gridpp.h) for the hot path only,
// header-only over the C-ABI of libgridpp_hip.so (include/gridpp_hip.h).
//
// Same namespace, type names, signatures, defaults and exception types as the reference, so code written
// against gridpp.h for this path compiles unchanged:
//   vec/vec2/vec3/ivec                         include/gridpp.h:25-41
//   Statistic, CoordinateType, MV              :49,88-100,120-123
//   Points, Grid, KDTree (queries)             :1746-2060
//   BarnesStructure (scalar form)              :2160-2185
//   optimal_interpolation(_full)(_ensi)        :162-294
//   neighbourhood*, get_neighbourhood_thresholds :588-716
//   nearest (all eight overloads)              :860-900
//   bilinear(Grid, Grid|Points, vec2|vec3)     :902-930
//   Downscaler, downscaling, simple_gradient, full_gradient (all four overloads each)  :132-135,844-871,1017-1098
//   ComparisonOperator, downscale_probability, mask_threshold_downscale_consensus / _quantile, smart  :138-143,945-990,1112
//   Extrapolation, apply_curve (all four overloads), interpolate, quantile_mapping_curve, monotonize_curve  :79-85,731-789,1549-1557
//   count, gridding, gridding_nearest          :938-1010
//   fill, fill_missing, doping_square/circle, neighbourhood_search, calc_gradient
//   calc_statistic / calc_quantile             :1454-1482
//   Metric, calc_score (three overloads), neighbourhood_score  :103-110
//   MV_CML, pi and the constants of the standard atmosphere    :51-67
//   dewpoint, relative_humidity, wetbulb, pressure, sea_level_pressure, qnh, wind_speed, wind_direction (scalar and vector)  :1249-1367
//   Transform, Identity, Log, BoxCox, StartedBoxCox            :2345-2435
// Nested vectors are flattened once, handed to the C-ABI as host buffers (GPP_MEM_HOST) and un-flattened,
// exactly where the reference flattens them itself (src/api/oi.cpp:69-86).  Errors: GPP_EINVAL ->
// std::invalid_argument, everything else -> std::runtime_error (swig/gridpp.i:21-40 maps these to python).
#pragma once
#include <algorithm>
#include <cmath>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <initializer_list>
#include <iostream>
#include <string>
#include <vector>
#include "../../include/gridpp_hip.h"

namespace gridpp {
typedef std::vector<float> vec;
typedef std::vector<vec> vec2;
typedef std::vector<vec2> vec3;
typedef std::vector<int> ivec;
typedef std::vector<ivec> ivec2;
static const float MV = NAN;
static const double radius_earth = 6.378137e6;
// include/gridpp.h:51-67
static const float MV_CML = -999;
static const float pi = 3.14159265;
static const float lapse_rate = 0.0065;
static const float standard_surface_temperature = 288.15;
static const float gravit = 9.80665;
static const float molar_mass = 0.0289644;
static const float gas_constant_mol = 8.31447;
static const float gas_constant_si = 287.05;

enum Statistic { Mean = 0, Min = 10, Median = 20, Max = 30, Quantile = 40, Std = 50, Variance = 60, Sum = 70, Count = 80, RandomChoice = 90, Unknown = -1 };
enum CoordinateType { Geodetic = 0, Cartesian = 1 };
enum Downscaler { Nearest = 0, Bilinear = 1 };   // include/gridpp.h:132-135
enum ComparisonOperator { Lt = 0, Leq = 10, Gt = 20, Geq = 30 };   // include/gridpp.h:138-143
enum Extrapolation { OneToOne = 0, MeanSlope = 10, NearestSlope = 20, Zero = 30, Unchanged = 40 };   // include/gridpp.h:79-85
enum Metric { Ets = 0, Ts = 1, Kss = 20, Pc = 30, Bias = 40, Hss = 50 };   // include/gridpp.h:103-110

namespace detail {
inline void check(int rc) {
    if(rc == GPP_OK) return;
    std::string msg = gpp_last_error();
    if(rc == GPP_EINVAL) throw std::invalid_argument(msg);
    throw std::runtime_error(msg);
}
inline vec flatten(const vec2& a, size_t& Y, size_t& X) {
    Y = a.size(); X = Y ? a[0].size() : 0;
    vec f; f.reserve(Y * X);
    for(const auto& r : a) { if(r.size() != X) throw std::invalid_argument("ragged 2-D array"); f.insert(f.end(), r.begin(), r.end()); }
    return f;
}
inline vec flatten(const vec3& a, size_t& Y, size_t& X, size_t& E) {
    Y = a.size(); X = Y ? a[0].size() : 0; E = (Y && X) ? a[0][0].size() : 0;
    vec f; f.reserve(Y * X * E);
    for(const auto& r : a) { if(r.size() != X) throw std::invalid_argument("ragged 3-D array");
        for(const auto& c : r) { if(c.size() != E) throw std::invalid_argument("ragged 3-D array"); f.insert(f.end(), c.begin(), c.end()); } }
    return f;
}
inline vec2 unflatten(const vec& f, size_t Y, size_t X) {
    vec2 o(Y);
    for(size_t y = 0; y < Y; y++) o[y].assign(f.begin() + y * X, f.begin() + (y + 1) * X);
    return o;
}
inline vec3 unflatten(const vec& f, size_t Y, size_t X, size_t E) {
    vec3 o(Y);
    for(size_t y = 0; y < Y; y++) { o[y].resize(X); for(size_t x = 0; x < X; x++) o[y][x].assign(f.begin() + (y * X + x) * E, f.begin() + (y * X + x + 1) * E); }
    return o;
}
struct Handle {
    gpp_points* p = nullptr;
    ~Handle() { if(p) gpp_points_destroy(p); }
};
}   // namespace detail

inline bool is_valid(float value) { return !std::isnan(value) && !std::isinf(value); }   // src/api/util.cpp:16-18
inline std::string version() { return gpp_version(); }
// include/gridpp.h:1410, src/api/gridpp.cpp:11-43 (the reference's table has no "variance": Unknown, like every other name it does not know)
inline Statistic get_statistic(const std::string& name) {
    static const struct { const char* n; Statistic s; } table[] = {{"mean", Mean}, {"min", Min}, {"max", Max}, {"median", Median}, {"quantile", Quantile},
                                                                   {"std", Std}, {"sum", Sum}, {"count", Count}, {"randomchoice", RandomChoice}};
    for(const auto& e : table) if(name == e.n) return e.s;
    return Unknown;
}
inline void set_omp_threads(int) {}        // src/api/gridpp.cpp:184-207: no meaning on the GPU path
inline int get_omp_threads() { return 1; }
// messages (include/gridpp.h:1394-1430, src/api/gridpp.cpp:70-76, src/api/util.cpp:226-252)
inline int& debug_level_ref() { static int level = 0; return level; }
inline void set_debug_level(int level) { debug_level_ref() = level; }
inline int get_debug_level() { return debug_level_ref(); }
inline void debug(const std::string& s) { std::cout << s << std::endl; }
inline void warning(const std::string& s) { std::cout << "Warning: " << s << std::endl; }
inline void error(const std::string& s) { std::cout << "Error: " << s << std::endl; throw std::runtime_error(s); }
inline void future_deprecation_warning(const std::string& function, const std::string& other = "") {
    std::cout << "Future deprecation warning: " << function << " will be deprecated";
    if(other != "") std::cout << ", use " << other << " instead." << std::endl;
    else std::cout << "." << std::endl;
}

class Points {
  public:
    Points() : Points(vec(), vec()) {}
    Points(vec lats, vec lons, vec elevs = vec(), vec lafs = vec(), CoordinateType type = Geodetic) : mType(type) {
        size_t N = lats.size();
        if(lons.size() != N) throw std::invalid_argument("Cannot create points with unequal lat and lon sizes");
        if(elevs.size() != 0 && elevs.size() != N) throw std::invalid_argument("'elevs' must either be size 0 or the same size at lats/lons");
        if(lafs.size() != 0 && lafs.size() != N) throw std::invalid_argument("'lafs' must either be size 0 or the same size at lats/lons");
        mH = std::make_shared<detail::Handle>();
        detail::check(gpp_points_create(lats.data(), lons.data(), elevs.size() == N && N ? elevs.data() : nullptr,
                                        lafs.size() == N && N ? lafs.data() : nullptr, (int)N, (int)type, &mH->p));
        mN = (int)N;
    }
    int size() const { return mN; }
    CoordinateType get_coordinate_type() const { return mType; }
    vec get_lats() const { return field(0); }
    vec get_lons() const { return field(1); }
    vec get_elevs() const { return field(2); }
    vec get_lafs() const { return field(3); }
    ivec get_neighbours(float lat, float lon, float radius, bool include_match = true) const {
        ivec idx(mN > 0 ? mN : 1); int count = 0;
        detail::check(gpp_points_get_neighbours(mH->p, lat, lon, radius, include_match, idx.data(), nullptr, (int)idx.size(), &count));
        idx.resize(count);
        return idx;
    }
    int get_num_neighbours(float lat, float lon, float radius, bool include_match = true) const { return (int)get_neighbours(lat, lon, radius, include_match).size(); }
    int get_nearest_neighbour(float lat, float lon, bool include_match = true) const {
        int i = -1;
        detail::check(gpp_points_nearest_neighbour(mH->p, &lat, &lon, 1, include_match, &i));
        return i;
    }
    gpp_points* handle() const { return mH->p; }
  protected:
    vec field(int k) const { vec o(mN); detail::check(gpp_points_get(mH->p, k, o.data())); return o; }
    std::shared_ptr<detail::Handle> mH;
    int mN = 0;
    CoordinateType mType = Geodetic;
};
typedef Points KDTree;

class Grid {
  public:
    Grid() : Grid(vec2(), vec2()) {}
    Grid(vec2 lats, vec2 lons, vec2 elevs = vec2(), vec2 lafs = vec2(), CoordinateType type = Geodetic) : mType(type) {
        size_t Y, X, Y2, X2;
        vec la = detail::flatten(lats, Y, X), lo = detail::flatten(lons, Y2, X2);
        if(Y != Y2 || X != X2) throw std::invalid_argument("lats and lons must have the same shape");
        size_t Ye, Xe, Yl, Xl;
        vec el = detail::flatten(elevs, Ye, Xe), lf = detail::flatten(lafs, Yl, Xl);
        if(Y * X == 0) Y = X = 0;
        mH = std::make_shared<detail::Handle>();
        detail::check(gpp_grid_create(la.data(), lo.data(), (Ye == Y && Xe == X && Y * X) ? el.data() : nullptr,   // grid.cpp:41-54
                                      (Yl == Y && Xl == X && Y * X) ? lf.data() : nullptr, (int)Y, (int)X, (int)type, &mH->p));
        mY = (int)Y; mX = (int)X;
    }
    ivec size() const { return ivec{mY, mX}; }
    CoordinateType get_coordinate_type() const { return mType; }
    ivec get_nearest_neighbour(float lat, float lon, bool include_match = true) const {   // grid.cpp:76-82,108-114
        if(mY * mX == 0) return ivec();
        int i = -1;
        detail::check(gpp_points_nearest_neighbour(mH->p, &lat, &lon, 1, include_match, &i));
        return ivec{i / mX, i % mX};
    }
    bool get_box(float lat, float lon, int& Y1_out, int& X1_out, int& Y2_out, int& X2_out) const {   // grid.cpp:149-229
        int inside = 0, box[4] = {-1, -1, -1, -1};
        detail::check(gpp_grid_get_box(mH->p, &lat, &lon, 1, &inside, box));
        Y1_out = box[0]; X1_out = box[1]; Y2_out = box[2]; X2_out = box[3];
        return inside != 0;
    }
    gpp_points* handle() const { return mH->p; }
  private:
    std::shared_ptr<detail::Handle> mH;
    int mY = 0, mX = 0;
    CoordinateType mType = Geodetic;
};

// ---- structure functions (include/gridpp.h:2069-2343), scalar forms -------------------------------------------
class StructureFunction {
  public:
    virtual ~StructureFunction() {}
    const gpp_structure* c_struct() const { return &mS; }
    float localization_distance() const { float d; detail::check(gpp_structure_localization_distance(&mS, 0.0f, 0.0f, &d)); return d; }
  protected:
    StructureFunction() { mS = gpp_structure(); }
    void init(int kind, float h, float v, float w, float hmax) {
        if(!is_valid(v) || v < 0) throw std::invalid_argument("v must be >= 0");
        if(!is_valid(w) || w < 0) throw std::invalid_argument("w must be >= 0");
        mS = gpp_structure();
        mS.kind = kind; mS.h = h; mS.v = v; mS.w = w;
        detail::check(gpp_structure_min_rho(kind, h, hmax, &mS.min_rho));
    }
    gpp_structure mS;
};
class BarnesStructure : public StructureFunction { public: BarnesStructure(float h, float v = 0, float w = 0, float hmax = MV) { init(GPP_SK_BARNES, h, v, w, hmax); } };
class CressmanStructure : public StructureFunction { public: CressmanStructure(float h, float v = 0, float w = 0) { init(GPP_SK_CRESSMAN, h, v, w, MV); } };
class SoarStructure : public StructureFunction { public: SoarStructure(float h, float v = 0, float w = 0, float hmax = MV) { init(GPP_SK_SOAR, h, v, w, hmax); } };
class ToarStructure : public StructureFunction { public: ToarStructure(float h, float v = 0, float w = 0, float hmax = MV) { init(GPP_SK_TOAR, h, v, w, hmax); } };
class PowerlawStructure : public StructureFunction { public: PowerlawStructure(float h, float v = 0, float w = 0, float hmax = MV) { init(GPP_SK_POWERLAW, h, v, w, hmax); } };
class LinearStructure : public StructureFunction { public: LinearStructure(float h, float v = 0, float w = 0, float hmax = MV) { init(GPP_SK_LINEAR, h, v, w, hmax); } };
class MultipleStructure : public StructureFunction {   // src/api/structure.cpp:90-138
  public:
    MultipleStructure(const StructureFunction& sh, const StructureFunction& sv, const StructureFunction& sw) {
        const gpp_structure *h = sh.c_struct(), *v = sv.c_struct(), *w = sw.c_struct();
        mS = *h;
        mS.v = v->v; mS.w = w->w;
        mS.kind_v = (v->kind_v ? v->kind_v - 1 : v->kind) + 1;
        mS.kind_w = (w->kind_w ? w->kind_w - 1 : w->kind) + 1;
        mS.loc = sh.localization_distance();
        mS.flags = GPP_ST_HAS_LOC;
        mS.cv_dist = 0;
        // (a nested MultipleStructure contributes the field of its own vertical / laf component)
        mS.field = h->field; mS.field_v = v->kind_v ? v->field_v : v->field; mS.field_w = w->kind_w ? w->field_w : w->field;
    }
};
class CrossValidation : public StructureFunction {     // src/api/structure.cpp:910-944
  public:
    CrossValidation(const StructureFunction& structure, float dist) {
        if(!is_valid(dist) || dist < 0) throw std::invalid_argument("Invalid 'dist' in CrossValidation structure");
        mS = *structure.c_struct();
        mS.flags |= GPP_ST_CV;
        mS.cv_dist = dist;
    }
};

// ---- optimal interpolation (include/gridpp.h:162-248) -------------------------------------------------
inline vec optimal_interpolation_full(const Points& bpoints, const vec& background, const vec& bvariance, const Points& points,
                                      const vec& obs, const vec& obs_variance, const vec& background_at_points,
                                      const vec& bvariance_at_points, const StructureFunction& structure, int max_points,
                                      vec& analysis_variance, bool allow_extrapolation = true) {
    if(max_points < 0) throw std::invalid_argument("max_points must be >= 0");
    if(bpoints.get_coordinate_type() != points.get_coordinate_type())
        throw std::invalid_argument("Both background points and observations points must be of same coordinate type (lat/lon or x/y)");
    if((int)background.size() != bpoints.size()) throw std::invalid_argument("Input field is not the same size as the grid");
    if(background.size() != bvariance.size()) throw std::invalid_argument("Input bvariance is not the same size as the grid");
    if((int)obs.size() != points.size()) throw std::invalid_argument("Observations and points size mismatch");
    if((int)obs_variance.size() != points.size()) throw std::invalid_argument("Obs variance and points size mismatch");
    if((int)background_at_points.size() != points.size()) throw std::invalid_argument("Background and points size mismatch");
    if((int)bvariance_at_points.size() != points.size()) throw std::invalid_argument("Background variance and points size mismatch");
    if(points.size() == 0) return background;   // oi.cpp:189-190 (analysis_variance left untouched)
    vec out(background.size());
    analysis_variance.assign(background.size(), 0);
    detail::check(gpp_optimal_interpolation_full(bpoints.handle(), background.data(), bvariance.data(), points.handle(), obs.data(),
                                                 obs_variance.data(), background_at_points.data(), bvariance_at_points.data(),
                                                 structure.c_struct(), max_points, allow_extrapolation, out.data(),
                                                 analysis_variance.data(), GPP_MEM_HOST));
    return out;
}
inline vec optimal_interpolation(const Points& bpoints, const vec& background, const Points& points, const vec& pobs, const vec& pratios,
                                 const vec& pbackground, const StructureFunction& structure, int max_points, bool allow_extrapolation = true) {
    if(max_points < 0) throw std::invalid_argument("max_points must be >= 0");
    if(bpoints.get_coordinate_type() != points.get_coordinate_type())
        throw std::invalid_argument("Both background points and observations points must be of same coordinate type (lat/lon or x/y)");
    if((int)background.size() != bpoints.size()) throw std::invalid_argument("Input field is not the same size as the grid");
    if((int)pobs.size() != points.size()) throw std::invalid_argument("Observations and points size mismatch");
    if((int)pratios.size() != points.size()) throw std::invalid_argument("Ratios and points size mismatch");
    if((int)pbackground.size() != points.size()) throw std::invalid_argument("Background and points size mismatch");
    vec out(background.size());
    if(background.empty()) return out;
    detail::check(gpp_optimal_interpolation_full(bpoints.handle(), background.data(), nullptr, points.handle(), pobs.data(), pratios.data(),
                                                 pbackground.data(), nullptr, structure.c_struct(), max_points, allow_extrapolation,
                                                 out.data(), nullptr, GPP_MEM_HOST));
    return out;
}
namespace detail {
inline void check_grid_field(const Grid& g, size_t Y, size_t X) {
    if((int)Y != g.size()[0] || (int)X != g.size()[1]) throw std::invalid_argument("input field is not the same size as the grid");
}
}
inline vec2 optimal_interpolation(const Grid& bgrid, const vec2& background, const Points& points, const vec& pobs, const vec& pratios,
                                  const vec& pbackground, const StructureFunction& structure, int max_points, bool allow_extrapolation = true) {
    if(max_points < 0) throw std::invalid_argument("max_points must be >= 0");
    if(bgrid.get_coordinate_type() != points.get_coordinate_type())
        throw std::invalid_argument("Both background grid and observations points must be of same coordinate type (lat/lon or x/y)");
    size_t Y, X;
    vec bg = detail::flatten(background, Y, X);
    detail::check_grid_field(bgrid, Y, X);
    if((int)pobs.size() != points.size() || (int)pratios.size() != points.size() || (int)pbackground.size() != points.size())
        throw std::invalid_argument("Observations / ratios / background and points size mismatch");
    vec out(bg.size());
    if(!bg.empty())
        detail::check(gpp_optimal_interpolation_full(bgrid.handle(), bg.data(), nullptr, points.handle(), pobs.data(), pratios.data(),
                                                     pbackground.data(), nullptr, structure.c_struct(), max_points, allow_extrapolation,
                                                     out.data(), nullptr, GPP_MEM_HOST));
    return detail::unflatten(out, Y, X);
}
inline vec2 optimal_interpolation_full(const Grid& bgrid, const vec2& background, const vec2& bvariance, const Points& points, const vec& obs,
                                       const vec& obs_variance, const vec& background_at_points, const vec& bvariance_at_points,
                                       const StructureFunction& structure, int max_points, vec2& analysis_variance, bool allow_extrapolation = true) {
    if(max_points < 0) throw std::invalid_argument("max_points must be >= 0");
    if(bgrid.get_coordinate_type() != points.get_coordinate_type())
        throw std::invalid_argument("Both background grid and observations points must be of same coordinate type (lat/lon or x/y)");
    size_t Y, X, Yv, Xv;
    vec bg = detail::flatten(background, Y, X), bv = detail::flatten(bvariance, Yv, Xv);
    detail::check_grid_field(bgrid, Y, X);
    if(Y != Yv || X != Xv) throw std::invalid_argument("Input bvariance is not the same size as the grid");
    if((int)obs.size() != points.size() || (int)obs_variance.size() != points.size() || (int)background_at_points.size() != points.size() ||
       (int)bvariance_at_points.size() != points.size())
        throw std::invalid_argument("Observation arrays and points size mismatch");
    if(points.size() == 0) { analysis_variance = bvariance; return background; }
    vec out(bg.size()), var(bg.size());
    detail::check(gpp_optimal_interpolation_full(bgrid.handle(), bg.data(), bv.data(), points.handle(), obs.data(), obs_variance.data(),
                                                 background_at_points.data(), bvariance_at_points.data(), structure.c_struct(), max_points,
                                                 allow_extrapolation, out.data(), var.data(), GPP_MEM_HOST));
    analysis_variance = detail::unflatten(var, Y, X);
    return detail::unflatten(out, Y, X);
}
// include/gridpp.h:263-294
namespace detail {
// the two warnings the reference prints at the end of optimal_interpolation_ensi (src/api/oi_ensi.cpp:557-566)
inline void ensi_warnings() {
    gpp_ensi_stats st;
    if(gpp_ensi_last_stats(&st) != GPP_OK) return;
    if(st.condition_passthrough > 0) warning("Condition number error in " + std::to_string(st.condition_passthrough) + " points. Using raw values in those points.");
    if(st.real_part_passthrough > 0) warning("Could not find the real part of W in " + std::to_string(st.real_part_passthrough) + " points. Using raw values in those points.");
}
}
inline vec2 optimal_interpolation_ensi(const Points& bpoints, const vec2& background, const Points& points, const vec& pobs, const vec& psigmas,
                                       const vec2& pbackground, const StructureFunction& structure, int max_points, bool allow_extrapolation = true) {
    if(max_points < 0) throw std::invalid_argument("max_points must be >= 0");
    if(points.size() == 0) return background;
    if(bpoints.get_coordinate_type() != points.get_coordinate_type())
        throw std::invalid_argument("Both background and observations points must be of same coorindate type (lat/lon or x/y)");
    size_t N, E, S, E2;
    vec bg = detail::flatten(background, N, E), pbg = detail::flatten(pbackground, S, E2);
    if((int)N != bpoints.size()) throw std::invalid_argument("Input field is not the same size as the grid");
    if((int)pobs.size() != points.size() || (int)psigmas.size() != points.size() || (int)S != points.size())
        throw std::invalid_argument("Observations / sigmas / background and points size mismatch");
    if(E != E2) throw std::invalid_argument("Ensemble size mismatch");
    vec out(bg.size());
    detail::check(gpp_optimal_interpolation_ensi(bpoints.handle(), bg.data(), (int)E, points.handle(), pobs.data(), psigmas.data(), pbg.data(),
                                                 structure.c_struct(), max_points, allow_extrapolation, out.data(), GPP_MEM_HOST));
    detail::ensi_warnings();
    return detail::unflatten(out, N, E);
}
inline vec3 optimal_interpolation_ensi(const Grid& bgrid, const vec3& background, const Points& points, const vec& pobs, const vec& psigmas,
                                       const vec2& pbackground, const StructureFunction& structure, int max_points, bool allow_extrapolation = true) {
    if(max_points < 0) throw std::invalid_argument("max_points must be >= 0");
    if(points.size() == 0) return background;
    if(bgrid.size()[0] == 0 || bgrid.size()[1] == 0) throw std::invalid_argument("Grid size cannot be zero");
    if(bgrid.get_coordinate_type() != points.get_coordinate_type())
        throw std::invalid_argument("Both background grid and observations points must be of same coordinate type (lat/lon or x/y)");
    size_t Y, X, E, S, E2;
    vec bg = detail::flatten(background, Y, X, E), pbg = detail::flatten(pbackground, S, E2);
    detail::check_grid_field(bgrid, Y, X);
    if((int)pobs.size() != points.size() || (int)psigmas.size() != points.size() || (int)S != points.size())
        throw std::invalid_argument("Observations / sigmas / background and points size mismatch");
    if(E != E2) throw std::invalid_argument("Ensemble members in gridded background is not the same as in the point background");
    vec out(bg.size());
    detail::check(gpp_optimal_interpolation_ensi(bgrid.handle(), bg.data(), (int)E, points.handle(), pobs.data(), psigmas.data(), pbg.data(),
                                                 structure.c_struct(), max_points, allow_extrapolation, out.data(), GPP_MEM_HOST));
    detail::ensi_warnings();
    return detail::unflatten(out, Y, X, E);
}

// include/gridpp.h:311-441 (optimal_interpolation_ensi_multi_ebe / _ebesc / _utem; variant 1 / 2 / 3 of the C-ABI entry point)
namespace detail {
inline vec2 ensi_multi_points(int variant, gpp_points* bhandle, int bsize, CoordinateType btype, const vec& bratios, const vec2& background, const vec2* background_corr,
                              const Points& points, const vec* pobs1, const vec2* pobs2, const vec& pratios, const vec2& pbackground,
                              const vec2* pbackground_corr, const StructureFunction& structure, int max_points, bool allow_extrapolation) {
    if(max_points < 0) throw std::invalid_argument("max_points must be >= 0");
    if(btype != points.get_coordinate_type())
        throw std::invalid_argument("Both background and observations points must be of same coorindate type (lat/lon or x/y)");
    if((int)background.size() != bsize) throw std::invalid_argument("Input background field is not the same size as the grid");
    if(background_corr && (int)background_corr->size() != bsize) throw std::invalid_argument("Input background_corr field is not the same size as the grid");
    if((int)bratios.size() != bsize) throw std::invalid_argument("Bratios and grid size mismatch");
    if((int)(pobs1 ? pobs1->size() : pobs2->size()) != points.size()) throw std::invalid_argument("Observations and points exception mismatch");
    if((int)pratios.size() != points.size()) throw std::invalid_argument("Pratios and points size mismatch");
    if((int)pbackground.size() != points.size()) throw std::invalid_argument("Background and points size mismatch");
    if(pbackground_corr && (int)pbackground_corr->size() != points.size()) throw std::invalid_argument("Background_corr and points size mismatch");
    if(points.size() == 0) return background;
    size_t N, E, S, E2;
    vec bg = flatten(background, N, E), pbg = flatten(pbackground, S, E2), bgc, pbgc, po;
    if(background_corr) { size_t a, b; bgc = flatten(*background_corr, a, b); pbgc = flatten(*pbackground_corr, a, b); }
    if(pobs2) { size_t a, b; po = flatten(*pobs2, a, b); } else po = *pobs1;
    if(E != E2) throw std::invalid_argument("Ensemble size mismatch");
    vec out(bg.size());
    check(gpp_optimal_interpolation_ensi_multi(variant, bhandle, bratios.data(), bg.data(), background_corr ? bgc.data() : nullptr, (int)E,
                                               points.handle(), po.data(), pratios.data(), pbg.data(), pbackground_corr ? pbgc.data() : nullptr,
                                               structure.c_struct(), max_points, allow_extrapolation, out.data(), GPP_MEM_HOST));
    return unflatten(out, N, E);
}
}  // namespace detail
inline vec2 optimal_interpolation_ensi_multi_ebe(const Points& bpoints, const vec& bratios, const vec2& background, const vec2& background_corr,
                                                 const Points& obs_points, const vec2& pobs, const vec& pratios, const vec2& pbackground,
                                                 const vec2& pbackground_corr, const StructureFunction& structure, int max_points, bool allow_extrapolation = true) {
    return detail::ensi_multi_points(1, bpoints.handle(), bpoints.size(), bpoints.get_coordinate_type(), bratios, background, &background_corr, obs_points, nullptr, &pobs, pratios, pbackground, &pbackground_corr,
                                     structure, max_points, allow_extrapolation);
}
inline vec2 optimal_interpolation_ensi_multi_ebesc(const Points& bpoints, const vec& bratios, const vec2& background, const Points& obs_points, const vec2& pobs,
                                                   const vec& pratios, const vec2& pbackground, const StructureFunction& structure, int max_points,
                                                   bool allow_extrapolation = true) {
    return detail::ensi_multi_points(2, bpoints.handle(), bpoints.size(), bpoints.get_coordinate_type(), bratios, background, nullptr, obs_points, nullptr, &pobs, pratios, pbackground, nullptr, structure, max_points,
                                     allow_extrapolation);
}
inline vec2 optimal_interpolation_ensi_multi_utem(const Points& bpoints, const vec& bratios, const vec2& background, const vec2& background_corr,
                                                  const Points& obs_points, const vec& pobs, const vec& pratios, const vec2& pbackground,
                                                  const vec2& pbackground_corr, const StructureFunction& structure, int max_points, bool allow_extrapolation = true) {
    return detail::ensi_multi_points(3, bpoints.handle(), bpoints.size(), bpoints.get_coordinate_type(), bratios, background, &background_corr, obs_points, &pobs, nullptr, pratios, pbackground, &pbackground_corr,
                                     structure, max_points, allow_extrapolation);
}
// Grid overloads (src/api/oi_ensi_multi.cpp:34-327): the grid's points in row-major order, fields flattened the same way
namespace detail {
inline vec2 flat_field(const vec3& f) { vec2 o; for(const auto& row : f) for(const auto& c : row) o.push_back(c); return o; }
inline vec flat_field(const vec2& f) { vec o; for(const auto& row : f) for(float c : row) o.push_back(c); return o; }
inline vec3 unflat_field(const vec2& f, size_t Y, size_t X) { vec3 o(Y, vec2(X)); for(size_t y = 0; y < Y; y++) for(size_t x = 0; x < X; x++) o[y][x] = f[y * X + x]; return o; }
}  // namespace detail
inline vec3 optimal_interpolation_ensi_multi_ebe(const Grid& bgrid, const vec2& bratios, const vec3& background, const vec3& background_corr,
                                                 const Points& obs_points, const vec2& pobs, const vec& pratios, const vec2& pbackground,
                                                 const vec2& pbackground_corr, const StructureFunction& structure, int max_points, bool allow_extrapolation = true) {
    const vec2 bgc = detail::flat_field(background_corr);
    return detail::unflat_field(detail::ensi_multi_points(1, bgrid.handle(), bgrid.size()[0] * bgrid.size()[1], bgrid.get_coordinate_type(), detail::flat_field(bratios),
                                detail::flat_field(background), &bgc, obs_points, nullptr, &pobs, pratios, pbackground, &pbackground_corr, structure, max_points,
                                allow_extrapolation), background.size(), background.empty() ? 0 : background[0].size());
}
inline vec3 optimal_interpolation_ensi_multi_ebesc(const Grid& bgrid, const vec2& bratios, const vec3& background, const Points& obs_points, const vec2& pobs,
                                                   const vec& pratios, const vec2& pbackground, const StructureFunction& structure, int max_points,
                                                   bool allow_extrapolation = true) {
    return detail::unflat_field(detail::ensi_multi_points(2, bgrid.handle(), bgrid.size()[0] * bgrid.size()[1], bgrid.get_coordinate_type(), detail::flat_field(bratios),
                                detail::flat_field(background), nullptr, obs_points, nullptr, &pobs, pratios, pbackground, nullptr, structure, max_points, allow_extrapolation), background.size(), background.empty() ? 0 : background[0].size());
}
inline vec3 optimal_interpolation_ensi_multi_utem(const Grid& bgrid, const vec2& bratios, const vec3& background, const vec3& background_corr,
                                                  const Points& obs_points, const vec& pobs, const vec& pratios, const vec2& pbackground,
                                                  const vec2& pbackground_corr, const StructureFunction& structure, int max_points, bool allow_extrapolation = true) {
    const vec2 bgc = detail::flat_field(background_corr);
    return detail::unflat_field(detail::ensi_multi_points(3, bgrid.handle(), bgrid.size()[0] * bgrid.size()[1], bgrid.get_coordinate_type(), detail::flat_field(bratios),
                                detail::flat_field(background), &bgc, obs_points, &pobs, nullptr, pratios, pbackground, &pbackground_corr, structure, max_points,
                                allow_extrapolation), background.size(), background.empty() ? 0 : background[0].size());
}

// ---- multi-GPU: one process per GPU, contiguous row tiles, observation values broadcast from rank 0 over RCCL --------
// No counterpart in include/gridpp.h (the reference's parallelism is OpenMP).  Usage, on every rank:
//     gridpp::multi::init(rank, world, id);                      // id from multi::unique_id() on rank 0, distributed by the caller
//     multi::row_tile(Y, rank, world, r0, r1);                   // build Grid(lats[r0:r1], lons[r0:r1]) and the full Points
//     tile = multi::optimal_interpolation(tile_grid, tile_background, points, pobs, pratios, pbackground, structure, max_points);
// pobs / pratios / pbackground need valid contents on rank 0 only (the other ranks pass vectors of the right size).
namespace multi {
inline void row_tile(int ny, int rank, int world, int& row0, int& row1) { detail::check(gpp_row_tile(ny, rank, world, &row0, &row1)); }
inline std::string unique_id() { std::string id(128, '\0'); detail::check(gpp_comm_unique_id(&id[0])); return id; }
inline void init(int rank, int world, const std::string& id) {
    if(id.size() != 128) throw std::invalid_argument("multi::init: the id must hold 128 bytes");
    detail::check(gpp_comm_init(rank, world, id.data()));
}
inline void destroy() { detail::check(gpp_comm_destroy()); }
inline void broadcast(vec& values, int root = 0) { detail::check(gpp_comm_broadcast_host(values.data(), values.size() * sizeof(float), root)); }
inline vec2 optimal_interpolation(const Grid& tile_grid, const vec2& tile_background, const Points& points, vec& pobs, vec& pratios, vec& pbackground,
                                  const StructureFunction& structure, int max_points, bool allow_extrapolation = true) {
    if((int)pobs.size() != points.size() || (int)pratios.size() != points.size() || (int)pbackground.size() != points.size())
        throw std::invalid_argument("Observations / ratios / background and points size mismatch");
    vec block;                                   // one broadcast for the three vectors
    block.reserve(3 * pobs.size());
    block.insert(block.end(), pobs.begin(), pobs.end());
    block.insert(block.end(), pratios.begin(), pratios.end());
    block.insert(block.end(), pbackground.begin(), pbackground.end());
    broadcast(block, 0);
    const size_t S = pobs.size();
    std::copy(block.begin(), block.begin() + S, pobs.begin());
    std::copy(block.begin() + S, block.begin() + 2 * S, pratios.begin());
    std::copy(block.begin() + 2 * S, block.end(), pbackground.begin());
    return gridpp::optimal_interpolation(tile_grid, tile_background, points, pobs, pratios, pbackground, structure, max_points, allow_extrapolation);
}
}  // namespace multi

// ---- neighbourhood (include/gridpp.h:588-716) ---------------------------------------------------------------
namespace detail {
inline vec2 nb(const vec& f, size_t Y, size_t X, size_t E, int is3d, int halfwidth, Statistic statistic) {
    if(halfwidth < 0) throw std::invalid_argument("Half width must be > 0");
    if(statistic == Quantile) throw std::invalid_argument("Use neighbourhood_quantile for computing neighbourhood quantiles");
    if(Y * X * E == 0) return vec2();
    vec out(Y * X);
    check(gpp_neighbourhood(f.data(), (int)Y, (int)X, (int)E, is3d, halfwidth, (int)statistic, out.data(), GPP_MEM_HOST));
    return unflatten(out, Y, X);
}
inline vec2 brute(const vec& f, size_t Y, size_t X, size_t E, int halfwidth, int statistic, float q) {
    if(halfwidth < 0) throw std::invalid_argument("Half width must be > 0");
    if(Y * X * E == 0) return vec2();
    vec out(Y * X);
    check(gpp_neighbourhood_brute_force(f.data(), (int)Y, (int)X, (int)E, halfwidth, statistic, q, out.data(), GPP_MEM_HOST));
    return unflatten(out, Y, X);
}
inline vec2 qfast(const vec& f, size_t Y, size_t X, size_t E, int is3d, const vec2& quantile, int halfwidth, const vec& thresholds) {
    if(halfwidth < 0) throw std::invalid_argument("Half width must be > 0");
    if(Y * X * E == 0) return vec2();
    size_t Yq, Xq;
    vec q = flatten(quantile, Yq, Xq);
    if(!(Yq == 1 && Xq == 1) && !(Yq == Y && Xq == X)) throw std::invalid_argument("Quantile must be the same size as input, or size (1, 1)");
    vec out(Y * X);
    check(gpp_neighbourhood_quantile_fast(f.data(), (int)Y, (int)X, (int)E, is3d, q.data(), (int)q.size(), halfwidth, thresholds.data(),
                                          (int)thresholds.size(), out.data(), GPP_MEM_HOST));
    return unflatten(out, Y, X);
}
}
inline vec2 neighbourhood(const vec2& input, int halfwidth, Statistic statistic) { size_t Y, X; vec f = detail::flatten(input, Y, X); return detail::nb(f, Y, X, 1, 0, halfwidth, statistic); }
inline vec2 neighbourhood(const vec3& input, int halfwidth, Statistic statistic) { size_t Y, X, E; vec f = detail::flatten(input, Y, X, E); return detail::nb(f, Y, X, E, 1, halfwidth, statistic); }
inline vec2 neighbourhood_brute_force(const vec2& input, int halfwidth, Statistic statistic) { size_t Y, X; vec f = detail::flatten(input, Y, X); return detail::brute(f, Y, X, 1, halfwidth, statistic, 0); }
inline vec2 neighbourhood_brute_force(const vec3& input, int halfwidth, Statistic statistic) { size_t Y, X, E; vec f = detail::flatten(input, Y, X, E); return detail::brute(f, Y, X, E, halfwidth, statistic, 0); }
inline vec2 neighbourhood_quantile(const vec2& input, float quantile, int halfwidth) { size_t Y, X; vec f = detail::flatten(input, Y, X); return detail::brute(f, Y, X, 1, halfwidth, Quantile, quantile); }
inline vec2 neighbourhood_quantile(const vec3& input, float quantile, int halfwidth) { size_t Y, X, E; vec f = detail::flatten(input, Y, X, E); return detail::brute(f, Y, X, E, halfwidth, Quantile, quantile); }
inline vec2 neighbourhood_quantile_fast(const vec2& input, const vec2& quantile, int halfwidth, const vec& thresholds) { size_t Y, X; vec f = detail::flatten(input, Y, X); return detail::qfast(f, Y, X, 1, 0, quantile, halfwidth, thresholds); }
inline vec2 neighbourhood_quantile_fast(const vec2& input, float quantile, int halfwidth, const vec& thresholds) { return neighbourhood_quantile_fast(input, vec2(1, vec(1, quantile)), halfwidth, thresholds); }
inline vec2 neighbourhood_quantile_fast(const vec3& input, const vec2& quantile, int halfwidth, const vec& thresholds) { size_t Y, X, E; vec f = detail::flatten(input, Y, X, E); return detail::qfast(f, Y, X, E, 1, quantile, halfwidth, thresholds); }
inline vec2 neighbourhood_quantile_fast(const vec3& input, float quantile, int halfwidth, const vec& thresholds) { return neighbourhood_quantile_fast(input, vec2(1, vec(1, quantile)), halfwidth, thresholds); }
// deprecated aliases (include/gridpp.h:710-716, src/api/neighbourhood.cpp:541-552)
inline vec2 neighbourhood_ens(const vec3& input, int halfwidth, Statistic statistic) { future_deprecation_warning("neighbourhood_ens", "neighbourhood"); return neighbourhood(input, halfwidth, statistic); }
inline vec2 neighbourhood_quantile_ens(const vec3& input, float quantile, int halfwidth) { future_deprecation_warning("neighbourhood_quantile_ens", "neighbourhood_quantile"); return neighbourhood_quantile(input, quantile, halfwidth); }
inline vec2 neighbourhood_quantile_ens_fast(const vec3& input, float quantile, int radius, const vec& thresholds) { future_deprecation_warning("neighbourhood_quantile_ens_fast", "neighbourhood_quantile_fast"); return neighbourhood_quantile_fast(input, quantile, radius, thresholds); }
namespace detail {
inline vec thresholds(const vec& f, int num) {
    if(num <= 0) throw std::invalid_argument("num_thresholds must be > 0");
    if(f.empty()) return vec();
    vec out(num >= (int)f.size() ? f.size() : num); int count = 0;
    check(gpp_calc_even_quantiles(f.data(), (long)f.size(), num, 1, out.data(), &count, GPP_MEM_HOST));
    out.resize(count);
    return out;
}
}
inline vec get_neighbourhood_thresholds(const vec2& input, int num_thresholds) { size_t Y, X; return detail::thresholds(detail::flatten(input, Y, X), num_thresholds); }
inline vec get_neighbourhood_thresholds(const vec3& input, int num_thresholds) { size_t Y, X, E; return detail::thresholds(detail::flatten(input, Y, X, E), num_thresholds); }

// ---- nearest (include/gridpp.h:895; src/api/nearest.cpp:124-144) ------------------------------------------------
namespace detail {
// values [T][n] flattened -> [T][nq]; `sized` = the size check of the overload passed (src/api/util.cpp:427-438)
inline vec nearest_flat(gpp_points* from, size_t nfrom, gpp_points* to, size_t nq, const vec& v, size_t T, bool sized, const char* what) {
    if(!sized) throw std::invalid_argument(what);
    vec out(T * nq, MV);
    if(T * nq == 0 || nfrom == 0) return out;
    if(v.size() != T * nfrom) throw std::invalid_argument(what);
    check(gpp_nearest_levels(from, to, v.data(), (int)T, out.data(), GPP_MEM_HOST));
    return out;
}
inline size_t cells(const Grid& g) { return (size_t)g.size()[0] * g.size()[1]; }
inline bool fits(const Grid& g, size_t Y, size_t X) { return (int)Y == g.size()[0] && (int)X == g.size()[1]; }
const char* const GRID_MISMATCH = "Grid size is not the same as values";
const char* const POINTS_MISMATCH = "Points size is not the same as values";
}   // namespace detail
// the eight overloads of src/api/nearest.cpp:7-222
inline vec nearest(const Grid& igrid, const Points& opoints, const vec2& ivalues) {
    size_t Y, X;
    vec v = detail::flatten(ivalues, Y, X);
    return detail::nearest_flat(igrid.handle(), detail::cells(igrid), opoints.handle(), opoints.size(), v, 1, Y == 0 || detail::fits(igrid, Y, X), detail::GRID_MISMATCH);
}
inline vec2 nearest(const Grid& igrid, const Points& opoints, const vec3& ivalues) {
    size_t T, Y, X;
    vec v = detail::flatten(ivalues, T, Y, X);
    return detail::unflatten(detail::nearest_flat(igrid.handle(), detail::cells(igrid), opoints.handle(), opoints.size(), v, T,
                                                  T == 0 || Y == 0 || detail::fits(igrid, Y, X), detail::GRID_MISMATCH), T, opoints.size());
}
inline vec2 nearest(const Grid& igrid, const Grid& ogrid, const vec2& ivalues) {
    size_t Y, X;
    vec v = detail::flatten(ivalues, Y, X);
    return detail::unflatten(detail::nearest_flat(igrid.handle(), detail::cells(igrid), ogrid.handle(), detail::cells(ogrid), v, 1,
                                                  Y == 0 || detail::fits(igrid, Y, X), detail::GRID_MISMATCH), ogrid.size()[0], ogrid.size()[1]);
}
inline vec3 nearest(const Grid& igrid, const Grid& ogrid, const vec3& ivalues) {
    size_t T, Y, X;
    vec v = detail::flatten(ivalues, T, Y, X);
    return detail::unflatten(detail::nearest_flat(igrid.handle(), detail::cells(igrid), ogrid.handle(), detail::cells(ogrid), v, T,
                                                  T == 0 || Y == 0 || detail::fits(igrid, Y, X), detail::GRID_MISMATCH), T, ogrid.size()[0], ogrid.size()[1]);
}
inline vec nearest(const Points& ipoints, const Points& opoints, const vec& ivalues) {
    return detail::nearest_flat(ipoints.handle(), ipoints.size(), opoints.handle(), opoints.size(), ivalues, 1, (int)ivalues.size() == ipoints.size(), detail::POINTS_MISMATCH);
}
inline vec2 nearest(const Points& ipoints, const Points& opoints, const vec2& ivalues) {
    size_t T, N;
    vec v = detail::flatten(ivalues, T, N);
    return detail::unflatten(detail::nearest_flat(ipoints.handle(), ipoints.size(), opoints.handle(), opoints.size(), v, T,
                                                  T == 0 || (int)N == ipoints.size(), detail::POINTS_MISMATCH), T, opoints.size());
}
inline vec2 nearest(const Points& ipoints, const Grid& ogrid, const vec& ivalues) {
    return detail::unflatten(detail::nearest_flat(ipoints.handle(), ipoints.size(), ogrid.handle(), detail::cells(ogrid), ivalues, 1,
                                                  (int)ivalues.size() == ipoints.size(), detail::POINTS_MISMATCH), ogrid.size()[0], ogrid.size()[1]);
}
inline vec3 nearest(const Points& ipoints, const Grid& ogrid, const vec2& ivalues) {
    size_t T, N;
    vec v = detail::flatten(ivalues, T, N);
    return detail::unflatten(detail::nearest_flat(ipoints.handle(), ipoints.size(), ogrid.handle(), detail::cells(ogrid), v, T,
                                                  T == 0 || (int)N == ipoints.size(), detail::POINTS_MISMATCH), T, ogrid.size()[0], ogrid.size()[1]);
}

// ---- count / gridding (include/gridpp.h:938-1010; src/api/count.cpp:6-66, src/api/gridding.cpp:6-131) -------------
inline vec count(const Points& ipoints, const Points& opoints, float radius) {
    vec out(opoints.size(), 0);
    if(opoints.size()) detail::check(gpp_count(ipoints.handle(), opoints.handle(), radius, out.data(), GPP_MEM_HOST));
    return out;
}
inline vec count(const Grid& igrid, const Points& opoints, float radius) {
    vec out(opoints.size(), 0);
    if(opoints.size()) detail::check(gpp_count(igrid.handle(), opoints.handle(), radius, out.data(), GPP_MEM_HOST));
    return out;
}
inline vec2 count(const Points& ipoints, const Grid& ogrid, float radius) {
    vec out(detail::cells(ogrid), 0);
    if(out.size()) detail::check(gpp_count(ipoints.handle(), ogrid.handle(), radius, out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, ogrid.size()[0], ogrid.size()[1]);
}
inline vec2 count(const Grid& igrid, const Grid& ogrid, float radius) {
    vec out(detail::cells(ogrid), 0);
    if(out.size()) detail::check(gpp_count(igrid.handle(), ogrid.handle(), radius, out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, ogrid.size()[0], ogrid.size()[1]);
}
// distance (include/gridpp.h; src/api/distance.cpp:6-120): largest calc_distance to the `num` nearest points of the input set
inline vec distance(const Grid& grid, const Points& points, int num) {
    if(grid.get_coordinate_type() != points.get_coordinate_type()) throw std::invalid_argument("Incompatible coordinate types");
    vec out(points.size(), 0);
    if(points.size()) detail::check(gpp_distance(grid.handle(), points.handle(), num, 1, out.data(), GPP_MEM_HOST));
    return out;
}
inline vec distance(const Points& ipoints, const Points& opoints, int num) {
    if(ipoints.get_coordinate_type() != opoints.get_coordinate_type()) throw std::invalid_argument("Incompatible coordinate types");
    vec out(opoints.size(), 0);
    if(opoints.size()) detail::check(gpp_distance(ipoints.handle(), opoints.handle(), num, 1, out.data(), GPP_MEM_HOST));
    return out;
}
inline vec2 distance(const Grid& igrid, const Grid& ogrid, int num) {
    if(igrid.get_coordinate_type() != ogrid.get_coordinate_type()) throw std::invalid_argument("Incompatible coordinate types");
    vec out(detail::cells(ogrid), 0);
    if(out.size()) detail::check(gpp_distance(igrid.handle(), ogrid.handle(), num, 0, out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, ogrid.size()[0], ogrid.size()[1]);
}
inline vec2 distance(const Points& points, const Grid& grid, int num) {
    if(points.get_coordinate_type() != grid.get_coordinate_type()) throw std::invalid_argument("Incompatible coordinate types");
    vec out(detail::cells(grid), 0);
    if(out.size()) detail::check(gpp_distance(points.handle(), grid.handle(), num, 0, out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, grid.size()[0], grid.size()[1]);
}
namespace detail {
inline vec gridding_flat(gpp_points* to, size_t nout, const Points& points, const vec& values, float radius, int min_num, Statistic statistic, bool nearest) {
    if((int)values.size() != points.size()) throw std::invalid_argument("Points size is not the same as values");
    if(!nearest && (std::isnan(radius) || std::isinf(radius) || radius < 0)) throw std::invalid_argument("radius must be >= 0");
    if(min_num < 0) throw std::invalid_argument("min_num must be >= 0");
    vec out(nout, MV);
    if(nearest) { if(nout || points.size()) check(gpp_gridding_nearest(to, points.handle(), values.data(), min_num, (int)statistic, out.data(), GPP_MEM_HOST)); }
    else if(nout) check(gpp_gridding(to, points.handle(), values.data(), radius, min_num, (int)statistic, out.data(), GPP_MEM_HOST));
    return out;
}
}   // namespace detail
inline vec2 gridding(const Grid& grid, const Points& points, const vec& values, float radius, int min_num, Statistic statistic) {
    return detail::unflatten(detail::gridding_flat(grid.handle(), detail::cells(grid), points, values, radius, min_num, statistic, false), grid.size()[0], grid.size()[1]);
}
inline vec gridding(const Points& opoints, const Points& ipoints, const vec& values, float radius, int min_num, Statistic statistic) {
    return detail::gridding_flat(opoints.handle(), opoints.size(), ipoints, values, radius, min_num, statistic, false);
}
inline vec2 gridding_nearest(const Grid& grid, const Points& points, const vec& values, int min_num, Statistic statistic) {
    return detail::unflatten(detail::gridding_flat(grid.handle(), detail::cells(grid), points, values, 0, min_num, statistic, true), grid.size()[0], grid.size()[1]);
}
inline vec gridding_nearest(const Points& opoints, const Points& ipoints, const vec& values, int min_num, Statistic statistic) {
    return detail::gridding_flat(opoints.handle(), opoints.size(), ipoints, values, 0, min_num, statistic, true);
}

// ---- fill / doping / neighbourhood_search / calc_gradient (src/api/fill.cpp, doping.cpp, neighbourhood_search.cpp,
//      calc_gradient.cpp) ---------------------------------------------------------------------------------------------
enum GradientType { MinMax = 0, LinearRegression = 10 };   // include/gridpp.h:126-129
inline vec2 fill(const Grid& igrid, const vec2& input, const Points& points, const vec& radii, float value, bool outside) {
    size_t Y, X;
    vec v = detail::flatten(input, Y, X);
    if(Y != 0 && !detail::fits(igrid, Y, X)) throw std::invalid_argument("Grid size is not the same as values");
    if((int)radii.size() != points.size()) throw std::invalid_argument("Points size is not the same as radii size");
    vec out(v.size(), MV);
    if(v.size()) detail::check(gpp_fill(igrid.handle(), v.data(), points.handle(), radii.data(), value, outside, out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, Y, X);
}
inline vec2 fill_missing(const vec2& values) {
    size_t Y, X;
    vec v = detail::flatten(values, Y, X);
    vec out(v.size(), MV);
    if(v.size()) detail::check(gpp_fill_missing(v.data(), (int)Y, (int)X, out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, Y, X);
}
namespace detail {
inline vec2 doping(const Grid& igrid, const vec2& background, const Points& points, const vec& observations, const int* halfwidth, const float* radii,
                   size_t nper, float max_elev_diff) {
    size_t Y, X;
    vec v = flatten(background, Y, X);
    if(Y != 0 && !fits(igrid, Y, X)) throw std::invalid_argument("Grid size is not the same as observations");
    if((int)observations.size() != points.size()) throw std::invalid_argument("Points size is not the same as observations size");
    if((int)nper != points.size()) throw std::invalid_argument(halfwidth ? "Points size is not the same as halfwidth size" : "Points size is not the same as radii size");
    vec out(v.size(), MV);
    if(v.size()) check(gpp_doping(igrid.handle(), v.data(), points.handle(), observations.data(), halfwidth, radii, max_elev_diff, out.data(), GPP_MEM_HOST));
    return unflatten(out, Y, X);
}
}   // namespace detail
inline vec2 doping_square(const Grid& igrid, const vec2& background, const Points& points, const vec& observations, const ivec& halfwidth, float max_elev_diff = MV) {
    return detail::doping(igrid, background, points, observations, halfwidth.data(), nullptr, halfwidth.size(), max_elev_diff);
}
inline vec2 doping_circle(const Grid& igrid, const vec2& background, const Points& points, const vec& observations, const vec& radii, float max_elev_diff = MV) {
    return detail::doping(igrid, background, points, observations, nullptr, radii.data(), radii.size(), max_elev_diff);
}
inline vec2 neighbourhood_search(const vec2& array, const vec2& search_array, int halfwidth, float search_target_min, float search_target_max,
                                 float search_delta, const ivec2& apply_array = ivec2()) {
    size_t Y, X, Ys, Xs;
    vec a = detail::flatten(array, Y, X), s = detail::flatten(search_array, Ys, Xs);
    if(Y != Ys || X != Xs) throw std::invalid_argument("search_array must either be the same size as array");
    ivec ap;
    if(apply_array.size() > 0) {
        if(apply_array.size() > 1 && (apply_array.size() != Y || apply_array[0].size() != X)) throw std::invalid_argument("apply_array must either be empty or same size as array");
        for(const auto& r : apply_array) ap.insert(ap.end(), r.begin(), r.end());
    }
    vec out(a.size(), MV);
    if(a.size()) detail::check(gpp_neighbourhood_search(a.data(), s.data(), (int)Y, (int)X, halfwidth, search_target_min, search_target_max, search_delta,
                                                        ap.size() == a.size() ? ap.data() : nullptr, out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, Y, X);
}
inline vec2 calc_gradient(const vec2& base, const vec2& values, GradientType gradient_type, int halfwidth, int min_num = 2, float min_range = MV,
                          float default_gradient = 0) {
    size_t Y, X, Yv, Xv;
    vec b = detail::flatten(base, Y, X), v = detail::flatten(values, Yv, Xv);
    if(Y == 0) throw std::invalid_argument("base input has no size");
    if(Y != Yv || X != Xv) throw std::invalid_argument("base is not the same size as values");
    vec out(b.size(), MV);
    detail::check(gpp_calc_gradient(b.data(), v.data(), (int)Y, (int)X, (int)gradient_type, halfwidth, min_num, min_range, default_gradient, out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, Y, X);
}

// ---- bilinear (include/gridpp.h:902-930; src/api/bilinear.cpp:26-135) -------------------------------------------
namespace detail {
// values [T][Y][X] flattened; size rule of src/api/util.cpp:427-432
inline vec bilinear_flat(const Grid& igrid, gpp_points* to, size_t nq, const vec& v, size_t T, size_t Y, size_t X, bool empty) {
    if(!empty && ((int)Y != igrid.size()[0] || (int)X != igrid.size()[1])) throw std::invalid_argument("Grid size is not the same as values");
    vec out(T * nq, MV);
    if(T * nq == 0 || igrid.size()[0] == 0 || igrid.size()[1] == 0) return out;   // bilinear.cpp:37-39
    if(empty) throw std::invalid_argument("Grid size is not the same as values");
    check(gpp_bilinear(igrid.handle(), to, v.data(), (int)T, out.data(), GPP_MEM_HOST));
    return out;
}
}   // namespace detail
inline vec bilinear(const Grid& igrid, const Points& opoints, const vec2& ivalues) {
    size_t Y, X;
    vec v = detail::flatten(ivalues, Y, X);
    return detail::bilinear_flat(igrid, opoints.handle(), opoints.size(), v, 1, Y, X, ivalues.size() == 0);
}
inline vec2 bilinear(const Grid& igrid, const Points& opoints, const vec3& ivalues) {
    size_t T, Y, X;
    vec v = detail::flatten(ivalues, T, Y, X);
    vec out = detail::bilinear_flat(igrid, opoints.handle(), opoints.size(), v, T, Y, X, T == 0 || Y == 0);
    return detail::unflatten(out, T, opoints.size());
}
inline vec2 bilinear(const Grid& igrid, const Grid& ogrid, const vec2& ivalues) {
    size_t Y, X;
    vec v = detail::flatten(ivalues, Y, X);
    size_t oy = ogrid.size()[0], ox = ogrid.size()[1];
    return detail::unflatten(detail::bilinear_flat(igrid, ogrid.handle(), oy * ox, v, 1, Y, X, ivalues.size() == 0), oy, ox);
}
inline vec3 bilinear(const Grid& igrid, const Grid& ogrid, const vec3& ivalues) {
    size_t T, Y, X;
    vec v = detail::flatten(ivalues, T, Y, X);
    size_t oy = ogrid.size()[0], ox = ogrid.size()[1];
    return detail::unflatten(detail::bilinear_flat(igrid, ogrid.handle(), oy * ox, v, T, Y, X, T == 0 || Y == 0), T, oy, ox);
}

// ---- downscaling, simple_gradient, full_gradient (include/gridpp.h:844-871,1017-1098) -------------------------------
namespace detail {
inline void check_downscaler(Downscaler d) { if(d != Nearest && d != Bilinear) throw std::invalid_argument("Invalid downscaler"); }   // downscaling.cpp:16-17
// values [T][Y][X] flattened -> [T][nq]; eg / lg NULL = that term is absent (full_gradient) -- simple_gradient passes neither
inline vec gradient_flat(bool full, const Grid& igrid, gpp_points* to, size_t nq, const vec& v, size_t T, bool empty, const vec* eg,
                         const vec* lg, float elev_gradient, Downscaler downscaler) {
    check_downscaler(downscaler);
    vec out(T * nq, MV);
    if(T * nq == 0) return out;
    if(cells(igrid) && empty) throw std::invalid_argument(GRID_MISMATCH);
    if(full) check(gpp_full_gradient(igrid.handle(), to, v.data(), (int)T, eg ? eg->data() : nullptr, lg ? lg->data() : nullptr, (int)downscaler,
                                     out.data(), GPP_MEM_HOST));
    else check(gpp_simple_gradient(igrid.handle(), to, v.data(), (int)T, elev_gradient, (int)downscaler, out.data(), GPP_MEM_HOST));
    return out;
}
inline bool compatible(const Grid& g, const vec2& v) { return v.size() == 0 || fits(g, v.size(), v[0].size()); }   // util.cpp:427-429
inline bool compatible(const Grid& g, const vec3& v) { return v.size() == 0 || v[0].size() == 0 || fits(g, v[0].size(), v[0][0].size()); }   // :430-432
// a gradient of the reference's size() == 0 is absent (NULL); any other must have the shape of the values (gradient.cpp:13-20;
// the other overloads only assert it and would read past the end)
inline const vec* gradient_field(const vec2& g, vec& flat, size_t Y, size_t X, const char* what) {
    if(g.size() == 0) return nullptr;
    size_t a, b;
    flat = flatten(g, a, b);
    if(a != Y || b != X) throw std::invalid_argument(what);
    return &flat;
}
inline const vec* gradient_field(const vec3& g, vec& flat, size_t T, size_t Y, size_t X, const char* what) {
    if(g.size() == 0) return nullptr;
    size_t a, b, c;
    flat = flatten(g, a, b, c);
    if(a != T || b != Y || c != X) throw std::invalid_argument(what);
    return &flat;
}
const char* const LAF_MISMATCH = "Laf gradient is the wrong size";
const char* const ELEV_MISMATCH = "Elevation gradient is the wrong size";
}   // namespace detail
// src/api/downscaling.cpp:7-61
inline vec downscaling(const Grid& igrid, const Points& opoints, const vec2& ivalues, Downscaler downscaler) {
    if(!detail::compatible(igrid, ivalues)) throw std::invalid_argument(detail::GRID_MISMATCH);
    detail::check_downscaler(downscaler);
    return downscaler == Nearest ? nearest(igrid, opoints, ivalues) : bilinear(igrid, opoints, ivalues);
}
inline vec2 downscaling(const Grid& igrid, const Grid& ogrid, const vec2& ivalues, Downscaler downscaler) {
    if(!detail::compatible(igrid, ivalues)) throw std::invalid_argument(detail::GRID_MISMATCH);
    detail::check_downscaler(downscaler);
    return downscaler == Nearest ? nearest(igrid, ogrid, ivalues) : bilinear(igrid, ogrid, ivalues);
}
inline vec2 downscaling(const Grid& igrid, const Points& opoints, const vec3& ivalues, Downscaler downscaler) {
    if(!detail::compatible(igrid, ivalues)) throw std::invalid_argument(detail::GRID_MISMATCH);
    detail::check_downscaler(downscaler);
    return downscaler == Nearest ? nearest(igrid, opoints, ivalues) : bilinear(igrid, opoints, ivalues);
}
inline vec3 downscaling(const Grid& igrid, const Grid& ogrid, const vec3& ivalues, Downscaler downscaler) {
    if(!detail::compatible(igrid, ivalues)) throw std::invalid_argument(detail::GRID_MISMATCH);
    detail::check_downscaler(downscaler);
    return downscaler == Nearest ? nearest(igrid, ogrid, ivalues) : bilinear(igrid, ogrid, ivalues);
}
// src/api/simple_gradient.cpp:5-100
inline vec2 simple_gradient(const Grid& igrid, const Grid& ogrid, const vec2& ivalues, float elev_gradient, Downscaler downscaler = Nearest) {
    if(!detail::compatible(igrid, ivalues)) throw std::invalid_argument(detail::GRID_MISMATCH);
    size_t Y, X;
    vec v = detail::flatten(ivalues, Y, X);
    size_t oy = ogrid.size()[0], ox = ogrid.size()[1];
    return detail::unflatten(detail::gradient_flat(false, igrid, ogrid.handle(), oy * ox, v, 1, Y == 0, nullptr, nullptr, elev_gradient, downscaler), oy, ox);
}
inline vec3 simple_gradient(const Grid& igrid, const Grid& ogrid, const vec3& ivalues, float elev_gradient, Downscaler downscaler = Nearest) {
    if(!detail::compatible(igrid, ivalues)) throw std::invalid_argument(detail::GRID_MISMATCH);
    size_t T, Y, X;
    vec v = detail::flatten(ivalues, T, Y, X);
    size_t oy = ogrid.size()[0], ox = ogrid.size()[1];
    return detail::unflatten(detail::gradient_flat(false, igrid, ogrid.handle(), oy * ox, v, T, T == 0 || Y == 0, nullptr, nullptr, elev_gradient, downscaler),
                             T, oy, ox);
}
inline vec simple_gradient(const Grid& igrid, const Points& opoints, const vec2& ivalues, float elev_gradient, Downscaler downscaler = Nearest) {
    if(!detail::compatible(igrid, ivalues)) throw std::invalid_argument(detail::GRID_MISMATCH);
    size_t Y, X;
    vec v = detail::flatten(ivalues, Y, X);
    return detail::gradient_flat(false, igrid, opoints.handle(), opoints.size(), v, 1, Y == 0, nullptr, nullptr, elev_gradient, downscaler);
}
inline vec2 simple_gradient(const Grid& igrid, const Points& opoints, const vec3& ivalues, float elev_gradient, Downscaler downscaler = Nearest) {
    if(!detail::compatible(igrid, ivalues)) throw std::invalid_argument(detail::GRID_MISMATCH);
    size_t T, Y, X;
    vec v = detail::flatten(ivalues, T, Y, X);
    return detail::unflatten(detail::gradient_flat(false, igrid, opoints.handle(), opoints.size(), v, T, T == 0 || Y == 0, nullptr, nullptr, elev_gradient,
                                                   downscaler), T, opoints.size());
}
// src/api/gradient.cpp:5-274
inline vec2 full_gradient(const Grid& igrid, const Grid& ogrid, const vec2& ivalues, const vec2& elev_gradient, const vec2& laf_gradient = vec2(),
                          Downscaler downscaler = Nearest) {
    if((int)ivalues.size() != igrid.size()[0] || (int)(ivalues.size() ? ivalues[0].size() : 0) != igrid.size()[1])   // gradient.cpp:10-11
        throw std::invalid_argument("Values is the wrong size");
    size_t Y, X;
    vec v = detail::flatten(ivalues, Y, X), lf, ef;
    const vec* lg = detail::gradient_field(laf_gradient, lf, Y, X, detail::LAF_MISMATCH);
    const vec* eg = detail::gradient_field(elev_gradient, ef, Y, X, detail::ELEV_MISMATCH);
    size_t oy = ogrid.size()[0], ox = ogrid.size()[1];
    return detail::unflatten(detail::gradient_flat(true, igrid, ogrid.handle(), oy * ox, v, 1, Y == 0, eg, lg, 0, downscaler), oy, ox);
}
inline vec3 full_gradient(const Grid& igrid, const Grid& ogrid, const vec3& ivalues, const vec3& elev_gradient, const vec3& laf_gradient,
                          Downscaler downscaler = Nearest) {
    if(!detail::compatible(igrid, ivalues)) throw std::invalid_argument(detail::GRID_MISMATCH);
    size_t T, Y, X;
    vec v = detail::flatten(ivalues, T, Y, X), lf, ef;
    const vec* lg = detail::gradient_field(laf_gradient, lf, T, Y, X, detail::LAF_MISMATCH);
    const vec* eg = detail::gradient_field(elev_gradient, ef, T, Y, X, detail::ELEV_MISMATCH);
    size_t oy = ogrid.size()[0], ox = ogrid.size()[1];
    return detail::unflatten(detail::gradient_flat(true, igrid, ogrid.handle(), oy * ox, v, T, T == 0 || Y == 0, eg, lg, 0, downscaler), T, oy, ox);
}
inline vec full_gradient(const Grid& igrid, const Points& opoints, const vec2& ivalues, const vec2& elev_gradient, const vec2& laf_gradient,
                         Downscaler downscaler = Nearest) {
    if(!detail::compatible(igrid, ivalues)) throw std::invalid_argument(detail::GRID_MISMATCH);
    size_t Y, X;
    vec v = detail::flatten(ivalues, Y, X), lf, ef;
    const vec* lg = detail::gradient_field(laf_gradient, lf, Y, X, detail::LAF_MISMATCH);
    const vec* eg = detail::gradient_field(elev_gradient, ef, Y, X, detail::ELEV_MISMATCH);
    return detail::gradient_flat(true, igrid, opoints.handle(), opoints.size(), v, 1, Y == 0, eg, lg, 0, downscaler);
}
inline vec2 full_gradient(const Grid& igrid, const Points& opoints, const vec3& ivalues, const vec3& elev_gradient, const vec3& laf_gradient,
                          Downscaler downscaler = Nearest) {
    if(!detail::compatible(igrid, ivalues)) throw std::invalid_argument(detail::GRID_MISMATCH);
    size_t T, Y, X;
    vec v = detail::flatten(ivalues, T, Y, X), lf, ef;
    const vec* lg = detail::gradient_field(laf_gradient, lf, T, Y, X, detail::LAF_MISMATCH);
    const vec* eg = detail::gradient_field(elev_gradient, ef, T, Y, X, detail::ELEV_MISMATCH);
    return detail::unflatten(detail::gradient_flat(true, igrid, opoints.handle(), opoints.size(), v, T, T == 0 || Y == 0, eg, lg, 0, downscaler),
                             T, opoints.size());
}

// ---- ensemble downscalers and smart (include/gridpp.h:945-990,1112) ----------------------------------------------------
namespace detail {
// the checks the reference leaves out (a wrong shape reads out of bounds there); returns the flattened threshold
inline vec ensemble_checks(const Grid& igrid, const Grid& ogrid, size_t Y, size_t X, const vec2& threshold, ComparisonOperator op) {
    if(cells(igrid) && !fits(igrid, Y, X)) throw std::invalid_argument(GRID_MISMATCH);
    size_t ty, tx;
    vec t = flatten(threshold, ty, tx);
    if(!((cells(ogrid) == 0 && t.empty()) || fits(ogrid, ty, tx))) throw std::invalid_argument("Grid size is not the same as threshold");
    if(igrid.get_coordinate_type() != ogrid.get_coordinate_type()) throw std::invalid_argument("Coordinate types must be the same");
    if(op != Lt && op != Leq && op != Gt && op != Geq) throw std::invalid_argument("Invalid comparison operator");
    return t;
}
inline vec2 mask_threshold_downscale(const Grid& igrid, const Grid& ogrid, const vec3& ivalues_true, const vec3& ivalues_false,
                                     const vec3& threshold_values, const vec2& threshold, ComparisonOperator op, Statistic statistic, float quantile) {
    size_t Y, X, E, y2, x2, e2, y3, x3, e3;
    vec vt = flatten(ivalues_true, Y, X, E), vf = flatten(ivalues_false, y2, x2, e2), tv = flatten(threshold_values, y3, x3, e3);
    if(y2 != Y || x2 != X || e2 != E || y3 != Y || x3 != X || e3 != E)
        throw std::invalid_argument("ivalues_true, ivalues_false and threshold_values must have the same shape");
    vec t = ensemble_checks(igrid, ogrid, Y, X, threshold, op);
    size_t oy = ogrid.size()[0], ox = ogrid.size()[1];
    vec out(oy * ox, MV);
    check(gpp_mask_threshold_downscale(igrid.handle(), ogrid.handle(), vt.data(), vf.data(), tv.data(), (int)E, t.data(), (int)op, (int)statistic,
                                       quantile, out.data(), GPP_MEM_HOST));
    return unflatten(out, oy, ox);
}
}   // namespace detail
// src/api/downscale_probability.cpp:7-67
inline vec2 downscale_probability(const Grid& igrid, const Grid& ogrid, const vec3& ivalues, const vec2& threshold,
                                  const ComparisonOperator& comparison_operator) {
    size_t Y, X, E;
    vec v = detail::flatten(ivalues, Y, X, E);
    vec t = detail::ensemble_checks(igrid, ogrid, Y, X, threshold, comparison_operator);
    size_t oy = ogrid.size()[0], ox = ogrid.size()[1];
    vec out(oy * ox, MV);
    detail::check(gpp_downscale_probability(igrid.handle(), ogrid.handle(), v.data(), (int)E, t.data(), (int)comparison_operator, out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, oy, ox);
}
// src/api/mask_threshold_downscale_consensus.cpp:12-82
inline vec2 mask_threshold_downscale_consensus(const Grid& igrid, const Grid& ogrid, const vec3& ivalues_true, const vec3& ivalues_false,
                                               const vec3& threshold_values, const vec2& threshold, const ComparisonOperator& comparison_operator,
                                               const Statistic& statistic) {
    return detail::mask_threshold_downscale(igrid, ogrid, ivalues_true, ivalues_false, threshold_values, threshold, comparison_operator, statistic, 0);
}
inline vec2 mask_threshold_downscale_quantile(const Grid& igrid, const Grid& ogrid, const vec3& ivalues_true, const vec3& ivalues_false,
                                              const vec3& threshold_values, const vec2& threshold, const ComparisonOperator& comparison_operator,
                                              const float quantile_level) {
    return detail::mask_threshold_downscale(igrid, ogrid, ivalues_true, ivalues_false, threshold_values, threshold, comparison_operator, Quantile,
                                            quantile_level);
}
// src/api/smart.cpp:12-66
inline vec2 smart(const Grid& igrid, const Grid& ogrid, const vec2& ivalues, int num, const StructureFunction& structure) {
    size_t Y, X;
    vec v = detail::flatten(ivalues, Y, X);
    if(detail::cells(igrid) && !detail::fits(igrid, Y, X)) throw std::invalid_argument(detail::GRID_MISMATCH);
    if(igrid.get_coordinate_type() != ogrid.get_coordinate_type()) throw std::invalid_argument("Coordinate types must be the same");
    size_t oy = ogrid.size()[0], ox = ogrid.size()[1];
    vec out(oy * ox, MV);
    detail::check(gpp_smart(igrid.handle(), ogrid.handle(), v.data(), num, structure.c_struct(), out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, oy, ox);
}

// ---- local_distribution_correction (include/gridpp.h:467-512) ----------------------------------------------------------------
// src/api/local_distribution_correction.cpp:33-203.  Ties in value are ordered by rho ascending (the reference leaves them to an
// unstable sort); shapes the reference would read out of bounds with are refused.
inline vec2 local_distribution_correction(const Grid& bgrid, const vec2& background, const Points& points, const vec2& pobs, const vec2& pbackground,
                                          const StructureFunction& structure, float min_quantile, float max_quantile, int min_points = 0) {
    size_t Y, X, T, S, T2, S2;
    vec b = detail::flatten(background, Y, X), po = detail::flatten(pobs, T, S), pb = detail::flatten(pbackground, T2, S2);
    if(pobs.size() != pbackground.size()) {   // :50-54
        std::stringstream ss;
        ss << "pobs (" << pobs.size() << "," << S << ") is not the same size as pbackground (" << pbackground.size() << "," << S2 << ")";
        throw std::invalid_argument(ss.str());
    }
    if(S != S2 || po.size() != pb.size()) {
        std::stringstream ss;
        ss << "pobs (" << pobs.size() << "," << S << ") is not the same shape as pbackground (" << pbackground.size() << "," << S2 << ")";
        throw std::invalid_argument(ss.str());
    }
    if(!((detail::cells(bgrid) == 0 && b.empty()) || detail::fits(bgrid, Y, X))) throw std::invalid_argument(detail::GRID_MISMATCH);
    if(!pobs.empty() && S != (size_t)points.size()) {
        std::stringstream ss;
        ss << "pobs (" << S << ") and points (" << points.size() << ") size mismatch";
        throw std::invalid_argument(ss.str());
    }
    if(bgrid.get_coordinate_type() != points.get_coordinate_type())
        throw std::invalid_argument("Both background grid and observations points must be of same coordinate type (lat/lon or x/y)");
    if(!(std::isfinite(min_quantile) && std::isfinite(max_quantile) && 0 <= min_quantile && min_quantile <= max_quantile && max_quantile <= 1))
        throw std::invalid_argument("min_quantile and max_quantile must be finite with 0 <= min_quantile <= max_quantile <= 1");
    size_t oy = bgrid.size()[0], ox = bgrid.size()[1];
    vec out(oy * ox, MV);
    detail::check(gpp_local_distribution_correction(bgrid.handle(), b.data(), points.handle(), po.data(), pb.data(), (int)pobs.size(),
                                                    structure.c_struct(), min_quantile, max_quantile, min_points, out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, oy, ox);
}
// :18-32
inline vec2 local_distribution_correction(const Grid& bgrid, const vec2& background, const Points& points, const vec& pobs, const vec& pbackground,
                                          const StructureFunction& structure, float min_quantile, float max_quantile, int min_points = 0) {
    return local_distribution_correction(bgrid, background, points, vec2(1, pobs), vec2(1, pbackground), structure, min_quantile, max_quantile,
                                         min_points);
}

// ---- calibration by a curve (include/gridpp.h:79-85,731-789,1549-1557) ---------------------------------------------------
// src/api/curve.cpp:6-77 (host only; the reference's lazy policy check)
inline float apply_curve(float input, const vec& curve_ref, const vec& curve_fcst, Extrapolation policy_below, Extrapolation policy_above) {
    float out = MV;
    detail::check(gpp_apply_curve_scalar(input, curve_ref.data(), (int)curve_ref.size(), curve_fcst.data(), (int)curve_fcst.size(), (int)policy_below,
                                         (int)policy_above, &out));
    return out;
}
// src/api/curve.cpp:79-94.  The array forms refuse an unknown policy whatever the data.
inline vec apply_curve(const vec& fcst, const vec& curve_ref, const vec& curve_fcst, Extrapolation policy_below, Extrapolation policy_above) {
    vec out(fcst.size(), MV);
    detail::check(gpp_apply_curve(fcst.data(), (long long)fcst.size(), curve_ref.data(), (int)curve_ref.size(), curve_fcst.data(), (int)curve_fcst.size(),
                                  (int)policy_below, (int)policy_above, out.data(), GPP_MEM_HOST));
    return out;
}
// src/api/curve.cpp:96-108 (rows may differ in length there; each row is one vector call, as in the reference)
inline vec2 apply_curve(const vec2& fcst, const vec& curve_ref, const vec& curve_fcst, Extrapolation policy_below, Extrapolation policy_above) {
    vec flat;
    for(const auto& r : fcst) flat.insert(flat.end(), r.begin(), r.end());
    vec out = apply_curve(flat, curve_ref, curve_fcst, policy_below, policy_above);
    vec2 o(fcst.size());
    size_t at = 0;
    for(size_t y = 0; y < fcst.size(); y++) { o[y].assign(out.begin() + at, out.begin() + at + fcst[y].size()); at += fcst[y].size(); }
    return o;
}
// src/api/curve.cpp:110-133: one curve per cell, curves (Y, X, C)
inline vec2 apply_curve(const vec2& fcst, const vec3& curve_ref, const vec3& curve_fcst, Extrapolation policy_below, Extrapolation policy_above) {
    size_t Y, X, yr, xr, cr, yf, xf, cf;
    vec v = detail::flatten(fcst, Y, X), r = detail::flatten(curve_ref, yr, xr, cr), f = detail::flatten(curve_fcst, yf, xf, cf);
    if(yr != yf || xr != xf || cr != cf) throw std::invalid_argument("curve_ref and curve_fcst dimension sizes mismatch");
    if(Y != yr || X != xr) throw std::invalid_argument("Fcst and curve_ref dimension sizes mismatch");
    vec out(Y * X, MV);
    detail::check(gpp_apply_curve_field(v.data(), r.data(), f.data(), (int)Y, (int)X, (int)cr, (int)cf, (int)policy_below, (int)policy_above, out.data(),
                                        GPP_MEM_HOST));
    return detail::unflatten(out, Y, X);
}
// src/api/util.cpp:377-426
inline float interpolate(float x, const vec& iX, const vec& iY) {
    float out = MV;
    detail::check(gpp_interpolate_scalar(x, iX.data(), (int)iX.size(), iY.data(), (int)iY.size(), &out));
    return out;
}
inline vec interpolate(const vec& x, const vec& iX, const vec& iY) {
    vec out(x.size(), MV);
    detail::check(gpp_interpolate(x.data(), (long long)x.size(), iX.data(), (int)iX.size(), iY.data(), (int)iY.size(), out.data(), GPP_MEM_HOST));
    return out;
}
// src/api/quantile_mapping.cpp:5-46 (host only): returns curve_ref, output_fcst receives curve_fcst
inline vec quantile_mapping_curve(const vec& ref, const vec& fcst, vec& output_fcst, vec quantiles = vec()) {
    const size_t cap = std::max(std::max(ref.size(), fcst.size()), std::max(quantiles.size(), (size_t)1));
    vec out_ref(cap), out_fcst(cap);
    int count = 0;
    detail::check(gpp_quantile_mapping_curve(ref.data(), (int)ref.size(), fcst.data(), (int)fcst.size(), quantiles.data(), (int)quantiles.size(),
                                             out_ref.data(), out_fcst.data(), &count));
    out_ref.resize(count);
    out_fcst.resize(count);
    output_fcst = out_fcst;
    return out_ref;
}
// src/api/curve.cpp:134-250 (host only): returns curve_ref, output_fcst receives curve_fcst
inline vec monotonize_curve(vec curve_ref, vec curve_fcst, vec& output_fcst) {
    const size_t cap = std::max(std::max(curve_ref.size(), curve_fcst.size()), (size_t)1);
    vec out_ref(cap), out_fcst(cap);
    int count = 0;
    detail::check(gpp_monotonize_curve(curve_ref.data(), (int)curve_ref.size(), curve_fcst.data(), (int)curve_fcst.size(), out_ref.data(), out_fcst.data(),
                                       &count));
    out_ref.resize(count);
    out_fcst.resize(count);
    output_fcst = out_fcst;
    return out_ref;
}

// ---- window statistics along the time axis (include/gridpp.h:1602-1611) ------------------------------------------------
// src/api/window.cpp:6-156: array is (case, time).  std::invalid_argument for length <= 0 and, for a non-empty array, for an even
// length without `before`; std::runtime_error for Quantile / Unknown (thrown inside the reference's loop, here before device work).
inline vec2 window(const vec2& array, int length, Statistic statistic, bool before = false, bool keep_missing = false, bool missing_edges = true) {
    if(length <= 0) throw std::invalid_argument("Length variable must be > 0");
    size_t Y, T;
    vec a = detail::flatten(array, Y, T);
    if(Y == 0) return vec2();        // window.cpp:14-17
    if(T == 0) return vec2(Y);       // :19-22
    vec out(Y * T, MV);
    detail::check(gpp_window(a.data(), (long long)Y, (int)T, length, (int)statistic, before ? 1 : 0, keep_missing ? 1 : 0, missing_edges ? 1 : 0, out.data(),
                             GPP_MEM_HOST));
    return detail::unflatten(out, Y, T);
}

// ---- verification scores (src/api/metric_optimizer.cpp:185-244, src/api/neighbourhood_score.cpp:6-60) ---------------------------------
// calc_score of a contingency table: host arithmetic with the reference's promotions; std::invalid_argument("Unknown metric").
inline float calc_score(float a, float b, float c, float d, Metric metric) {
    float out = MV;
    detail::check(gpp_calc_score_table(a, b, c, d, (int)metric, &out));
    return out;
}
// the table of the first fcst.size() elements, counted on the GPU (nothing to count needs none).  A ref shorter than fcst is read out of
// bounds by the reference: std::invalid_argument here.
inline float calc_score(const vec& ref, const vec& fcst, float threshold, float fthreshold, Metric metric) {
    if(ref.size() < fcst.size()) throw std::invalid_argument("ref and fcst not the same size");
    float out = MV;
    detail::check(gpp_calc_score(ref.data(), fcst.data(), (long long)fcst.size(), threshold, fthreshold, (int)metric, &out, GPP_MEM_HOST));
    return out;
}
inline float calc_score(const vec& ref, const vec& fcst, float threshold, Metric metric) { return calc_score(ref, fcst, threshold, threshold, metric); }
// neighbourhood_score.cpp:6-60, the checks in its order (the last one is gridding_nearest's)
inline vec2 neighbourhood_score(const Grid& grid, const Points& points, const vec2& fcst, const vec& ref, int half_width, Metric metric, float threshold) {
    size_t Y, X;
    vec f = detail::flatten(fcst, Y, X);
    if(Y != 0 && !detail::fits(grid, Y, X)) throw std::invalid_argument("Grid size is not the same as forecast values");
    if(half_width <= 0) throw std::invalid_argument("half_width must be greater than 0");
    calc_score(0, 0, 0, 0, metric);
    if((int)ref.size() != points.size()) throw std::invalid_argument("Points size is not the same as values");
    if(detail::cells(grid) == 0) return vec2(grid.size()[0]);
    if(Y == 0) throw std::invalid_argument("Grid size is not the same as forecast values");   // (the reference reads fcst[0] of an empty vector here)
    vec out(Y * X, MV);
    detail::check(gpp_neighbourhood_score(grid.handle(), points.handle(), f.data(), ref.data(), half_width, (int)metric, threshold, out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, Y, X);
}

// ---- weather diagnostics (include/gridpp.h:1249-1367) -----------------------------------------------------------------------------
// The scalar overloads are host arithmetic (the per-value source of the kernels); the vector overloads run one kernel over host buffers.
// std::invalid_argument with the reference's texts for vectors of different sizes; sea_level_pressure throws std::runtime_error as
// pressure.cpp:32-38 does (the vector overload for the lowest offending index).
namespace detail {
inline float diagnostic(int which, std::initializer_list<float> args) {
    float out = MV;
    check(gpp_diagnostic_scalar(which, args.begin(), (int)args.size(), &out));
    return out;
}
}   // namespace detail
inline float dewpoint(float temperature, float relative_humidity) { return detail::diagnostic(GPP_DIAG_DEWPOINT, {temperature, relative_humidity}); }
inline vec dewpoint(const vec& temperature, const vec& relative_humidity) {
    if(temperature.size() != relative_humidity.size()) throw std::invalid_argument("Temperature and relative_humidity vectors are not the same size");
    vec out(temperature.size(), MV);
    detail::check(gpp_dewpoint(temperature.data(), relative_humidity.data(), (long long)out.size(), out.data(), GPP_MEM_HOST));
    return out;
}
inline float relative_humidity(float temperature, float dewpoint) { return detail::diagnostic(GPP_DIAG_RELATIVE_HUMIDITY, {temperature, dewpoint}); }
inline vec relative_humidity(const vec& temperature, const vec& dewpoint) {
    if(temperature.size() != dewpoint.size()) throw std::invalid_argument("Temperature and dewpoint vectors are not the same size");
    vec out(temperature.size(), MV);
    detail::check(gpp_relative_humidity(temperature.data(), dewpoint.data(), (long long)out.size(), out.data(), GPP_MEM_HOST));
    return out;
}
inline float wetbulb(float temperature, float pressure, float relative_humidity) {
    return detail::diagnostic(GPP_DIAG_WETBULB, {temperature, pressure, relative_humidity});
}
inline vec wetbulb(const vec& temperature, const vec& pressure, const vec& relative_humidity) {
    if(temperature.size() != pressure.size()) throw std::invalid_argument("Temperature and pressure vectors are not the same size");
    if(temperature.size() != relative_humidity.size()) throw std::invalid_argument("Temperature and relative_humidity vectors are not the same size");
    vec out(temperature.size(), MV);
    detail::check(gpp_wetbulb(temperature.data(), pressure.data(), relative_humidity.data(), (long long)out.size(), out.data(), GPP_MEM_HOST));
    return out;
}
inline float pressure(float ielev, float oelev, float ipressure, float itemperature = 288.15) {
    return detail::diagnostic(GPP_DIAG_PRESSURE, {ielev, oelev, ipressure, itemperature});
}
inline vec pressure(const vec& ielev, const vec& oelev, const vec& ipressure, const vec& itemperature) {
    const size_t N = ielev.size();
    if(oelev.size() != N || ipressure.size() != N || itemperature.size() != N) throw std::invalid_argument("pressure: Input arguments must be of the same size");
    vec out(N, MV);
    detail::check(gpp_pressure(ielev.data(), oelev.data(), ipressure.data(), itemperature.data(), (long long)N, out.data(), GPP_MEM_HOST));
    return out;
}
inline float sea_level_pressure(float ps, float altitude, float temperature, float rh = MV, float dewpoint = MV) {
    return detail::diagnostic(GPP_DIAG_SEA_LEVEL_PRESSURE, {ps, altitude, temperature, rh, dewpoint});
}
inline vec sea_level_pressure(const vec& ps, const vec& altitude, const vec& temperature, const vec& rh, const vec& dewpoint) {
    const size_t N = ps.size();
    if(altitude.size() != N || temperature.size() != N || rh.size() != N || dewpoint.size() != N)
        throw std::invalid_argument("slp: Input arguments must be of the same size");
    vec out(N, MV);
    detail::check(gpp_sea_level_pressure(ps.data(), altitude.data(), temperature.data(), rh.data(), dewpoint.data(), (long long)N, out.data(), GPP_MEM_HOST));
    return out;
}
inline float qnh(float pressure, float altitude) { return detail::diagnostic(GPP_DIAG_QNH, {pressure, altitude}); }
inline vec qnh(const vec& pressure, const vec& altitude) {
    if(pressure.size() != altitude.size()) throw std::invalid_argument("Pressure and altitude vectors are not the same size");
    vec out(pressure.size(), MV);
    detail::check(gpp_qnh(pressure.data(), altitude.data(), (long long)out.size(), out.data(), GPP_MEM_HOST));
    return out;
}
inline float wind_speed(float xwind, float ywind) { return detail::diagnostic(GPP_DIAG_WIND_SPEED, {xwind, ywind}); }
inline vec wind_speed(const vec& xwind, const vec& ywind) {
    if(xwind.size() != ywind.size()) throw std::invalid_argument("xwind and ywind must be of the same size");
    vec out(xwind.size(), MV);
    detail::check(gpp_wind_speed(xwind.data(), ywind.data(), (long long)out.size(), out.data(), GPP_MEM_HOST));
    return out;
}
inline float wind_direction(float xwind, float ywind) { return detail::diagnostic(GPP_DIAG_WIND_DIRECTION, {xwind, ywind}); }
inline vec wind_direction(const vec& xwind, const vec& ywind) {
    if(xwind.size() != ywind.size()) throw std::invalid_argument("xwind and ywind must be of the same size");
    vec out(xwind.size(), MV);
    detail::check(gpp_wind_direction(xwind.data(), ywind.data(), (long long)out.size(), out.data(), GPP_MEM_HOST));
    return out;
}

// ---- value transforms (include/gridpp.h:2345-2435, src/api/transform.cpp) -----------------------------------------------------------
// The scalar forms are host arithmetic; the vec / vec2 / vec3 forms flatten their input (rows may differ in length, as in the
// reference's loops), run one kernel and restore the nesting.  The base class's scalar forms return -1 (transform.cpp:7-12), and so
// do its vector forms element by element.
class Transform {
    public:
        Transform() : m_kind(-1), m_p0(0), m_p1(0) {}
        virtual ~Transform() {}
        virtual float forward(float value) const { return scalar(value, 0); }
        virtual float backward(float value) const { return scalar(value, 1); }
        vec forward(const vec& input) const { return apply(input, 0); }
        vec backward(const vec& input) const { return apply(input, 1); }
        vec2 forward(const vec2& input) const { return apply(input, 0); }
        vec2 backward(const vec2& input) const { return apply(input, 1); }
        vec3 forward(const vec3& input) const { return apply(input, 0); }
        vec3 backward(const vec3& input) const { return apply(input, 1); }
    protected:
        Transform(int kind, float p0, float p1 = 0) : m_kind(kind), m_p0(p0), m_p1(p1) {}
        // the one kernel call behind the six vector forms: a transform defined outside this header overrides it (and the scalar forms)
        virtual vec apply(const vec& input, int backward) const {
            vec out(input.size(), MV);
            if(m_kind < 0) std::fill(out.begin(), out.end(), -1.0f);
            else detail::check(gpp_transform(input.data(), (long long)input.size(), m_kind, backward, m_p0, m_p1, out.data(), GPP_MEM_HOST));
            return out;
        }
    private:
        int m_kind;   // GPP_TRANSFORM_*, -1: the base class
        float m_p0, m_p1;
        float scalar(float value, int backward) const {
            if(m_kind < 0) return -1;
            float out = MV;
            detail::check(gpp_transform_scalar(value, m_kind, backward, m_p0, m_p1, &out));
            return out;
        }
        vec2 apply(const vec2& input, int backward) const {
            vec flat;
            for(const auto& r : input) flat.insert(flat.end(), r.begin(), r.end());
            const vec out = apply(flat, backward);
            vec2 o(input.size());
            size_t at = 0;
            for(size_t y = 0; y < input.size(); y++) { o[y].assign(out.begin() + at, out.begin() + at + input[y].size()); at += input[y].size(); }
            return o;
        }
        vec3 apply(const vec3& input, int backward) const {
            vec flat;
            for(const auto& r : input) for(const auto& c : r) flat.insert(flat.end(), c.begin(), c.end());
            const vec out = apply(flat, backward);
            vec3 o(input.size());
            size_t at = 0;
            for(size_t y = 0; y < input.size(); y++) {
                o[y].resize(input[y].size());
                for(size_t x = 0; x < input[y].size(); x++) { o[y][x].assign(out.begin() + at, out.begin() + at + input[y][x].size()); at += input[y][x].size(); }
            }
            return o;
        }
};
class Identity : public Transform {
    public:
        Identity() : Transform(GPP_TRANSFORM_IDENTITY, 0) {}
        using Transform::forward;
        using Transform::backward;
};
class Log : public Transform {
    public:
        Log() : Transform(GPP_TRANSFORM_LOG, 0) {}
        using Transform::forward;
        using Transform::backward;
};
class BoxCox : public Transform {
    public:
        BoxCox(float threshold) : Transform(GPP_TRANSFORM_BOXCOX, threshold) {}   // transform.cpp:97-99: no validation
        using Transform::forward;
        using Transform::backward;
};
class StartedBoxCox : public Transform {
    public:
        StartedBoxCox(float threshold, float scaling_factor) : Transform(GPP_TRANSFORM_STARTED_BOXCOX, threshold, scaling_factor) {   // transform.cpp:126-132
            if(!is_valid(threshold) || threshold <= 0) throw std::invalid_argument("threshold parameter must be > 0 in the started Box-Cox distribution");
            if(!is_valid(scaling_factor) || scaling_factor <= 0)
                throw std::invalid_argument("Scaling factor parameter must be > 0 in the started Box-Cox distribution");
        }
        using Transform::forward;
        using Transform::backward;
};

// ---- util (include/gridpp.h:1454-1482) -----------------------------------------------------------------------------
inline float calc_statistic(const vec& array, Statistic statistic) {
    float out = MV;
    detail::check(gpp_calc_statistic(array.data(), 1, (int)array.size(), (int)statistic, &out, GPP_MEM_HOST));
    return out;
}
inline float calc_quantile(const vec& array, float quantile) {
    float out = MV;
    detail::check(gpp_calc_quantile(array.data(), 1, (int)array.size(), &quantile, 1, &out, GPP_MEM_HOST));
    return out;
}
namespace detail {
// The rows of the reference's vec2 may differ in length: each is padded with NaN to the longest.  Every statistic skips invalid
// values, so the results are the reference's; an empty row gives what an empty vec gives.
inline vec pad_rows(const vec2& a, size_t& len) {
    len = 0;
    for(const auto& r : a) len = std::max(len, r.size());
    vec f(a.size() * len, MV);
    for(size_t n = 0; n < a.size(); n++) std::copy(a[n].begin(), a[n].end(), f.begin() + n * len);
    return f;
}
}   // namespace detail
inline vec calc_statistic(const vec2& array, Statistic statistic) {   // util.cpp:209-216
    size_t len;
    const vec f = detail::pad_rows(array, len);
    vec out(array.size(), MV);
    detail::check(gpp_calc_statistic(f.data(), (long)array.size(), (int)len, (int)statistic, out.data(), GPP_MEM_HOST));
    return out;
}
inline vec calc_quantile(const vec2& array, float quantile = MV) {   // util.cpp:179-186
    size_t len;
    const vec f = detail::pad_rows(array, len);
    vec out(array.size(), MV);
    detail::check(gpp_calc_quantile(f.data(), (long)array.size(), (int)len, &quantile, 1, out.data(), GPP_MEM_HOST));
    return out;
}
inline vec2 calc_quantile(const vec3& array, const vec2& quantile) {   // util.cpp:187-208
    if(quantile.size() != array.size() || (array.size() && quantile[0].size() != array[0].size()))   // compatible_size(vec2, vec3), util.cpp:448-461
        throw std::invalid_argument("Dimension mismatch between array and quantile");
    size_t Y, X, E, qy, qx;
    const vec f = detail::flatten(array, Y, X, E);
    if(Y == 0 || X == 0) return vec2();
    if(E == 0) return vec2(Y, vec(X, MV));
    const vec q = detail::flatten(quantile, qy, qx);
    vec out(Y * X, MV);
    detail::check(gpp_calc_quantile(f.data(), (long)(Y * X), (int)E, q.data(), (long)(Y * X), out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, Y, X);
}
}   // namespace gridpp
