// gridpp.hpp -- C++ host mirror of the reference's public API (include/gridpp.h) for the hot path only,
// header-only over the C-ABI of libgridpp_hip.so (include/gridpp_hip.h).
//
// Same namespace, type names, signatures, defaults and exception types as the reference, so code written
// against gridpp.h for this path compiles unchanged:
//   vec/vec2/vec3/ivec/ivec2/ivec3             include/gridpp.h:25-41
//   Statistic, CoordinateType, MV              :49,88-100,120-123
//   Point (both constructors)                  :1713-1743
//   KDTree (queries, getters, the static distance helpers)  :1746-1873
//     (one addition: calc_distance_fast(const Point&, const Point&), which the reference does not declare)
//   Points, Grid (every public member)         :1876-2060
//   StructureFunction (corr / corr_background for one point and for a vector, localization_distance, clone,
//     default_min_rho), StructureFunctionPtr   :2067-2105
//   Barnes / Soar / Toar / Powerlaw / Linear structures (scalar and spatially varying forms), CressmanStructure,
//     MultipleStructure, CrossValidation       :2107-2343
//   staticcorr_points                          :462
//   convert_coordinates (both overloads), is_valid_lat, is_valid_lon, num_missing_values  :1492-1522
//   init_vec2 / init_ivec2 / init_vec3 / init_ivec3, compatible_size (all seven overloads)  :1565-1660
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
#include <mutex>
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
typedef std::vector<ivec2> ivec3;
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
// A point set in HBM, shared by every copy of the KDTree / Points / Grid that made it.  The set never changes, so the host copy of a
// field (0 lat, 1 lon, 2 elev, 3 laf, 4 x, 5 y, 6 z) is fetched once, the first time a getter asks for it, and kept.
struct Handle {
    gpp_points* p = nullptr;
    ~Handle() { if(p) gpp_points_destroy(p); }
    const vec& field(int k, size_t n) {
        std::lock_guard<std::mutex> lock(m);
        if(!have[k]) {
            host[k].resize(n);
            check(gpp_points_get(p, k, host[k].data()));
            have[k] = true;
        }
        return host[k];
    }
  private:
    std::mutex m;
    vec host[7];
    bool have[7] = {false, false, false, false, false, false, false};
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

// ---- coordinates, Point (include/gridpp.h:1492-1516,1713-1743) ----------------------------------------------------
inline bool is_valid_lat(float lat, CoordinateType type) {   // src/api/util.cpp:617-621: a Cartesian y is any valid value
    if(type == Cartesian) return is_valid(lat);
    return is_valid(lat) && (lat >= -90.001) && (lat <= 90.001);
}
inline bool is_valid_lon(float lon, CoordinateType) { return is_valid(lon); }   // util.cpp:622-624
// util.cpp:583-615; GPP_EINVAL "Invalid coords" -> std::invalid_argument
inline bool convert_coordinates(const vec& lats, const vec& lons, CoordinateType type, vec& x_coords, vec& y_coords, vec& z_coords) {
    const size_t N = lats.size();
    if(lons.size() != N) throw std::invalid_argument("lats and lons must have the same size");
    x_coords.resize(N); y_coords.resize(N); z_coords.resize(N);
    if(N) detail::check(gpp_convert_coordinates(lats.data(), lons.data(), (int)N, (int)type, x_coords.data(), y_coords.data(), z_coords.data()));
    return true;
}
inline bool convert_coordinates(float lat, float lon, CoordinateType type, float& x_coord, float& y_coord, float& z_coord) {
    detail::check(gpp_convert_coordinates(&lat, &lon, 1, (int)type, &x_coord, &y_coord, &z_coord));
    return true;
}
class Point {   // src/api/point.cpp:5-26
  public:
    Point(float lat, float lon, float elev = MV, float laf = MV, CoordinateType type = Geodetic) : lat(lat), lon(lon), elev(elev), laf(laf), type(type) {
        if(type == Geodetic) convert_coordinates(lat, lon, type, x, y, z);
        else { x = lat; y = lon; z = 0; }
    }
    Point(float lat, float lon, float elev, float laf, CoordinateType type, float x, float y, float z)
        : lat(lat), lon(lon), elev(elev), laf(laf), type(type), x(x), y(y), z(z) {}
    float lat, lon, elev, laf;
    CoordinateType type;
    float x, y, z;
};
namespace detail {
// the C-ABI's record of a point: x, y, z, elev, laf, lat, lon
struct Seven { float f[7]; explicit Seven(const Point& p) : f{p.x, p.y, p.z, p.elev, p.laf, p.lat, p.lon} {} };
}

// ---- KDTree / Points / Grid (include/gridpp.h:1746-2060) ----------------------------------------------------------
class Grid;
class KDTree {
  public:
    KDTree(vec lats, vec lons, CoordinateType type = Geodetic) : KDTree(lats, lons, vec(), vec(), type) {}
    KDTree(CoordinateType type = Geodetic) : KDTree(vec(), vec(), vec(), vec(), type) {}
    int size() const { return mN; }
    CoordinateType get_coordinate_type() const { return mType; }
    vec get_lats() const { return field(0); }
    vec get_lons() const { return field(1); }
    const vec& get_x() const { return field(4); }
    const vec& get_y() const { return field(5); }
    const vec& get_z() const { return field(6); }
    ivec get_neighbours(float lat, float lon, float radius, bool include_match = true) const {
        ivec idx(mN > 0 ? mN : 1); int count = 0;
        detail::check(gpp_points_get_neighbours(mH->p, lat, lon, radius, include_match, idx.data(), nullptr, (int)idx.size(), &count));
        idx.resize(count);
        return idx;
    }
    ivec get_neighbours_with_distance(float lat, float lon, float radius, vec& distances, bool include_match = true) const {
        ivec idx(mN > 0 ? mN : 1); int count = 0;
        distances.assign(idx.size(), 0);
        detail::check(gpp_points_get_neighbours(mH->p, lat, lon, radius, include_match, idx.data(), distances.data(), (int)idx.size(), &count));
        idx.resize(count); distances.resize(count);
        return idx;
    }
    int get_num_neighbours(float lat, float lon, float radius, bool include_match = true) const { return (int)get_neighbours(lat, lon, radius, include_match).size(); }
    ivec get_closest_neighbours(float lat, float lon, int num, bool include_match = true) const {
        ivec idx(num > 0 ? num : 1); int count = 0;
        detail::check(gpp_points_get_closest_neighbours(mH->p, lat, lon, num, include_match, idx.data(), &count));
        idx.resize(count);
        return idx;
    }
    int get_nearest_neighbour(float lat, float lon, bool include_match = true) const {
        int i = -1;
        detail::check(gpp_points_nearest_neighbour(mH->p, &lat, &lon, 1, include_match, &i));
        return i;
    }
    // src/api/kdtree.cpp:107-200, host scalar arithmetic: angles are rounded to float32 by deg2rad, the trigonometry is double
    static float deg2rad(float deg) { return (float)((double)deg * 3.14159265358979323846 / 180); }
    static float rad2deg(float rad) { return (float)((double)rad * 180 / 3.14159265358979323846); }
    static float calc_distance(float lat1, float lon1, float lat2, float lon2, CoordinateType type = Geodetic) {
        if(type == Cartesian) return planar(lat1, lon1, lat2, lon2);
        if(lat1 == lat2 && lon1 == lon2) return 0;
        const double la1 = deg2rad(lat1), la2 = deg2rad(lat2), lo1 = deg2rad(lon1), lo2 = deg2rad(lon2);
        const double ratio = std::cos(la1) * std::cos(lo1) * std::cos(la2) * std::cos(lo2) + std::cos(la1) * std::sin(lo1) * std::cos(la2) * std::sin(lo2)
                             + std::sin(la1) * std::sin(la2);
        return (float)(std::acos(ratio) * radius_earth);
    }
    static float calc_distance(const Point& p1, const Point& p2) {
        if(p1.type != p2.type) throw std::runtime_error("Coordinate types must be the same");
        return calc_distance(p1.lat, p1.lon, p2.lat, p2.lon, p1.type);
    }
    static float calc_distance_fast(float lat1, float lon1, float lat2, float lon2, CoordinateType type = Geodetic) {
        if(type == Cartesian) return planar(lat1, lon1, lat2, lon2);
        const double two_pi = 2 * 3.14159265358979323846;
        const double la1 = deg2rad(lat1), la2 = deg2rad(lat2), lo1 = deg2rad(lon1), lo2 = deg2rad(lon2);
        double dlon = std::fmod(std::fabs(lo1 - lo2), two_pi);
        if(dlon > two_pi / 2) dlon = two_pi - dlon;   // the longitudes wrap
        const double c = std::cos(std::fabs(la2) > std::fabs(la1) ? la2 : la1);
        const float dx2 = (float)(c * c * dlon * dlon), dy2 = (float)((la1 - la2) * (la1 - la2));
        return (float)(radius_earth * std::sqrt((double)(dx2 + dy2)));
    }
    // (an addition: the reference declares only the float form, gridpp.h:1836; the python mirror has this one too)
    static float calc_distance_fast(const Point& p1, const Point& p2) {
        if(p1.type != p2.type) throw std::runtime_error("Coordinate types must be the same");
        return calc_distance_fast(p1.lat, p1.lon, p2.lat, p2.lon, p1.type);
    }
    static float calc_straight_distance(float x0, float y0, float z0, float x1, float y1, float z1) {
        return std::sqrt((x0 - x1) * (x0 - x1) + (y0 - y1) * (y0 - y1) + (z0 - z1) * (z0 - z1));
    }
    static float calc_straight_distance(const Point& p1, const Point& p2) { return calc_straight_distance(p1.x, p1.y, p1.z, p2.x, p2.y, p2.z); }
    gpp_points* handle() const { return mH->p; }
  protected:
    KDTree(const vec& lats, const vec& lons, const vec& elevs, const vec& lafs, CoordinateType type) : mType(type) {
        size_t N = lats.size();
        if(lons.size() != N) throw std::invalid_argument("Cannot create points with unequal lat and lon sizes");
        if(elevs.size() != 0 && elevs.size() != N) throw std::invalid_argument("'elevs' must either be size 0 or the same size at lats/lons");
        if(lafs.size() != 0 && lafs.size() != N) throw std::invalid_argument("'lafs' must either be size 0 or the same size at lats/lons");
        mH = std::make_shared<detail::Handle>();
        detail::check(gpp_points_create(lats.data(), lons.data(), elevs.size() == N && N ? elevs.data() : nullptr,
                                        lafs.size() == N && N ? lafs.data() : nullptr, (int)N, (int)type, &mH->p));
        mN = (int)N;
    }
    static float planar(float lat1, float lon1, float lat2, float lon2) { const float dx = lon1 - lon2, dy = lat1 - lat2; return std::sqrt(dx * dx + dy * dy); }
    const vec& field(int k) const { return mH->field(k, mN); }
    std::shared_ptr<detail::Handle> mH;
    int mN = 0;
    CoordinateType mType = Geodetic;
};

class Points : public KDTree {   // a KDTree with elevations and land-area fractions (the reference's Points holds one: src/api/points.cpp)
  public:
    Points() : Points(vec(), vec()) {}
    Points(vec lats, vec lons, vec elevs = vec(), vec lafs = vec(), CoordinateType type = Geodetic) : KDTree(lats, lons, elevs, lafs, type) {}
    Points(KDTree tree, vec elevs = vec(), vec lafs = vec()) : KDTree(tree.get_lats(), tree.get_lons(), elevs, lafs, tree.get_coordinate_type()) {}
    vec get_elevs() const { return field(2); }
    vec get_lafs() const { return field(3); }
    Point get_point(int index) const {   // points.cpp:128-130
        float f[7];
        for(int k = 0; k < 7; k++) f[k] = field(k).at(index);   // (single elements of the kept host copies)
        return Point(f[0], f[1], f[2], f[3], mType, f[4], f[5], f[6]);
    }
    ivec get_in_domain_indices(const Grid& grid) const;   // points.cpp:77-92: the points some box of the grid encloses (Grid::get_box)
    Points get_in_domain(const Grid& grid) const { return subset(get_in_domain_indices(grid)); }   // :93-109 (default coordinate type, as there)
    Points subset(const ivec& indices) const {            // :131-150
        const vec &la = field(0), &lo = field(1), &el = field(2), &lf = field(3);
        const size_t N = indices.size();
        vec lats(N), lons(N), elevs(N), lafs(N);
        for(size_t i = 0; i < N; i++) {
            const int k = indices[i];
            if(k >= mN) throw std::invalid_argument("Index exceeds number of points");
            if(k < 0) throw std::invalid_argument("Index is negative");   // (the reference reads before its vectors here)
            lats[i] = la[k]; lons[i] = lo[k]; elevs[i] = el[k]; lafs[i] = lf[k];
        }
        return Points(lats, lons, elevs, lafs);
    }
};

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
    vec2 get_lats() const { return field2(0); }
    vec2 get_lons() const { return field2(1); }
    vec2 get_elevs() const { return field2(2); }
    vec2 get_lafs() const { return field2(3); }
    ivec get_nearest_neighbour(float lat, float lon, bool include_match = true) const {   // grid.cpp:76-82,108-114
        if(mY * mX == 0) return ivec();
        int i = -1;
        detail::check(gpp_points_nearest_neighbour(mH->p, &lat, &lon, 1, include_match, &i));
        return ivec{i / mX, i % mX};
    }
    // the radius and k-nearest queries of the flat set, each index as (y, x) (grid.cpp:56-75)
    ivec2 get_neighbours(float lat, float lon, float radius, bool include_match = true) const { return yx(flat_neighbours(lat, lon, radius, include_match, nullptr)); }
    ivec2 get_neighbours_with_distance(float lat, float lon, float radius, vec& distances, bool include_match = true) const {
        return yx(flat_neighbours(lat, lon, radius, include_match, &distances));
    }
    int get_num_neighbours(float lat, float lon, float radius, bool include_match = true) const { return (int)flat_neighbours(lat, lon, radius, include_match, nullptr).size(); }
    ivec2 get_closest_neighbours(float lat, float lon, int num, bool include_match = true) const {
        ivec idx(num > 0 ? num : 1); int count = 0;
        detail::check(gpp_points_get_closest_neighbours(mH->p, lat, lon, num, include_match, idx.data(), &count));
        idx.resize(count);
        return yx(idx);
    }
    bool get_box(float lat, float lon, int& Y1_out, int& X1_out, int& Y2_out, int& X2_out) const {   // grid.cpp:149-229
        int inside = 0, box[4] = {-1, -1, -1, -1};
        detail::check(gpp_grid_get_box(mH->p, &lat, &lon, 1, &inside, box));
        Y1_out = box[0]; X1_out = box[1]; Y2_out = box[2]; X2_out = box[3];
        return inside != 0;
    }
    Points to_points() const { return Points(field(0), field(1), field(2), field(3), mType); }   // grid.cpp:131-145
    Point get_point(int y_index, int x_index) const {   // grid.cpp:230-233
        const size_t i = (size_t)y_index * mX + x_index;
        float f[7];
        for(int k = 0; k < 7; k++) f[k] = field(k).at(i);
        return Point(f[0], f[1], f[2], f[3], mType, f[4], f[5], f[6]);
    }
    gpp_points* handle() const { return mH->p; }
  private:
    const vec& field(int k) const { return mH->field(k, (size_t)mY * mX); }
    vec2 field2(int k) const { return detail::unflatten(field(k), mY, mX); }
    ivec flat_neighbours(float lat, float lon, float radius, bool include_match, vec* distances) const {
        ivec idx(mY * mX > 0 ? mY * mX : 1); int count = 0;
        if(distances) distances->assign(idx.size(), 0);
        detail::check(gpp_points_get_neighbours(mH->p, lat, lon, radius, include_match, idx.data(), distances ? distances->data() : nullptr, (int)idx.size(), &count));
        idx.resize(count);
        if(distances) distances->resize(count);
        return idx;
    }
    ivec2 yx(const ivec& flat) const { ivec2 o(flat.size()); for(size_t i = 0; i < flat.size(); i++) o[i] = ivec{flat[i] / mX, flat[i] % mX}; return o; }
    std::shared_ptr<detail::Handle> mH;
    int mY = 0, mX = 0;
    CoordinateType mType = Geodetic;
};
inline ivec Points::get_in_domain_indices(const Grid& grid) const {
    ivec indices;
    if(mN == 0 || grid.size()[0] * grid.size()[1] == 0) return indices;
    const vec &lats = field(0), &lons = field(1);
    ivec inside(mN), boxes(4 * (size_t)mN);
    detail::check(gpp_grid_get_box(grid.handle(), lats.data(), lons.data(), mN, inside.data(), boxes.data()));
    for(int i = 0; i < mN; i++) if(inside[i]) indices.push_back(i);
    return indices;
}

// ---- structure functions (include/gridpp.h:2069-2343) -----------------------------------------------------------
namespace detail {
// the h, v, w fields of a spatially varying structure in HBM, and the grid they borrow: shared by every copy and clone of the structure
struct Field {
    Field(const Grid& g) : grid(g) {}
    ~Field() { if(f) gpp_field_destroy(f); }
    Field(const Field&) = delete;
    Field& operator=(const Field&) = delete;
    gpp_field* f = nullptr;
    Grid grid;
};
template <class T> struct MinRho { static const float default_min_rho; };   // (a static data member a header can define)
template <class T> const float MinRho<T>::default_min_rho = 0.0013f;        // structure.cpp:5
}
class StructureFunction;
typedef std::shared_ptr<StructureFunction> StructureFunctionPtr;
class StructureFunction : public detail::MinRho<void> {
  public:
    virtual ~StructureFunction() {}
    const gpp_structure* c_struct() const { return &mS; }
    float localization_distance() const { float d; detail::check(gpp_structure_localization_distance(&mS, 0.0f, 0.0f, &d)); return d; }
    float localization_distance(const Point& p) const { float d; detail::check(gpp_structure_localization_distance(&mS, p.lat, p.lon, &d)); return d; }
    float corr(const Point& p1, const Point& p2) const { return one(p1, p2, 0); }
    vec corr(const Point& p1, const std::vector<Point>& p2) const { return many(p1, p2, 0); }
    float corr_background(const Point& p1, const Point& p2) const { return one(p1, p2, 1); }
    vec corr_background(const Point& p1, const std::vector<Point>& p2) const { return many(p1, p2, 1); }
    // the descriptor and the shared fields are all a structure function holds: the copy is complete for every derived class
    StructureFunctionPtr clone() const { return StructureFunctionPtr(new StructureFunction(*this)); }
  protected:
    StructureFunction() { mS = gpp_structure(); }
    void init(int kind, float h, float v, float w, float hmax) {
        if(!is_valid(v) || v < 0) throw std::invalid_argument("v must be >= 0");
        if(!is_valid(w) || w < 0) throw std::invalid_argument("w must be >= 0");
        mS = gpp_structure();
        mS.kind = kind; mS.h = h; mS.v = v; mS.w = w;
        detail::check(gpp_structure_min_rho(kind, h, hmax, &mS.min_rho));
    }
    // (grid, h, v, w, min_rho), e.g. structure.cpp:168-184
    void init(int kind, const Grid& grid, const vec2& h, const vec2& v, const vec2& w, float min_rho) {
        size_t Yh, Xh, Yv, Xv, Yw, Xw;
        const vec fh = detail::flatten(h, Yh, Xh), fv = detail::flatten(v, Yv, Xv), fw = detail::flatten(w, Yw, Xw);
        mS = gpp_structure();
        mS.kind = kind; mS.min_rho = min_rho;
        if(Yh * Xh == 1 && Yv * Xv == 1 && Yw * Xw == 1) { mS.h = fh[0]; mS.v = fv[0]; mS.w = fw[0]; return; }   // not spatial (:174-176)
        const size_t Y = grid.size()[0], X = grid.size()[1];
        if(Yh != Y || Xh != X || Yv != Y || Xv != X || Yw != Y || Xw != X) throw std::invalid_argument("Grid size not the same as scale size");
        auto field = std::make_shared<detail::Field>(grid);
        detail::check(gpp_field_create(field->grid.handle(), fh.data(), fv.data(), fw.data(), kind, min_rho, &field->f));
        mS.field = field->f;
        mFields.push_back(field);
    }
    void share_fields(const StructureFunction& other) { mFields.insert(mFields.end(), other.mFields.begin(), other.mFields.end()); }
    gpp_structure mS;
    std::vector<std::shared_ptr<detail::Field> > mFields;   // what mS.field / field_v / field_w point into
  private:
    float one(const Point& p1, const Point& p2, int background) const {
        float rho;
        detail::check(gpp_structure_corr(&mS, detail::Seven(p1).f, detail::Seven(p2).f, background, &rho));
        return rho;
    }
    vec many(const Point& p1, const std::vector<Point>& p2, int background) const {   // one launch for the whole vector
        vec rec; rec.reserve(7 * p2.size());
        for(const Point& p : p2) { const detail::Seven s(p); rec.insert(rec.end(), s.f, s.f + 7); }
        vec rho(p2.size());
        detail::check(gpp_structure_corr_many(&mS, detail::Seven(p1).f, rec.data(), (long long)p2.size(), background, rho.data()));
        return rho;
    }
};
#define GPP_SPATIAL_STRUCTURE(Name, KIND)                                                                                           \
    class Name : public StructureFunction {                                                                                         \
      public:                                                                                                                       \
        Name(float h, float v = 0, float w = 0, float hmax = MV) { init(KIND, h, v, w, hmax); }                                      \
        Name(Grid grid, vec2 h, vec2 v, vec2 w, float min_rho = StructureFunction::default_min_rho) { init(KIND, grid, h, v, w, min_rho); } \
    }
GPP_SPATIAL_STRUCTURE(BarnesStructure, GPP_SK_BARNES);       // structure.cpp:143-184
GPP_SPATIAL_STRUCTURE(SoarStructure, GPP_SK_SOAR);           // :317-341
GPP_SPATIAL_STRUCTURE(ToarStructure, GPP_SK_TOAR);           // :467-491
GPP_SPATIAL_STRUCTURE(PowerlawStructure, GPP_SK_POWERLAW);   // :618-642
GPP_SPATIAL_STRUCTURE(LinearStructure, GPP_SK_LINEAR);       // :765-789
#undef GPP_SPATIAL_STRUCTURE
class CressmanStructure : public StructureFunction { public: CressmanStructure(float h, float v = 0, float w = 0) { init(GPP_SK_CRESSMAN, h, v, w, MV); } };
class MultipleStructure : public StructureFunction {   // src/api/structure.cpp:90-138
  public:
    MultipleStructure(const StructureFunction& sh, const StructureFunction& sv, const StructureFunction& sw) {
        const gpp_structure *h = sh.c_struct(), *v = sv.c_struct(), *w = sw.c_struct();
        mS = *h;
        mS.v = v->v; mS.w = w->w;
        mS.kind_v = (v->kind_v ? v->kind_v - 1 : v->kind) + 1;
        mS.kind_w = (w->kind_w ? w->kind_w - 1 : w->kind) + 1;
        if(h->field) { mS.loc = 0; mS.flags = 0; }   // the localization distance is the field's, at the first point
        else { mS.loc = sh.localization_distance(); mS.flags = GPP_ST_HAS_LOC; }
        mS.cv_dist = 0;
        // (a nested MultipleStructure contributes the field of its own vertical / laf component)
        mS.field = h->field; mS.field_v = v->kind_v ? v->field_v : v->field; mS.field_w = w->kind_w ? w->field_w : w->field;
        share_fields(sh); share_fields(sv); share_fields(sw);
    }
};
class CrossValidation : public StructureFunction {     // src/api/structure.cpp:910-944
  public:
    CrossValidation(const StructureFunction& structure, float dist) {
        if(!is_valid(dist) || dist < 0) throw std::invalid_argument("Invalid 'dist' in CrossValidation structure");
        mS = *structure.c_struct();
        mS.flags |= GPP_ST_CV;
        mS.cv_dist = dist;
        share_fields(structure);
    }
};

// ---- container helpers (include/gridpp.h:1509-1660; src/api/util.cpp:217-225,427-504) -----------------------------
inline int num_missing_values(const vec2& iArray) {
    int count = 0;
    for(const vec& row : iArray) for(float value : row) count += !is_valid(value);
    return count;
}
inline vec2 init_vec2(int Y, int X, float value = MV) { return vec2(Y, vec(X, value)); }
inline ivec2 init_ivec2(int Y, int X, int value) { return ivec2(Y, ivec(X, value)); }
inline vec3 init_vec3(int Y, int X, int E, float value = MV) { return vec3(Y, vec2(X, vec(E, value))); }
inline ivec3 init_ivec3(int Y, int X, int E, int value) { return ivec3(Y, ivec2(X, ivec(E, value))); }
inline bool compatible_size(const Grid& grid, const vec2& v) { return v.size() == 0 || (grid.size()[0] == (int)v.size() && grid.size()[1] == (int)v[0].size()); }
// (v is [T][Y][X]; a first level without rows passes, util.cpp:430-432)
inline bool compatible_size(const Grid& grid, const vec3& v) {
    return v.size() == 0 || v[0].size() == 0 || (grid.size()[0] == (int)v[0].size() && grid.size()[1] == (int)v[0][0].size());
}
inline bool compatible_size(const Points& points, const vec& v) { return points.size() == (int)v.size(); }
inline bool compatible_size(const Points& points, const vec2& v) { return v.size() == 0 || points.size() == (int)v[0].size(); }
inline bool compatible_size(const vec2& a, const vec2& b) {
    if(a.size() != b.size()) return false;
    for(size_t y = 0; y < a.size(); y++) if(a[y].size() != b[y].size()) return false;
    return true;
}
inline bool compatible_size(const vec2& a, const vec3& b) {   // the first two sizes only (util.cpp:448-461)
    if(a.size() != b.size()) return false;
    return a.size() == 0 || a[0].size() == b[0].size();
}
inline bool compatible_size(const vec3& a, const vec3& b) {
    if(a.size() != b.size()) return false;
    for(size_t t = 0; t < a.size(); t++) {
        if(a[t].size() != b[t].size()) return false;
        for(size_t y = 0; y < a[t].size(); y++) if(a[t][y].size() != b[t][y].size()) return false;
    }
    return true;
}
// include/gridpp.h:462, src/api/corr_points.cpp:26-131: (L, K) static correlations between a set of points and a set of knots
inline vec2 staticcorr_points(const Points& points, const Points& knots, const StructureFunction& structure, int max_points) {
    if(max_points < 0) throw std::invalid_argument("max_points must be >= 0");
    if(points.get_coordinate_type() != knots.get_coordinate_type())
        throw std::invalid_argument("Both background grid and observations points must be of same coordinate type (lat/lon or x/y)");
    const size_t L = points.size(), K = knots.size();
    vec out(L * K);
    if(!out.empty()) detail::check(gpp_staticcorr_points(points.handle(), knots.handle(), structure.c_struct(), max_points, out.data(), GPP_MEM_HOST));
    return detail::unflatten(out, L, K);
}

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
