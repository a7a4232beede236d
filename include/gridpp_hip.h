/*
 * gridpp_hip.h -- C-ABI of the MI355X-native gridpp hot path (libgridpp_hip.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, int status codes, no
 * C++ / torch types.  Each entry point names the reference interface it
 * replaces (paths relative to the metno/gridpp repository root).  The C++ host
 * mirror (gridpp_amd/host/gridpp.hpp) and the Python mirror (gridpp_amd/)
 * both bind exactly these symbols; INTEGRATION.md shows the binding a gridpp
 * maintainer would add.
 *
 * Conventions
 *  - every function returns GPP_OK or a negative error code; the message of the
 *    last error on the calling thread is gpp_last_error().
 *      GPP_EINVAL   -> std::invalid_argument / Python ValueError
 *      GPP_ERUNTIME -> std::runtime_error    / Python RuntimeError
 *  - `mem` says where the caller's field arrays live: GPP_MEM_HOST (the library
 *    stages them through HBM) or GPP_MEM_DEVICE (pointers are HBM addresses of
 *    the current device, e.g. torch tensor .data_ptr(); nothing is copied).
 *    Coordinate arrays given to the *_create functions are always host arrays.
 *  - 2-D fields are row-major [Y][X]; 3-D fields are [Y][X][E] with E fastest
 *    (swig/vector.i:385-390).
 *  - the library keeps its scratch buffers and its stream per process: calls are NOT re-entrant.  One call at a time per
 *    process, which is what the reference's python module does anyway (its calls hold the GIL, swig/python/CMakeLists.txt:5-9);
 *    a multi-threaded C++ host serialises its calls with a mutex.  Handles (gpp_points, gpp_field) are immutable once
 *    created, apart from internal caches that a call fills under that same rule.
 *  - all work is enqueued on the library stream (gpp_get_stream) and the call
 *    returns after the stream is synchronised, unless GPP_MEM_DEVICE |
 *    GPP_ASYNC is given.
 */
#ifndef GRIDPP_HIP_H
#define GRIDPP_HIP_H

#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GPP_OK 0
#define GPP_EINVAL -1
#define GPP_ERUNTIME -2
#define GPP_ENODEVICE -3

#define GPP_MEM_HOST 0
#define GPP_MEM_DEVICE 1
#define GPP_ASYNC 2
/* With GPP_MEM_DEVICE, gpp_neighbourhood_quantile_fast only: the `quantile` argument is in HOST memory although the fields are in HBM -- the
 * scalar quantile of a script (include/gridpp.h:469-486 takes it by value) beside a device-resident cube. */
#define GPP_Q_HOST 8
/* With GPP_MEM_HOST: the float INPUT fields of the call hold float64 values (numpy's default dtype); they are uploaded as
 * they are and cast to float32 on the device -- the rounding the reference's typemap applies on the host
 * (swig/vector.i:42-55).  Outputs stay float32.  Honoured by gpp_optimal_interpolation_full,
 * gpp_optimal_interpolation_ensi, gpp_neighbourhood, gpp_nearest(_levels), gpp_bilinear, gpp_simple_gradient,
 * gpp_full_gradient, gpp_downscale_probability, gpp_mask_threshold_downscale (the cubes and the threshold), gpp_smart and gpp_local_distribution_correction
 * (every `const float*` argument of these that follows `mem` is then a `const double*`), by gpp_fill_missing, gpp_neighbourhood_search and gpp_calc_gradient
 * (their float fields), by gpp_neighbourhood_quantile_fast for `input` only, by gpp_apply_curve and gpp_interpolate for the values
 * (their curves are host float32 arrays), by gpp_apply_curve_field for the values and both curve slabs, by gpp_window for `array`, by gpp_neighbourhood_score for `fcst`,
 * by gpp_dewpoint, gpp_relative_humidity, gpp_wetbulb, gpp_pressure, gpp_sea_level_pressure, gpp_qnh, gpp_wind_speed and
 * gpp_wind_direction for all their inputs, by gpp_transform and gpp_gamma_transform for `in` and by gpp_gamma_inv for its three inputs,
 * by gpp_get_optimal_threshold and gpp_metric_optimizer_curve for `ref` and `fcst` (the thresholds are host float32 values). */
#define GPP_HOST_F64 4

/* include/gridpp.h:120-123 */
#define GPP_GEODETIC 0
#define GPP_CARTESIAN 1

/* include/gridpp.h:88-100 */
#define GPP_MEAN 0
#define GPP_MIN 10
#define GPP_MEDIAN 20
#define GPP_MAX 30
#define GPP_QUANTILE 40
#define GPP_STD 50
#define GPP_VARIANCE 60
#define GPP_SUM 70
#define GPP_COUNT 80
#define GPP_RANDOMCHOICE 90

/* ---- runtime ----------------------------------------------------------- */
const char* gpp_last_error(void);
const char* gpp_version(void);            /* include/gridpp.h:15 GRIDPP_VERSION */
int gpp_device_count(int* count);
/* Path overrides: switches that select between implementations with identical results (the tests reach rarely taken paths with them, A/B
 * timings compare them).  The library reads NO environment variable: an override exists only after gpp_set_path_override(name, value)
 * (name = "GPP_...", value NULL clears it; process-wide).  gpp_active_overrides: the names that are set, comma separated, into buf (NUL
 * terminated); returns how many -- a benchmark must run with none.  No counterpart in the reference.
 * GPP_GRID_CAP = n (n >= 1) is the one override that is no choice of a path: every kernel that walks its work with a grid stride is launched
 * with at most n workgroups (beside its own cap, which stays), so that a small input sends each workgroup through its loop several times, as
 * only a field far beyond the cap does otherwise.  A value below 1 or not a number has no effect (the name is still listed).  No result
 * depends on it, except where a kernel adds inexact per-workgroup partial sums in grid order (the general path of gpp_fractions_skill_score:
 * within that function's stated tolerance). */
int gpp_set_path_override(const char* name, const char* value);
int gpp_active_overrides(char* buf, int len);
/* releases the library's large call-to-call device workspaces (kept otherwise for the next call) and the pool of staging buffers that the
 * host-side fields of a call are copied through (buffers of up to 256 MiB, at most 1 GiB in all) */
int gpp_release_workspaces(void);
int gpp_set_device(int device);           /* one process per GPU: call once with LOCAL_RANK */
int gpp_get_stream(void** hip_stream);    /* the hipStream_t all kernels are launched on */
int gpp_synchronize(void);
/* Page-locked host buffers for results (optional): a caller that hands such a buffer as `out` of a GPP_MEM_HOST call gets
 * the device-to-host copy as one DMA transfer instead of a staged copy into pageable memory.  The python mirror returns its
 * large results in such buffers (the reference returns freshly allocated numpy arrays, swig/vector.i:172-180). */
int gpp_host_alloc(size_t bytes, void** out);
int gpp_host_free(void* p);

/* ---- point sets: gridpp::Points / gridpp::Grid / gridpp::KDTree ----------
 * replaces gridpp::Points::Points (src/api/points.cpp:9-31),
 * gridpp::Grid::Grid (src/api/grid.cpp:12-55) and KDTree::KDTree
 * (src/api/kdtree.cpp:6-16): validates coordinates, converts lat/lon to the
 * float32 x,y,z of src/api/util.cpp:596-612 and keeps them resident in HBM.
 * elevs / lafs may be NULL (filled with NaN).  A grid is a point set with
 * nx > 0 (row-major, index = y*nx + x, src/api/grid.cpp:108-114). */
typedef struct gpp_points gpp_points;
int gpp_points_create(const float* lats, const float* lons, const float* elevs, const float* lafs,
                      int n, int coordinate_type, gpp_points** out);
int gpp_grid_create(const float* lats, const float* lons, const float* elevs, const float* lafs,
                    int ny, int nx, int coordinate_type, gpp_points** out);
/* The same from float64 arrays (numpy's default dtype; the reference's typemap casts them to float32 on the host,
 * swig/vector.i:42-55): the cast happens on the device for large sets. */
int gpp_points_create_f64(const double* lats, const double* lons, const double* elevs, const double* lafs,
                          int n, int coordinate_type, gpp_points** out);
int gpp_grid_create_f64(const double* lats, const double* lons, const double* elevs, const double* lafs,
                        int ny, int nx, int coordinate_type, gpp_points** out);
int gpp_points_destroy(gpp_points* p);
int gpp_points_size(const gpp_points* p, int* n, int* ny, int* nx, int* coordinate_type);
/* field: 0 lat, 1 lon, 2 elev, 3 laf, 4 x, 5 y, 6 z; copies n floats to host `out` */
int gpp_points_get(const gpp_points* p, int field, float* out);

/* gridpp::convert_coordinates (src/api/util.cpp:583-615), host arrays */
int gpp_convert_coordinates(const float* lats, const float* lons, int n, int coordinate_type,
                            float* x, float* y, float* z);

/* KDTree::get_neighbours (src/api/kdtree.cpp:39-60): indices (ascending) of the
 * points strictly inside the +-radius box and within `radius` chord distance of
 * (lat, lon).  Writes at most `cap` indices; *count is the full count. */
int gpp_points_get_neighbours(gpp_points* p, float lat, float lon, float radius, int include_match,
                              int* indices, float* distances /* may be NULL */, int cap, int* count);
/* KDTree::get_closest_neighbours (src/api/kdtree.cpp:82-103): the `num` nearest points, nearest first (ties: lower
 * index); indices must hold `num` ints, *count is the number found. */
int gpp_points_get_closest_neighbours(gpp_points* p, float lat, float lon, int num, int include_match,
                                      int* indices, int* count);
/* KDTree::get_nearest_neighbour / Points::get_nearest_neighbour
 * (src/api/kdtree.cpp:82-106, src/api/points.cpp:55-61) for nq query points
 * (host arrays); index -1 when the set is empty or nothing qualifies. */
int gpp_points_nearest_neighbour(gpp_points* p, const float* qlats, const float* qlons, int nq,
                                 int include_match, int* indices);
/* gridpp::nearest(Grid|Points, Points, values) (src/api/nearest.cpp:124-144):
 * out[i] = values[nearest index of query i]; NaN if the source set is empty.
 * values/out follow `mem`. */
int gpp_nearest(gpp_points* from, gpp_points* to, const float* values, float* out, int mem);
/* The overloads with a leading time dimension (src/api/nearest.cpp:32-71,95-122,145-175,198-222):
 * values [nt][size of from] -> out [nt][size of to]. */
int gpp_nearest_levels(gpp_points* from, gpp_points* to, const float* values, int nt, float* out, int mem);

/* Batched KDTree::get_neighbours / get_neighbours_with_distance / get_num_neighbours (src/api/kdtree.cpp:39-64) for nq
 * lookups (host arrays): counts[nq] always; offsets[nq+1] if given; indices / distances (CSR, ascending index inside a
 * location) if given and *total <= cap -- otherwise only the counts and *total are produced, so that the caller can size
 * the buffers and call again. */
int gpp_points_get_neighbours_batch(gpp_points* p, const float* qlats, const float* qlons, int nq, float radius,
                                    int include_match, int* counts, long long* offsets, int* indices, float* distances,
                                    long long cap, long long* total);
/* gridpp::count (src/api/count.cpp:6-66, all four overloads): out[i] = number of points of `from` within `radius` of
 * location i of `to`.  out follows `mem`. */
int gpp_count(gpp_points* from, gpp_points* to, float radius, float* out, int mem);
/* gridpp::distance (src/api/distance.cpp:6-120, all four overloads): out[i] = the largest KDTree::calc_distance
 * (src/api/kdtree.cpp:107-133) between location i of `to` and its `num` nearest points of `from`.  query_first = 1 for
 * the overloads whose output is a Points (they call calc_distance(location, neighbour)), 0 for those whose output is a
 * Grid (calc_distance(neighbour, location)).  GPP_EINVAL if the coordinate types differ.  The candidate lists (min(num, size of
 * `from`) entries per location) live in an HBM scratch filled in slabs of 2^28 entries (at least one location); the path override
 * GPP_KNN_SLAB = n (n > 0) sets another number of entries per slab.  The result does not depend on it. */
int gpp_distance(gpp_points* from, gpp_points* to, int num, int query_first, float* out, int mem);
/* gridpp::gridding (src/api/gridding.cpp:6-63): statistic of the values of the points of `from` within `radius` of every
 * location of `to`; NaN where fewer than min_num (> 0) points are found.  GPP_EINVAL for radius < 0 / NaN, min_num < 0.
 * values / out follow `mem`. */
int gpp_gridding(gpp_points* to, gpp_points* from, const float* values, float radius, int min_num, int statistic,
                 float* out, int mem);
/* gridpp::gridding_nearest (src/api/gridding.cpp:65-131): every point of `from` is assigned to its nearest location of
 * `to`; statistic of what each location received (in input order), NaN for none / fewer than min_num. */
int gpp_gridding_nearest(gpp_points* to, gpp_points* from, const float* values, int min_num, int statistic, float* out, int mem);

/* gridpp::fill (src/api/fill.cpp:6-41): cells of `igrid` within radii[i] of point i get `value` (outside = 0), or keep
 * `input` while every other cell gets `value` (outside = 1).  radii: host array, one per point.  input/out follow `mem`. */
int gpp_fill(gpp_points* igrid, const float* input, gpp_points* points, const float* radii, float value, int outside,
             float* out, int mem);
/* gridpp::fill_missing (src/api/fill.cpp:43-134): linear interpolation across runs of missing values along rows and
 * along columns, averaged. */
int gpp_fill_missing(const float* values, int ny, int nx, float* out, int mem);
/* gridpp::doping_square (halfwidth != NULL) / doping_circle (radii != NULL) (src/api/doping.cpp:5-93): grid cells in the
 * index window around the nearest grid point of observation i / within radii[i] of it take observations[i]; later
 * observations win; cells whose elevation differs from the observation's by more than max_elev_diff (if valid) are left.
 * halfwidth / radii: host arrays.  background / observations / out follow `mem`. */
int gpp_doping(gpp_points* igrid, const float* background, gpp_points* points, const float* observations,
               const int* halfwidth, const float* radii, float max_elev_diff, float* out, int mem);
/* gridpp::neighbourhood_search (src/api/neighbourhood_search.cpp:7-113); apply_array may be NULL (follows `mem`). */
int gpp_neighbourhood_search(const float* array, const float* search_array, int ny, int nx, int halfwidth,
                             float search_target_min, float search_target_max, float search_delta,
                             const int* apply_array, float* out, int mem);
/* gridpp::calc_gradient (src/api/calc_gradient.cpp:7-126); gradient types as include/gridpp.h:126-129. */
#define GPP_GRADIENT_MINMAX 0
#define GPP_GRADIENT_LINEAR_REGRESSION 10
int gpp_calc_gradient(const float* base, const float* values, int ny, int nx, int gradient_type, int halfwidth, int num_min,
                      float min_range, float default_gradient, float* out, int mem);

/* gridpp::bilinear(Grid, Points|Grid, vec2|vec3) (src/api/bilinear.cpp:26-135; per location :322-403, weights
 * :137-320): `values` holds nt time levels of the input grid, [nt][ny][nx]; out is [nt][size of `to`].  A location
 * outside the grid, or whose box has a missing corner, takes the nearest grid point's value; all NaN if the input
 * grid is empty.  GPP_ERUNTIME ("Problem with bilinear interpolation...") when the weights of a box leave [0, 1]
 * (the reference throws std::runtime_error, :309-313).  values/out follow `mem`. */
int gpp_bilinear(gpp_points* igrid, gpp_points* to, const float* values, int nt, float* out, int mem);
/* Grid::get_box (src/api/grid.cpp:149-229) for nq lookups (host arrays): inside[i] and boxes[4*i..] = Y1, X1, Y2, X2
 * (-1 when no box encloses the point). */
int gpp_grid_get_box(gpp_points* grid, const float* qlats, const float* qlons, int nq, int* inside, int* boxes);
/* gridpp::point_in_rectangle (src/api/util.cpp:571-582): corners A, B, C, D as (lat, lon) pairs. */
int gpp_point_in_rectangle(const float corners_latlon[8], float lat, float lon, int* inside);

/* ---- downscaling with elevation / laf gradients (include/gridpp.h:132-135,844-871,1017-1098) ---------------------------
 * downscaler: GPP_NEAREST (what gpp_nearest_levels computes) or GPP_BILINEAR (what gpp_bilinear computes), applied to each
 * field on its own; anything else is GPP_EINVAL "Invalid downscaler" (src/api/downscaling.cpp:7-61).  `igrid` is a grid;
 * values are [nt][ny][nx] of igrid, out is [nt][size of `to`]; all NaN if igrid is empty.  GPP_ERUNTIME ("Problem with
 * bilinear interpolation...") exactly where gpp_bilinear would raise on one of the fields the reference downscales.  The
 * nearest index and, for GPP_BILINEAR, the box and the weights are found once per location for all fields and levels.
 * values / gradients / out follow `mem` (GPP_HOST_F64 honoured for the input fields). */
#define GPP_NEAREST 0
#define GPP_BILINEAR 1
/* gridpp::simple_gradient, all four overloads (src/api/simple_gradient.cpp:5-100): out = d(values) + (elev of `to` -
 * d(elevs of igrid)) * elev_gradient, with no validity test (a missing elevation or gradient gives NaN). */
int gpp_simple_gradient(gpp_points* igrid, gpp_points* to, const float* values, int nt, float elev_gradient, int downscaler,
                        float* out, int mem);
/* gridpp::full_gradient, all four overloads (src/api/gradient.cpp:5-274): out = d(values) + (laf_corr + elev_corr) with
 * elev_corr = d(elev_gradient) * (elev of `to` - d(elevs of igrid)) where both elevations are valid, else 0, and laf_corr
 * the same with lafs.  elev_gradient / laf_gradient are [nt][ny][nx] (level t of the values uses level t) or NULL: that
 * term is absent (the reference's size() == 0). */
int gpp_full_gradient(gpp_points* igrid, gpp_points* to, const float* values, int nt, const float* elev_gradient,
                      const float* laf_gradient, int downscaler, float* out, int mem);

/* ---- ensemble downscalers (include/gridpp.h:138-143,945-990) ----------------------------------------------------------
 * igrid is a grid, ogrid a grid (or any point set) of the same coordinate type; cubes are [ny][nx][ne] of igrid with the
 * ne members contiguous, threshold and out are [size of ogrid].  Every output cell reads the members of its nearest input
 * cell (what gpp_nearest computes, found once per call).  All NaN if igrid is empty.  GPP_EINVAL for a comparison operator
 * that is none of the four.  Cubes / threshold / out follow `mem` (GPP_HOST_F64 honoured for the inputs). */
#define GPP_LT 0
#define GPP_LEQ 10
#define GPP_GT 20
#define GPP_GEQ 30
/* members of a masked row that gpp_mask_threshold_downscale stages on chip; longer rows take a slower path through HBM */
#define GPP_ENSEMBLE_ROW_CAP 1024
/* gridpp::downscale_probability (src/api/downscale_probability.cpp:7-67): out = (valid members with member OP threshold) /
 * (valid members), NaN where no member is valid. */
int gpp_downscale_probability(gpp_points* igrid, gpp_points* ogrid, const float* values, int ne, const float* threshold,
                              int comparison_operator, float* out, int mem);
/* gridpp::mask_threshold_downscale_consensus / _quantile (src/api/mask_threshold_downscale_consensus.cpp:12-82): member k of
 * a cell's masked row is NaN where threshold_values is not valid, ivalues_true where threshold_values OP threshold, else
 * ivalues_false; out = calc_statistic(row, statistic), or calc_quantile(row, quantile) for GPP_QUANTILE (the _quantile
 * form; _consensus passes quantile 0).  GPP_ERUNTIME "Internal error. Cannot compute statistic" for an unknown statistic,
 * GPP_EINVAL for a quantile outside [0, 1] (a NaN quantile gives NaN).  GPP_RANDOMCHOICE: some valid member of the row.
 * Rows longer than GPP_ENSEMBLE_ROW_CAP go through an HBM scratch in slabs of 2^26 masked members (at least one cell); the path
 * override GPP_ENSEMBLE_SLAB = n (n > 0) sets another number of members per slab.  The result does not depend on it. */
int gpp_mask_threshold_downscale(gpp_points* igrid, gpp_points* ogrid, const float* ivalues_true, const float* ivalues_false,
                                 const float* threshold_values, int ne, const float* threshold, int comparison_operator,
                                 int statistic, float quantile, float* out, int mem);

/* ---- calibration by a curve (include/gridpp.h:79-85,731-789,1549-1557) -----------------------------------------------------
 * Extrapolation policies of apply_curve (include/gridpp.h:79-85). */
#define GPP_ONE_TO_ONE 0
#define GPP_MEAN_SLOPE 10
#define GPP_NEAREST_SLOPE 20
#define GPP_ZERO 30
#define GPP_UNCHANGED 40
/* gridpp::apply_curve(vec | vec2, vec, vec, ...) (src/api/curve.cpp:79-108): one curve for all n values.  Inside
 * [curve_fcst[0], curve_fcst[nc-1]] out = interpolate(fcst, curve_fcst, curve_ref), outside nearestObs + slope * (fcst -
 * nearestFcst) with the slope of the policy (curve.cpp:6-77, quirks included: see gridpp_amd/csrc/curve.h).  The curve is always a
 * host float32 array (the library uploads it); any curve works, sorted or not.  fcst / out follow `mem` (GPP_HOST_F64 honoured
 * for fcst).  GPP_EINVAL before any device work: nc_ref != nc_fcst, nc == 0, a policy that is none of the five ("Unknown
 * extrapolation policy": checked up front whatever the data -- the reference throws only when some value extrapolates with
 * nc > 1).  n == 0 returns GPP_OK and writes nothing. */
int gpp_apply_curve(const float* fcst, long long n, const float* curve_ref, int nc_ref, const float* curve_fcst, int nc_fcst,
                    int policy_below, int policy_above, float* out, int mem);
/* gridpp::apply_curve(vec2, vec3, vec3, ...) (src/api/curve.cpp:110-133): one curve per cell.  fcst / out are [ny][nx], the curves
 * [ny][nx][nc] with nc contiguous; all follow `mem` (GPP_HOST_F64 honoured for the three inputs).  Errors as gpp_apply_curve. */
int gpp_apply_curve_field(const float* fcst, const float* curve_ref, const float* curve_fcst, int ny, int nx, int nc_ref, int nc_fcst,
                          int policy_below, int policy_above, float* out, int mem);
/* gridpp::interpolate(vec, vec, vec) (src/api/util.cpp:415-426): out[i] = the curve (ix, iy) at x[i] with the linear-scan index
 * rules of util.cpp:339-376, the end value outside [ix[0], ix[nc-1]], NaN for a NaN x or an empty curve.  ix / iy are host
 * float32 arrays; x / out follow `mem` (GPP_HOST_F64 honoured for x).  GPP_EINVAL "Dimension mismatch. Cannot interpolate." */
int gpp_interpolate(const float* x, long long n, const float* ix, int nc_x, const float* iy, int nc_y, float* out, int mem);
/* Host-only forms (no GPU needed, like gpp_convert_coordinates); they run the per-value source of the kernels.
 * gridpp::apply_curve(float, ...) (curve.cpp:6-77), with the reference's lazy policy check: an unknown policy is GPP_EINVAL only
 * where the input extrapolates with it and nc > 1. */
int gpp_apply_curve_scalar(float input, const float* curve_ref, int nc_ref, const float* curve_fcst, int nc_fcst, int policy_below,
                           int policy_above, float* out);
/* gridpp::interpolate(float, vec, vec) (util.cpp:377-414): an invalid x gives NaN before the sizes are compared, as there. */
int gpp_interpolate_scalar(float x, const float* ix, int nc_x, const float* iy, int nc_y, float* out);
/* gridpp::monotonize_curve (curve.cpp:134-250): out_ref / out_fcst hold nc floats, *count = entries written (0 where no pair of
 * the curve is valid: the reference reads an empty vector there). */
int gpp_monotonize_curve(const float* curve_ref, int nc_ref, const float* curve_fcst, int nc_fcst, float* out_ref, float* out_fcst,
                         int* count);
/* gridpp::quantile_mapping_curve (src/api/quantile_mapping.cpp:5-46): quantiles may be NULL (nq = 0).  out_ref / out_fcst hold
 * max(n, nq) floats, *count = entries written.  With quantiles the index int(q * (n - 1)) selects from the UNSORTED inputs, as
 * the reference does (:41-42).  NaN inputs sort last. */
int gpp_quantile_mapping_curve(const float* ref, int n_ref, const float* fcst, int n_fcst, const float* quantiles, int nq,
                               float* out_ref, float* out_fcst, int* count);

/* ---- structure functions (src/api/structure.cpp) -----------------------------
 * Scalar forms of BarnesStructure, CressmanStructure, SoarStructure, ToarStructure,
 * PowerlawStructure, LinearStructure (structure.cpp:143-167,287-299,317-341,467-491,
 * 618-642,765-789), MultipleStructure (:90-138: horizontal / vertical / laf factors taken
 * from three structures), the CrossValidation wrapper (:910-944) and the spatially varying
 * forms (per-grid-point h, v, w looked up at the first point of corr(p1, p2), :168-214). */
#define GPP_SK_BARNES 0
#define GPP_SK_CRESSMAN 1
#define GPP_SK_SOAR 2
#define GPP_SK_TOAR 3
#define GPP_SK_POWERLAW 4
#define GPP_SK_LINEAR 5
#define GPP_ST_HAS_LOC 1   /* `loc` holds the localization distance (else derived from kind, h, min_rho) */
#define GPP_ST_CV 2        /* CrossValidation: corr_background = 0 within cv_dist */
typedef struct gpp_structure {
    int kind;        /* kernel of the horizontal factor (GPP_SK_*) */
    float h, v, w;   /* scales: horizontal [m], vertical [m], land-area-fraction */
    float min_rho;   /* m_min_rho of the horizontal structure; see gpp_structure_min_rho */
    int kind_v;      /* kernel of the vertical factor + 1; 0 = same as `kind` (MultipleStructure sets these) */
    int kind_w;      /* kernel of the laf factor + 1;      0 = same as `kind` */
    float loc;       /* localization distance if flags & GPP_ST_HAS_LOC */
    float cv_dist;   /* CrossValidation distance if flags & GPP_ST_CV */
    int flags;
    struct gpp_field* field;   /* spatially varying form: h, v, w fields (gpp_field_create); NULL = scalar */
    /* MultipleStructure(sh, sv, sw) with spatially varying parts (structure.cpp:90-138): `field` = sh's (its h and the localization
     * distance), field_v = sv's (its v), field_w = sw's (its w); NULL = that factor is scalar (v / w above) */
    struct gpp_field* field_v;
    struct gpp_field* field_w;
} gpp_structure;
/* BarnesStructure(Grid, vec2 h, vec2 v, vec2 w, min_rho) and the Soar/Toar/Powerlaw/Linear equivalents
 * (structure.cpp:168-184,342-358,...): h, v, w are host arrays with one value per point of `grid`
 * (which must outlive the field). */
typedef struct gpp_field gpp_field;
int gpp_field_create(gpp_points* grid, const float* h, const float* v, const float* w, int kind, float min_rho, gpp_field** out);
int gpp_field_destroy(gpp_field* field);
/* m_min_rho of the scalar constructors from hmax (NaN: default 0.0013); validates h >= 0, hmax >= 0 */
int gpp_structure_min_rho(int kind, float h, float hmax, float* min_rho);
/* StructureFunction::localization_distance(Point) (structure.cpp:87-89,271-282,454-459,604-610,755-757,902-904);
 * (lat, lon) only matters for the spatially varying forms */
int gpp_structure_localization_distance(const gpp_structure* s, float lat, float lon, float* dist);
/* corr (background = 0) / corr_background (background = 1) for one pair of points given as
 * (x, y, z, elev, laf, lat, lon) -- runs the same device code as the OI kernels */
int gpp_structure_corr(const gpp_structure* s, const float p1[7], const float p2[7], int background, float* rho);
/* corr / corr_background of p1 against n points, StructureFunction::corr(const Point&, const std::vector<Point>&)
 * (include/gridpp.h:2078,2086; structure.cpp:13-25,113-135,231-267): the scales are taken at p1 ONCE (structure.cpp:234-243) and all
 * pairs run in one kernel launch over the device code of gpp_structure_corr, so the values equal that entry's bit for bit.
 * p2: n records of 7 floats (x, y, z, elev, laf, lat, lon), host memory; rho: n floats, host memory.  n == 0: nothing is done. */
int gpp_structure_corr_many(const gpp_structure* s, const float p1[7], const float* p2, long long n, int background, float* rho);
/* the same against every point of a Points / Grid handle (its x, y, z, elev, laf are already in HBM: nothing is uploaded);
 * rho: size of the handle (row-major for a grid), GPP_MEM_HOST or GPP_MEM_DEVICE.  An empty handle: nothing is done. */
int gpp_structure_corr_points(const gpp_structure* s, const float p1[7], gpp_points* to, int background, float* rho, int mem);

/* gridpp::staticcorr_points (src/api/corr_points.cpp:26-131): out [size of points][size of knots] = corr_background(point,
 * knot) for the knots a point keeps (inside its localization radius, rho > 0, the max_points largest if there are more; 0
 * elsewhere).  Scalar structure functions.  out follows `mem`. */
int gpp_staticcorr_points(gpp_points* points, gpp_points* knots, const gpp_structure* structure, int max_points, float* out, int mem);

/* gridpp::smart (src/api/smart.cpp:12-66): out [size of ogrid] = mean of `values` ([ny][nx] of igrid) over the min(num, n)
 * input cells of largest corr(output cell, input cell) among the n cells within the structure's localization distance
 * (rho descending, ties -> lower index of the input grid; cells with rho = 0 take part).  No validity test on the values;
 * NaN where n = 0 or num <= 0.  Scalar structure functions.  values / out follow `mem` (GPP_HOST_F64 honoured). */
int gpp_smart(gpp_points* igrid, gpp_points* ogrid, const float* values, int num, const gpp_structure* structure, float* out, int mem);

/* gridpp::local_distribution_correction (src/api/local_distribution_correction.cpp:18-203; the vec form :18-32 is nT = 1):
 * out [ny][nx] of grid = `background` mapped through the two cumulative-rho curves of the valid, non-negative
 * (pobs, pbackground) pairs ([nT][size of points] each) of the stations within the structure's localization distance, rho =
 * corr_background(cell, station); stations with rho = 0 take part.  Both curves are sorted by value and, where values tie,
 * by rho ascending -- the reference leaves the order of tied values to an unstable sort and to its R-tree;
 * on tie-free data this is the reference's result.  A cell with an invalid background or fewer than min_points pairs keeps
 * its background; an empty point set returns the background.  EINVAL: different coordinate types, nT < 0, quantiles not
 * finite or not 0 <= min_quantile <= max_quantile <= 1.  Scalar structure functions.  `out` must not overlap an input.
 * background / pobs / pbackground / out follow `mem` (GPP_HOST_F64 honoured). */
int gpp_local_distribution_correction(gpp_points* grid, const float* background, gpp_points* points, const float* pobs,
                                      const float* pbackground, int nT, const gpp_structure* structure, float min_quantile,
                                      float max_quantile, int min_points, float* out, int mem);

/* ---- optimal interpolation ------------------------------------------------
 * replaces gridpp::optimal_interpolation_full (src/api/oi.cpp:138-341, Points
 * form; the Grid form :342-412 is the same call on a grid handle) and through
 * it gridpp::optimal_interpolation (src/api/oi.cpp:26-136: bvariance == NULL
 * and bvariance_at_points == NULL mean "all ones", out_variance may be NULL).
 * background/bvariance/out/out_variance have bgrid-size elements; obs,
 * obs_variance, background_at_points, bvariance_at_points have points-size
 * elements.  Errors: GPP_EINVAL as oi.cpp:152-186; GPP_ERUNTIME if a local
 * (P+R) matrix is singular (arma::inv throws, oi.cpp:315). */
int gpp_optimal_interpolation_full(gpp_points* bgrid, const float* background, const float* bvariance,
                                   gpp_points* points, const float* obs, const float* obs_variance,
                                   const float* background_at_points, const float* bvariance_at_points,
                                   const gpp_structure* structure, int max_points, int allow_extrapolation,
                                   float* out, float* out_variance, int mem);

/* ---- ensemble optimal interpolation (EnSI) ----------------------------------------
 * replaces gridpp::optimal_interpolation_ensi (src/api/oi_ensi.cpp:114-568, Points
 * form; the Grid form :33-112 is the same call on a grid handle).  background and out
 * are [bgrid-size][ne], background_at_points is [points-size][ne]; obs and sigmas have
 * points-size elements.  Members that are invalid anywhere in the field are left
 * untouched (oi_ensi.cpp:187-201). */
int gpp_optimal_interpolation_ensi(gpp_points* bgrid, const float* background, int ne, gpp_points* points,
                                   const float* obs, const float* sigmas, const float* background_at_points,
                                   const gpp_structure* structure, int max_points, int allow_extrapolation,
                                   float* out, int mem);
int gpp_ensi_last_kernel_ms(float* ms);
/* Statistics of the calling thread's last gpp_optimal_interpolation_ensi: condition_passthrough = grid points left at their background
 * values because their E x E system is singular or not finite -- the count behind the reference's warning "Condition number error in N
 * points. Using raw values in those points." (src/api/oi_ensi.cpp:153,386-390,557-561), which the mirrors print; real_part_passthrough
 * = the reference's second counter (:154,423-426,562-566: an empty real part of the matrix square root), which cannot happen for the
 * symmetric square root the kernels form and is always 0. */
typedef struct gpp_ensi_stats {
    long long cells;
    long long condition_passthrough;
    long long real_part_passthrough;
    float kernel_ms;
} gpp_ensi_stats;
int gpp_ensi_last_stats(gpp_ensi_stats* stats);
/* 1: the Jacobi sweeps of the per-cell eigenproblem run to convergence (reference-grade last bits, ~2x the time);
 * 0 (default): they stop at |off-diagonal| <= 0.040 (E - 1) and a perturbation series supplies the rest (since round 4 this
 * mode meets the plain 1e-5 measure on every value of the randomised soak as well: worst 2.5e-6, the same as with converged sweeps).
 * Per calling thread. */
int gpp_ensi_set_convergence(int to_convergence);

/* gridpp::optimal_interpolation_ensi_multi_ebe / _ebesc / _utem (include/gridpp.h:311-441, src/api/oi_ensi_multi.cpp:329-1311;
 * Points overloads, a Grid is its row-major flattening).  variant: 1 = ebe, 2 = ebesc, 3 = utem.  bratios [bgrid-size];
 * background / background_corr / out [bgrid-size][ne]; pobs [points-size][ne] (ebe, ebesc) or [points-size] (utem); pratios
 * [points-size]; pbackground / pbackground_corr [points-size][ne].  background_corr / pbackground_corr are ignored by ebesc
 * (may be NULL).  Members invalid in any of the fields are left untouched (:395-418). */
int gpp_optimal_interpolation_ensi_multi(int variant, gpp_points* bgrid, const float* bratios, const float* background,
                                         const float* background_corr, int ne, gpp_points* points, const float* pobs,
                                         const float* pratios, const float* pbackground, const float* pbackground_corr,
                                         const gpp_structure* structure, int max_points, int allow_extrapolation, float* out, int mem);   /* hipEvent time of the last EnSI kernel (diagnostics / bench) */

/* ---- multi-GPU helpers (no counterpart in the reference, whose parallelism is OpenMP, src/api/oi.cpp:221) --------
 * One process per GPU.  The output grid is cut into contiguous row tiles (gpp_row_tile), every rank builds its tile's Grid and
 * the full Points, rank 0 owns the observation values of a step and broadcasts them (gpp_comm_broadcast: ncclBroadcast over
 * xGMI on the library stream), the neighbourhood filters get their halfwidth-row halos from the neighbouring ranks
 * (gpp_comm_halo_exchange: ncclSend / ncclRecv).  There is no other cross-tile dependence.  RCCL is loaded on first use. */
int gpp_row_tile(int ny, int rank, int world, int* row0, int* row1);
int gpp_comm_unique_id(char* id128);                              /* rank 0; the caller distributes the 128 bytes */
int gpp_comm_init(int rank, int world, const char* id128);        /* collective; after gpp_set_device */
int gpp_comm_rank(int* rank, int* world);                         /* (0, 1) without a communicator */
int gpp_comm_broadcast(void* device_buf, size_t bytes, int root); /* in place, device memory, library stream */
int gpp_comm_broadcast_host(void* host_buf, size_t bytes, int root); /* host memory, staged through HBM */
int gpp_comm_halo_exchange(const float* tile, int rows, size_t row_floats, int halfwidth, float* padded, int* top_rows);
int gpp_comm_destroy(void);

/* ---- neighbourhood filters (src/api/neighbourhood.cpp) -------------------------
 * input is [ny][nx] (is3d == 0, ne must be 1) or [ny][nx][ne] (is3d == 1); out is
 * [ny][nx].  Empty input (any extent 0) returns GPP_OK and writes nothing
 * (neighbourhood.cpp:33-34).  Windows are clipped at the domain edge; NaN / inf
 * values are ignored (util.cpp:16-18). */
/* gridpp::neighbourhood(vec2|vec3, halfwidth, statistic) (neighbourhood.cpp:12-242) */
int gpp_neighbourhood(const float* input, int ny, int nx, int ne, int is3d, int halfwidth, int statistic,
                      float* out, int mem);
/* gridpp::neighbourhood_brute_force (statistic != GPP_QUANTILE) and
 * gridpp::neighbourhood_quantile (statistic == GPP_QUANTILE, exact order statistics)
 * (neighbourhood.cpp:528-539,557-654; util.cpp:19-178) */
int gpp_neighbourhood_brute_force(const float* input, int ny, int nx, int ne, int halfwidth, int statistic,
                                  float quantile, float* out, int mem);
/* gridpp::neighbourhood_quantile_fast, all four overloads (neighbourhood.cpp:296-527):
 * quantile is one value (nq == 1) or a [ny][nx] field (nq == ny*nx); thresholds[nt]. */
int gpp_neighbourhood_quantile_fast(const float* input, int ny, int nx, int ne, int is3d,
                                    const float* quantile, int nq, int halfwidth,
                                    const float* thresholds, int nt, float* out, int mem);
/* Many levels per cell, no counterpart in the reference (gridpp_amd.neighbourhood_quantiles_fast): out is [ny][nx][nq] with nq contiguous,
 * out[y][x][j] = exactly the bits gpp_neighbourhood_quantile_fast gives at (y, x) for the scalar level quantiles[j], on every path.  input,
 * thresholds and out follow `mem` (GPP_HOST_F64 applies to `input` only); `quantiles` is a host float32 array whatever `mem` says, in any
 * order, repeats allowed.  Checked in this order, before any device work: halfwidth < 0 is GPP_EINVAL ("Half width must be > 0"); an empty
 * field returns GPP_OK and writes nothing; a NULL pointer is GPP_EINVAL; a level below 0 or above 1 is GPP_EINVAL ("All quantiles must be >= 0
 * and <= 1"; NaN passes and gives a NaN plane); nq == 0 returns GPP_OK and writes nothing.  nt == 0 gives NaN everywhere.  The member pass and
 * the window sums run once for all levels (csrc/qf_box.hip, k_qf_box_multi); GPP_QF_NO_FUSED, GPP_QF_NO_RANKS and
 * GPP_QF_NO_SPEC act as they do on gpp_neighbourhood_quantile_fast, and the two entry points may follow each other in any order. */
int gpp_neighbourhood_quantiles_fast(const float* input, int ny, int nx, int ne, int is3d,
                                     const float* quantiles, int nq, int halfwidth,
                                     const float* thresholds, int nt, float* out, int mem);
/* The curve gpp_neighbourhood_quantile_fast interpolates in (gridpp_amd.neighbourhood_cdf): out is [ny][nx][nt] with nt contiguous, out[y][x][t] =
 * P(member <= thresholds[t]) over the window and the members -- the reference's yarray[t] (neighbourhood.cpp:490-509; 2-D input: :374-394) for the
 * thresholds as given, in [0, 1], NaN where the window holds no valid cell.  halfwidth < 0 is GPP_EINVAL ("Half width must be > 0"); an empty
 * field or nt == 0 returns GPP_OK and writes nothing; a NULL pointer is GPP_EINVAL.  Same passes, paths and overrides as above. */
int gpp_neighbourhood_cdf(const float* input, int ny, int nx, int ne, int is3d, int halfwidth,
                          const float* thresholds, int nt, float* out, int mem);
/* A spatial filter of every member, no counterpart in the reference (gridpp_amd.neighbourhood_members): input and out are
 * [ny][nx][ne] with ne contiguous, plane e of out = gpp_neighbourhood of plane e of input as a 2-D field.  Mean, Sum, Count, Min, Max, Std and
 * Variance at any halfwidth >= 0.  Checked in this order, before any device work: halfwidth < 0 is GPP_EINVAL ("Half width must be > 0");
 * GPP_QUANTILE is GPP_EINVAL with gpp_neighbourhood's message; GPP_MEDIAN and GPP_RANDOMCHOICE are GPP_EINVAL (order statistics per member are
 * not supported); an empty cube returns GPP_OK and writes nothing; a NULL pointer is GPP_EINVAL.  input / out follow `mem` (GPP_HOST_F64: input).
 * Mean / Sum / Count (and Std / Variance through them) run in one kernel out of LDS where halfwidth * ne <= 1024 and in two passes over bands of rows
 * otherwise (csrc/members.hip); the path overrides GPP_MEMBERS_TWO_PASS (the two-pass form everywhere), GPP_MEMBERS_BAND_ROWS (rows of a band) and
 * GPP_MEMBERS_SEG_ROWS (rows a workgroup of the fused form marches down) choose between them; the result does not depend on the path. */
int gpp_neighbourhood_members(const float* input, int ny, int nx, int ne, int halfwidth, int statistic, float* out, int mem);
/* gpp_calc_gradient of every member (gridpp_amd.calc_gradient_members): values and out are [ny][nx][ne]; base is [ny][nx]
 * (base_members == 1: one field shared by the members) or [ny][nx][ne] (base_members == ne).  Plane e of out = gpp_calc_gradient(base_e, plane e
 * of values, ...).  The checks of gpp_calc_gradient in its order with its messages, then base_members outside {1, ne} ("base is not the same size
 * as values"), all GPP_EINVAL before any device work.  base / values / out follow `mem` (GPP_HOST_F64: base and values). */
int gpp_calc_gradient_members(const float* base, int base_members, const float* values, int ny, int nx, int ne, int gradient_type, int halfwidth,
                              int num_min, float min_range, float default_gradient, float* out, int mem);

/* ---- per-row statistics (src/api/util.cpp) -------------------------------------
 * array is [rows][len]; one result per row. */
/* gridpp::calc_statistic(vec|vec2, statistic) (util.cpp:19-110,208-215) */
int gpp_calc_statistic(const float* array, long rows, int len, int statistic, float* out, int mem);
/* gridpp::calc_quantile(vec|vec2, q) and (vec3, vec2 q) (util.cpp:111-207): nq == 1 or nq == rows, else GPP_EINVAL ("Dimension mismatch between
 * array and quantile"); then a level below 0 or above 1 is GPP_EINVAL (NaN passes and gives NaN).  `quantile` lives where `array` does: with
 * GPP_MEM_DEVICE its range is checked on the device and one flag is read back.  Exact order statistics, rows of any length and any number
 * (csrc/rows_select.hip: selection by keys out of LDS for rows of up to 160 values, a radix select per row beyond, several workgroups per row
 * for few long rows); the result does not depend on the path. */
int gpp_calc_quantile(const float* array, long rows, int len, const float* quantile, long nq, float* out, int mem);
/* Many levels per row, no counterpart in the reference (gridpp_amd.calc_quantiles, quantile_mapping_curves): out is [rows][nq] with nq contiguous,
 * out[r][j] = exactly the bits gpp_calc_quantile gives for row r at the level quantiles[j].  array / out follow `mem`; `quantiles` is a host
 * float32 array whatever `mem` says (like the curves of gpp_apply_curve), in any order, repeats allowed.  GPP_EINVAL before any device work: a
 * NULL pointer, a level below 0 or above 1 ("calc_quantiles: Quantiles must be between 0 and 1 inclusive"; NaN passes and gives NaN).  rows == 0
 * or nq == 0 returns GPP_OK and writes nothing.  Rows of up to 8192 values are sorted once in LDS and every level picked out of the sorted row
 * where that beats one selection per level (csrc/rows_quantiles.hip; the path override GPP_ROWS_QUANTILES = tile | block | loop forces a path
 * where it applies); longer rows, and nq == 1, run gpp_calc_quantile's selection once per level.  The result does not depend on the path. */
int gpp_calc_quantiles(const float* array, long rows, int len, const float* quantiles, int nq, float* out, int mem);
/* Ranks within rows, no counterpart in the reference (gridpp_amd.calc_ranks, sort_rows, reorder_by_ranks, calc_crps).  Valid means
 * finite; valid values compare numerically (-0.0 == +0.0) and equal values are ordered by position, lower index first: the order of
 * numpy.argsort(kind="stable") on the valid values of a row.  All arrays are [rows][len] with len contiguous and follow `mem`.  GPP_EINVAL
 * before any device work: a negative size, a NULL pointer.  rows == 0 returns GPP_OK and writes nothing.  Rows of up to 160 values are ranked by
 * counting out of LDS, 64 rows per wave; rows of up to 8192 are sorted in LDS, one workgroup per row; longer rows go through a segmented radix
 * sort (csrc/rows_rank.hip; the path override GPP_ROWS_RANKS = tile | block | long forces a path where it applies).  The result does not depend
 * on the path. */
/* ranks[r][i] (int32) = #{valid j : a[j] < a[i]} + #{valid j < i : a[j] == a[i]}, -1 for an invalid a[i]; sorted[r][ranks[r][i]] = a[i] with
 * its bits kept, NaN from the number of valid values on.  Either output may be NULL (both NULL is GPP_EINVAL); both come from one launch. */
int gpp_calc_ranks(const float* array, long rows, int len, int* ranks, float* sorted, int mem);
/* out[r][i] = sorted(values row r)[rank of templ[r][i] within its row]; NaN where templ[r][i] is invalid or its rank is not below the number of
 * valid entries of the values row.  Bit for bit the composition of the two outputs of gpp_calc_ranks. */
int gpp_reorder_by_ranks(const float* values, const float* templ, long rows, int len, float* out, int mem);
/* out[r] = (1 / N) sum_k |x_(k) - y| - (1 / N^2) sum_k (2 k - N + 1) x_(k) over the N sorted valid members x_(k) of ensemble row r, y = ref[r];
 * both sums in double, cast to float32 last; NaN when N == 0 or y is not finite.  ref and out hold rows values. */
int gpp_calc_crps(const float* ensemble, const float* ref, long rows, int len, float* out, int mem);
/* gridpp::calc_even_quantiles (util.cpp:261-338) and, with only_valid = 1,
 * gridpp::get_neighbourhood_thresholds (neighbourhood.cpp:243-295) over the n
 * values of a flattened field.  out holds num floats; *count = number written. */
int gpp_calc_even_quantiles(const float* values, long n, int num, int only_valid, float* out, int* count, int mem);

/* ---- window statistics along the time axis (src/api/window.cpp) -----------------
 * gridpp::window (src/api/window.cpp:6-156, include/gridpp.h:1602-1611): array and out are [ny][nx] = (case, time) with time
 * contiguous; out[y][x] = the statistic over the window [x - length + 1, x] (before != 0) or [x - length / 2, x + length / 2] of row
 * y, clipped to the row.  NaN and +-Inf do not count (util.cpp:16-18).  GPP_MEAN / GPP_SUM / GPP_COUNT take differences of the row's
 * sequential float32 prefix sum, as the reference does (window.cpp:33-111: the result is that difference, not the exact window sum);
 * Count ignores the two flags.  GPP_MIN / GPP_MAX / GPP_MEDIAN / GPP_STD / GPP_VARIANCE / GPP_RANDOMCHOICE are calc_statistic over the
 * clipped window (window.cpp:112-153).  keep_missing: NaN where the window holds a value that does not count; missing_edges: NaN where
 * the window reaches past either end of the row.  Checks in the reference's order, all before any device work: GPP_EINVAL "Length
 * variable must be > 0"; ny * nx == 0 returns GPP_OK and writes nothing; GPP_EINVAL "Length variable must be an odd number" (an even
 * length with before == 0); GPP_ERUNTIME for GPP_QUANTILE and any value that is no statistic (the reference throws inside its loop).
 * array / out follow `mem` (GPP_HOST_F64 honoured for array).  Any length and any nx: spans that do not fit the fused tile
 * (GPP_WINDOW_FUSED_SPAN) take a general path with the same results. */
#define GPP_WINDOW_TILE_ROWS 64    /* rows of a tile of the fused kernels */
#define GPP_WINDOW_TILE_COLS 32    /* columns of a chunk of a tile */
#define GPP_WINDOW_FUSED_SPAN 31   /* fused while back + lead <= this: back = length - 1 (before) or length / 2, lead = 0 (before) or
                                    * length / 2 rounded up to a multiple of 4, both after clamping length / 2 and length - 1 to nx */
int gpp_window(const float* array, long long ny, int nx, int length, int statistic, int before, int keep_missing, int missing_edges,
               float* out, int mem);

/* ---- verification scores (include/gridpp.h:103-110,  src/api/metric_optimizer.cpp:185-244, src/api/neighbourhood_score.cpp) ----
 * gridpp::Metric (include/gridpp.h:103-110). */
#define GPP_METRIC_ETS 0
#define GPP_METRIC_TS 1
#define GPP_METRIC_KSS 20
#define GPP_METRIC_PC 30
#define GPP_METRIC_BIAS 40
#define GPP_METRIC_HSS 50
/* gridpp::calc_score(a, b, c, d, metric) (metric_optimizer.cpp:207-244) with the reference's float / double promotions, operation for
 * operation.  Host only, no GPU needed.  GPP_EINVAL "Unknown metric" for a value that is none of the six. */
int gpp_calc_score_table(float a, float b, float c, float d, int metric, float* out);
/* gridpp::calc_score(ref, fcst, threshold, fthreshold, metric) (metric_optimizer.cpp:188-206; the four-argument form passes threshold
 * twice): the contingency table of the first n elements of both vectors, counted on the device in integers, then the scalar rule above.  A
 * NaN ref is counted nowhere, a NaN fcst as c or d (it fails `fcst > fthreshold`), as in the reference, whose float counters stop growing
 * at 2^24: every count is clamped to 16777216.  n == 0 needs no device (Bias is 1, the others NaN).  The caller makes sure that ref holds n
 * elements (the reference reads past a shorter one).  ref / fcst follow `mem`; *out is host memory. */
int gpp_calc_score(const float* ref, const float* fcst, long long n, float threshold, float fthreshold, int metric, float* out, int mem);
/* gridpp::neighbourhood_score (neighbourhood_score.cpp:6-60): fcst and out are [ny][nx] of `grid` (a grid handle) and follow `mem`
 * (GPP_HOST_F64 honoured for fcst); ref is a HOST array of one value per point of `points`, whatever `mem` says.  ref_grid =
 * gridding_nearest(grid, points, ref, 1, Mean); a cell counts where ref_grid and fcst are both finite, as a / b (fcst > threshold, ref_grid
 * > / <= threshold) or c / d; out = calc_score of the four fractions (float)((double)n / area) over the window [y +- half_width] x [x +-
 * half_width] clipped to the grid, area = the cells of the clipped window.  GPP_EINVAL before any device work: "half_width must be greater
 * than 0", then "Unknown metric".  The sizes of fcst and ref are the caller's to check (the reference's first and last check).  An empty
 * grid returns GPP_OK and writes nothing.  Half widths up to GPP_SCORE_FUSED_MAXHW take one fused kernel (row and column pass over one
 * byte per cell, the four counts packed in 16-bit lanes, which holds while (2 half_width + 1)^2 < 65536); wider ones, and every call
 * under the path override GPP_SCORE_GENERAL, a separable pair with 32-bit counters.  Both give the same bits.  The fused launch cuts the
 * rows into segments so that about 1024 workgroups exist; the path override GPP_SCORE_FILL = n (n >= 1) sets another number, n = 1 giving
 * one workgroup per strip that marches down every row, as on fields of millions of cells.  The result does not depend on it. */
#define GPP_SCORE_TILE_COLS 64      /* output columns of a strip of the fused kernel */
#define GPP_SCORE_TILE_ROWS 32      /* rows of a chunk of the strip */
#define GPP_SCORE_FUSED_MAXHW 16    /* the ring of the fused kernel holds 32 + 2 * 16 rows; (2 * 16 + 1)^2 = 1089 < 65536 */
int gpp_neighbourhood_score(gpp_points* grid, gpp_points* points, const float* fcst, const float* ref, int half_width, int metric,
                            float threshold, float* out, int mem);
/* The Fractions Skill Score for nt thresholds x nh half widths in one call, no counterpart in the reference (gridpp_amd.fractions_skill_score;
 * DESIGN.md 4.22).  fcst is [ny][nx] (is3d == 0, ne must be 1) or a cube [ny][nx][ne] (is3d == 1), ref is [ny][nx]; both follow `mem`
 * (GPP_HOST_F64 is not honoured).  thresholds[nt], halfwidths[nh] and the three outputs are HOST arrays whatever `mem` says: fbs and fbs_worst
 * are [nt][nh] doubles, cells is [nh].  A cell counts where ref is valid and fcst has a valid member; with m its valid members, k those that
 * meet `member op threshold` and o = `ref op threshold`, a cell whose window [y +- hw] x [x +- hw] (clipped to the grid) holds n > 0 counting
 * cells adds (K / M - O / n)^2 to fbs[t][h] and (K / M)^2 + (O / n)^2 to fbs_worst[t][h], K, M, O the exact integer sums of k, m, o over the
 * counting cells of the window and the arithmetic double; cells[h] = the number of such cells.  The score itself is GPP_FSS_VALUE of the two
 * sums, and of their sums over many calls when cases are pooled.  GPP_EINVAL before any device work: a negative size, ne != 1 with is3d == 0,
 * a NULL array that would be read or written, a NaN threshold (+-Inf are legal), "Half width must be > 0" for a negative one, "Invalid
 * comparison operator" for a value that is not GPP_LT / GPP_LEQ / GPP_GT / GPP_GEQ.  nt == 0, nh == 0 and an empty field need no device: the
 * outputs that exist are zero.  Half widths up to GPP_FSS_FUSED_MAXHW take one fused kernel per half width (row and column pass, the four
 * sums packed in one 64-bit word with lanes of bk, bk, bn and bn bits: bn the smallest width that holds (2 hw + 1)^2, bk = (64 - 2 bn) / 2,
 * taken while (2 hw + 1)^2 ne < 2^bk and ne <= 32767); wider ones, larger ensembles and every call under the path override
 * GPP_FSS_GENERAL a separable pair with 64-bit window sums (GPP_FSS_GENERAL = wide: with 64-bit row sums too, as for (2 hw + 1) ne >= 2^32).
 * The path override GPP_FSS_FILL = n sets the workgroups per threshold the fused launch aims for (1024), as GPP_SCORE_FILL does.  Partial sums
 * are stored per workgroup and added in a fixed order: the results are bit-identical from call to call, on either path; between the paths
 * they differ by the order of the additions only. */
#define GPP_FSS_TILE_COLS 64      /* output columns of a strip of the fused kernel */
#define GPP_FSS_TILE_ROWS 32      /* rows of a chunk of the strip */
#define GPP_FSS_FUSED_MAXHW 16    /* the ring of the fused kernel holds 32 + 2 * 16 rows */
#define GPP_FSS_VALUE(fbs, fbs_worst) ((fbs_worst) == 0.0 ? (double)NAN : 1.0 - (double)(fbs) / (double)(fbs_worst))   /* needs <math.h> */
int gpp_fractions_skill_score(const float* fcst, const float* ref, int ny, int nx, int ne, int is3d, const float* thresholds, int nt,
                              const int* halfwidths, int nh, int comparison_operator, double* fbs, double* fbs_worst, long long* cells, int mem);

/* ---- the optimal forecast threshold (include/gridpp.h, src/api/metric_optimizer.cpp:105-184) ----------------------------------------
 * NOT the reference's result: the reference minimises with Boost's brent_find_minima, which ends on an arbitrary point of whichever
 * plateau of the piecewise-constant score it reaches.  These entries return the exact optimum over all plateaus, so
 * they are no part of the reference-compatible surface.
 * s(x) = gpp_calc_score(ref, fcst, n, threshold, x, metric), with its counting rules and its cap of 2^24 per count.  u_0 < ... < u_{m-1}
 * are the distinct finite values of fcst (-0 counts as +0); s is constant on [u_k, u_{k+1}) and at u_{m-1}.  best = the largest score
 * over these plateaus that is neither NaN nor infinite; [lo, hi) = the lowest run of adjacent plateaus whose score equals best (hi =
 * u_{m-1} when the run reaches the top); *out = (float)(((double)lo + (double)hi) / 2), or lo where hi > lo and that rounds to hi.  NaN
 * when no plateau has a valid score, when best <= 0.0001f, and when |best - s(u_0)| < 0.001f or |best - s(u_{m-1})| < 0.001f (the
 * reference's filters, metric_optimizer.cpp:165-182); also for n == 0 (no device needed) and without a finite fcst.  GPP_EINVAL "Unknown
 * metric".  The caller makes sure that ref holds n elements.  ref / fcst follow `mem` (GPP_HOST_F64 honoured for both); *out is host
 * memory.  One radix sort of the (fcst, ref) pairs, then one sweep over the sorted order; up to 2^31 values.  The path override
 * GPP_MO_TILE = k (1 <= k <= GPP_MO_TILE_ITEMS) sets the elements a workgroup of the sweep takes; the result does not depend on it. */
#define GPP_MO_TILE_ITEMS 2048   /* elements of a workgroup of the sweep: 256 lanes with 8 each */
#define GPP_MO_GROUP 4           /* thresholds a workgroup of the sweep carries in registers */
int gpp_get_optimal_threshold(const float* ref, const float* fcst, long long n, float threshold, int metric, float* out, int mem);
/* gridpp::metric_optimizer_curve (metric_optimizer.cpp:105-127): the rule above for each of the num_thresholds thresholds, in order, with
 * ONE sort and the thresholds swept GPP_MO_GROUP to a workgroup; where the result x is valid, out_ref[k] = x and out_fcst[k] = the
 * threshold (the reference's naming), k counting the valid ones; *out_count = their number.  thresholds, out_ref, out_fcst (room for
 * num_thresholds values each) and out_count are host memory; ref / fcst follow `mem`.  num_thresholds == 0 and n == 0 need no device. */
int gpp_metric_optimizer_curve(const float* ref, const float* fcst, long long n, const float* thresholds, int num_thresholds, int metric,
                               float* out_ref, float* out_fcst, int* out_count, int mem);

/* ---- weather diagnostics and value transforms (include/gridpp.h:1249-1367,2345-2435) ----------------------------------------------
 * Element-wise over n values: every input array and `out` hold n floats and follow `mem` (GPP_MEM_HOST or GPP_MEM_DEVICE;
 * GPP_HOST_F64 honoured for ALL inputs of a call: they are then `const double*` and are rounded to float32 on the device as the first
 * operation).  The per-value arithmetic is gridpp_amd/csrc/pointwise.h (the reference's float / double promotions operation by
 * operation, transcendentals evaluated in double), shared with the host-only scalar forms below.  n == 0 returns GPP_OK and writes
 * nothing; n < 0 and a NULL array are GPP_EINVAL.  The sizes of the arrays are the caller's to compare (the reference's
 * std::invalid_argument texts are raised by the mirrors).  One streaming kernel: GPP_POINTWISE_BLOCK lanes per workgroup, at most
 * GPP_POINTWISE_MAX_BLOCKS workgroups walking the values with a grid stride, four values per lane and step through 16-byte loads
 * and stores where every pointer is 16-byte aligned (one value per lane otherwise, and for the n mod 4 tail). */
#define GPP_POINTWISE_BLOCK 256
#define GPP_POINTWISE_MAX_BLOCKS 2048
/* gridpp::dewpoint (src/api/humidity.cpp:5-32) */
int gpp_dewpoint(const float* temperature, const float* relative_humidity, long long n, float* out, int mem);
/* gridpp::relative_humidity (src/api/humidity.cpp:33-90) */
int gpp_relative_humidity(const float* temperature, const float* dewpoint, long long n, float* out, int mem);
/* gridpp::wetbulb (src/api/humidity.cpp:91-122) */
int gpp_wetbulb(const float* temperature, const float* pressure, const float* relative_humidity, long long n, float* out, int mem);
/* gridpp::pressure (src/api/pressure.cpp:5-26) */
int gpp_pressure(const float* ielev, const float* oelev, const float* ipressure, const float* itemperature, long long n, float* out, int mem);
/* gridpp::sea_level_pressure (src/api/pressure.cpp:28-93).  Where the reference throws for an element ("sea_level_pressure: altitude
 * is NAN", "sea_level_pressure: temperature is NAN", "sea_level_pressure: unphysical values in input", tested in that order) the call
 * returns GPP_ERUNTIME with the message of the LOWEST offending index (the reference throws inside an OpenMP loop); `out` is then
 * written all the same, with NaN at the offending elements. */
int gpp_sea_level_pressure(const float* ps, const float* altitude, const float* temperature, const float* rh, const float* dewpoint,
                           long long n, float* out, int mem);
/* gridpp::qnh (src/api/qnh.cpp:6-41) */
int gpp_qnh(const float* pressure, const float* altitude, long long n, float* out, int mem);
/* gridpp::wind_speed / wind_direction (src/api/wind.cpp:6-37) */
int gpp_wind_speed(const float* xwind, const float* ywind, long long n, float* out, int mem);
int gpp_wind_direction(const float* xwind, const float* ywind, long long n, float* out, int mem);
/* gridpp::Identity / Log / BoxCox / StartedBoxCox ::forward and ::backward over n values (src/api/transform.cpp:13-84 over :85-154,
 * 180-185).  p0 = threshold (BoxCox, StartedBoxCox), p1 = scaling_factor (StartedBoxCox); ignored otherwise.  GPP_EINVAL for a kind
 * that is none of the four, and for StartedBoxCox with the texts of its constructor (transform.cpp:128-131): "threshold parameter
 * must be > 0 in the started Box-Cox distribution", "Scaling factor parameter must be > 0 in the started Box-Cox distribution". */
#define GPP_TRANSFORM_IDENTITY 0
#define GPP_TRANSFORM_LOG 1
#define GPP_TRANSFORM_BOXCOX 2
#define GPP_TRANSFORM_STARTED_BOXCOX 3
int gpp_transform(const float* in, long long n, int kind, int backward, float p0, float p1, float* out, int mem);
/* Host-only forms (no GPU needed); they run the per-value source of the kernels.
 * The scalar overloads of the eight diagnostics (humidity.cpp:5-21,33-79,91-109, pressure.cpp:5-13,28-80, qnh.cpp:6-30, wind.cpp:6-8,
 * 20-26): args holds the nargs arguments in the reference's order; GPP_EINVAL for an unknown `which` or a wrong nargs;
 * GPP_DIAG_SEA_LEVEL_PRESSURE returns GPP_ERUNTIME with the three messages above. */
#define GPP_DIAG_DEWPOINT 0
#define GPP_DIAG_RELATIVE_HUMIDITY 1
#define GPP_DIAG_WETBULB 2
#define GPP_DIAG_PRESSURE 3
#define GPP_DIAG_SEA_LEVEL_PRESSURE 4
#define GPP_DIAG_QNH 5
#define GPP_DIAG_WIND_SPEED 6
#define GPP_DIAG_WIND_DIRECTION 7
int gpp_diagnostic_scalar(int which, const float* args, int nargs, float* out);
/* Transform::forward(float) / backward(float) of the four kinds (transform.cpp:85-154,180-185); errors as gpp_transform. */
int gpp_transform_scalar(float value, int kind, int backward, float p0, float p1, float* out);

/* ---- the gamma distribution (include/gridpp.h:573,2438-2455) -----------------------------------------------------------------------
 * Element-wise over n values like the entries above (`mem`, GPP_HOST_F64, n == 0, n < 0 and NULL as there).  The per-value arithmetic is
 * gridpp_amd/csrc/gamma_fn.h: the regularised incomplete gamma function, its inverse and the normal quantile in double, every loop
 * with a compile-time bound, shared with the host-only scalar forms below.  Where the reference raises through Boost's error policies
 * the entries return IEEE values, so they are no part of the reference-compatible surface.  One value per lane:
 * GPP_GAMMA_BLOCK lanes per workgroup, at most GPP_GAMMA_MAX_BLOCKS workgroups walking the values with a grid stride. */
#define GPP_GAMMA_BLOCK 256
#define GPP_GAMMA_MAX_BLOCKS 2048
/* gridpp::gamma_inv (src/api/distribution.cpp:5-33): out[i] = (float)(scale[i] * x) with P(shape[i], x) = levels[i]; 0 for level 0, +inf
 * for level 1.  GPP_EINVAL with the reference's texts for the lowest offending index, level before shape before scale: "Invalid level
 * '<v>'. Levels must be on the interval [0, 1].", "Invalid shape '<v>'. Shapes must be > 0.", "Invalid scale '<v>'. Scale must be > 0."
 * (<v> as an ostream prints a float).  The three arrays hold n values each: that is the caller's to make sure. */
int gpp_gamma_inv(const float* levels, const float* shape, const float* scale, long long n, float* out, int mem);
/* gridpp::Gamma::forward / backward over n values (src/api/transform.cpp:155-179 over :13-84).  forward: NaN for an invalid value and
 * for value + tolerance < 0, -inf / +inf where the float32 cdf is 0 / 1; backward: NaN for an invalid value, +inf where the float32
 * normal cdf is 1.  GPP_EINVAL with the texts of the constructor (transform.cpp:158-163): "Shape parameter must be > 0 in the gamma
 * distribution", "Scale parameter must be > 0 in the gamma distribution", "Tolerance must be >= 0 in the gamma distribution". */
int gpp_gamma_transform(const float* in, long long n, int backward, float shape, float scale, float tolerance, float* out, int mem);
/* Host-only forms (no GPU needed); they run the per-value source of the kernels.
 * gridpp::gamma_inv for one element (src/api/distribution.cpp:5-33); errors as gpp_gamma_inv. */
int gpp_gamma_inv_scalar(float level, float shape, float scale, float* out);
/* Gamma::forward(float) / backward(float) (src/api/transform.cpp:166-179); errors as gpp_gamma_transform. */
int gpp_gamma_transform_scalar(float value, int backward, float shape, float scale, float tolerance, float* out);

/* per-call statistics of the last OI call on this thread (diagnostics / bench) */
typedef struct gpp_oi_stats {
    long long cells;          /* grid cells processed */
    long long cells_updated;  /* cells with at least one usable observation */
    long long solves;         /* local (P+R) factorisations actually performed */
    long long fallback_tiles; /* tiles k_oi_union handed to k_oi (or all tiles when the call was redone with the pivoted LU) */
    float kernel_ms;          /* hipEvent time of the OI kernel(s) on the library stream.  Host-array calls on the banded path (a grid of >= 2^20 cells
                               * that takes the tile kernel): each band's launch waits for the band's upload, so this and union_kernel_ms
                               * include the host-to-device copies of the background; device-array calls: kernel time alone */
    float union_kernel_ms;    /* of which k_oi_union, first pass (one factorisation per tile); 0 when that kernel was not used */
    long long fallback_subtiles; /* work items (4 cells, or whole tiles) k_oi_union's list passes left to k_oi */
    long long big_cells;      /* grid points with more than 62 usable observations (done by k_oi_big) */
    long long bulk_certified; /* of `solves`: work items of k_oi_union whose bulk disc was certified (every per-candidate test decided once per item);
                               * 0 under GPP_OI_NO_BULK_CERT, with elevation / land-fraction factors, and on k_oi_union_pair / k_oi_union_sp */
    /* The pair table of the observation set (csrc/oi_pair_table.h): for a scalar Barnes structure on a 2-D grid, k_oi_union takes the pair
     * correlations of P from a table kept with the Points handle, built by the first call with that structure and window.  It is a cache: a
     * work item that meets a pair the table does not hold evaluates its P as without it.  Path overrides: GPP_OI_NO_PAIR_TABLE (none is built
     * or used), GPP_OI_PAIR_WINDOW = n (a window of n bins instead of the estimate).  The result depends on neither. */
    int pair_window;          /* half-width of the table's window in bins of the observation index; 0: no table was used */
    long long pair_table_bytes;    /* its size; at most 128 MiB (the window shrinks to fit) */
    long long pair_fallback_items; /* work items of k_oi_union that redid their P build by evaluation */
    float pair_table_build_ms;     /* host time of the build inside this call; 0 when the cached table was used */
} gpp_oi_stats;
int gpp_oi_last_stats(gpp_oi_stats* stats);
/* diagnostics: the two coordinate axes (0 = x, 1 = y, 2 = z; the two of largest extent) on which the observation index of `points` is binned --
 * the axes along which optimal_interpolation's tile kernels take a tile's extent.  Builds the index when the set has none yet. */
int gpp_debug_obs_axes(gpp_points* points, int* axis_a, int* axis_b);
/* Diagnostics: the bin layout of that index: dims[3] = {nbx, nby, 1 if the index was built on the device}, geom[3] = {amin, bmin, inv_s}, and
 * the first min(cap, nbx * nby + 1) entries of its bin_start (bin_start may be NULL). */
int gpp_debug_obs_index(gpp_points* points, int* dims, float* geom, int* bin_start, int cap);

/* Asynchronous optimal interpolation (no counterpart in the reference, whose calls return their result; this is for a caller that streams
 * analyses -- one per observation set -- through one GPU, e.g. a rank of the multi-GPU tiling, src/api/oi.cpp:221-338 has no state between
 * calls).  gpp_optimal_interpolation_full(..., mem = GPP_MEM_DEVICE | GPP_ASYNC) enqueues the call on the library stream and returns; every
 * such call is completed, in order, by ONE gpp_wait() of the same thread, which returns the status of that call (the results are in `out`
 * when it returns GPP_OK; gpp_oi_last_stats() then describes that call).  Only a call in the steady state of a repeated analysis (the same
 * Grid / Points handles as the call before) is really deferred; any other runs synchronously at once and its gpp_wait() returns immediately.
 * Until the wait returns the caller keeps inputs, outputs and handles alive and unchanged; at most 4 calls are deferred at a time (further
 * ones run synchronously).  gpp_pending() tells how many waits are outstanding.  A GPP_ASYNC call that returns an error (bad arguments, out
 * of memory: nothing was enqueued) is queued as a completed call too, so a caller may pair one gpp_wait() with every submission without looking
 * at the return code of the submission; that wait returns the same code and message again. */
int gpp_wait(void);
int gpp_pending(int* count);

/* ---- the reusable OI gain (no counterpart in the reference; gridpp_amd/csrc/oi_gain.hip) -----------------------------
 * In a loop of optimal_interpolation calls over ensemble members, hours or perturbed observations the grid, the stations, the ratios, the
 * structure function and max_points stay the same and only values change.  The candidate scan and the factorisation depend on none of the
 * values (src/api/oi.cpp:229-317): a gain holds their result -- for every background point the observations the reference would select,
 * their weights w = G (P + R)^-1 as doubles and a = w . g -- and analyses any number of fields with it:
 *     out[cell, e] = background[cell, e] + clamp(sum_k w[cell, k] * d[idx[cell, k], e]),   d = (double) pobs - (double) pbackground
 * (the sum in double, the clamp of oi.cpp:318-334 over the selected d of that cell and field when allow_extrapolation is 0, the cast to
 * float32 last; an invalid background value and a cell without a selection pass through).  A gain holds about cells * max_points * 12
 * bytes of HBM until gpp_oi_gain_destroy; it copies what it needs, so the Grid, Points and structure it was built from may be destroyed
 * first, and it shares no workspace with the OI calls (which may run, GPP_ASYNC or not, between its operations).  GPP_ASYNC is ignored here. */
#define GPP_OI_GAIN_MAX_POINTS 62   /* what the register-tile kernels of optimal_interpolation serve; a lane of a wave per column */
typedef struct gpp_oi_gain gpp_oi_gain;
/* pratios: S host floats -- the `pratios` of optimal_interpolation; a caller of optimal_interpolation_full passes obs_variance /
 * bvariance_at_points divided in float32 (oi.cpp:194).  usable: S host bytes, NULL = every station; a station with missing values in ANY of
 * the fields to come is marked unusable here (the reference drops it per call, oi.cpp:252).  GPP_EINVAL before any device work: differing
 * coordinate types (the text of oi.cpp:155-157), max_points < 1 (a gain has max_points columns per cell: 0, "no limit", has no fixed
 * width), max_points > GPP_OI_GAIN_MAX_POINTS.  No observations, or none usable: a valid gain without selections.  GPP_ERUNTIME for an
 * exactly singular local system, as gpp_optimal_interpolation_full on the same inputs. */
int gpp_oi_gain_create(gpp_points* bgrid, gpp_points* points, const float* pratios, const unsigned char* usable,
                       const gpp_structure* structure, int max_points, gpp_oi_gain** gain);
/* background, out: [cells][ne] (gridpp's cube layout, the field index innermost: (Y, X, E) or (N, E)); pbackground: [S][ne]; pobs: [S]
 * (pobs_per_field 0) or [S][ne]; `mem` as everywhere, GPP_HOST_F64 for the three inputs.  GPP_EINVAL naming the lowest offending
 * (field, station) when pobs or pbackground is invalid at a usable station.  From 16 fields on a wave runs along the fields of a cell. */
int gpp_oi_gain_apply(gpp_oi_gain* gain, const float* background, int ne, const float* pobs, int pobs_per_field, const float* pbackground,
                      int allow_extrapolation, float* out, int mem);
/* the analysis variance of optimal_interpolation_full: bvariance * (1 - a) where the cell has a selection, bvariance elsewhere */
int gpp_oi_gain_variance(gpp_oi_gain* gain, const float* bvariance, float* out, int mem);
/* any pointer may be NULL; bytes: the HBM the gain holds now (the planes and the innovation table of its last apply) */
int gpp_oi_gain_info(const gpp_oi_gain* gain, long long* cells, int* stations, int* max_points, long long* bytes, int* largest_selection);
/* counts[cells] (int), indices[cells][max_points] (int, the caller's observation order, ascending, -1 behind the selection),
 * weights[cells][max_points] (double, 0 behind the selection); any of them may be NULL; `mem`: where the three arrays live */
int gpp_oi_gain_selection(gpp_oi_gain* gain, int* counts, int* indices, double* weights, int mem);
int gpp_oi_gain_destroy(gpp_oi_gain* gain);

/* ---- the reusable downscaling plan (no counterpart in the reference; gridpp_amd/csrc/downscale_plan.hip) -------------
 * nearest, bilinear, simple_gradient and full_gradient start with the same value-independent work: the nearest grid point of every output
 * location and, for Bilinear, its box (Grid::get_box) and the weights (s, t).  A plan holds the result -- 4 bytes per output location for
 * Nearest, one 16-byte record for Bilinear -- and downscales any number of fields with it; every result is, bit for bit, that of the
 * direct call on the same inputs.  A plan copies what it needs (the records, and the elevations and land area fractions of both sets for
 * the gradient methods), so the Grid / Points it was built from may be destroyed first.  GPP_ASYNC is ignored here. */
typedef struct gpp_downscale_plan gpp_downscale_plan;
/* igrid: a Grid; to: a Grid or Points; downscaler: 0 Nearest, 1 Bilinear.  GPP_EINVAL before any device work: a NULL handle, an input that
 * is no Grid, "Invalid downscaler", and for Nearest "Coordinate types must be the same".  A box whose weights leave [0, 1] never fails the
 * construction: it is counted (gpp_downscale_plan_info: distorted), and an apply raises "Problem with bilinear interpolation..."
 * (GPP_ERUNTIME) exactly where the direct call would -- when one of the fields it downscales has four valid corners at such a location. */
int gpp_downscale_plan_create(gpp_points* igrid, gpp_points* to, int downscaler, gpp_downscale_plan** plan);
/* values [nt][Y * X] -> out [nt][locations]: gpp_nearest_levels / gpp_bilinear.  `mem` as everywhere (GPP_HOST_F64 for values). */
int gpp_downscale_plan_apply(gpp_downscale_plan* plan, const float* values, int nt, float* out, int mem);
/* values [Y * X][ne] -> out [locations][ne] (gridpp's cube layout, the member index innermost): plane e is gpp_nearest_levels /
 * gpp_bilinear of plane e; for Bilinear the four-corner validity test is per member and location.  Any ne >= 0. */
int gpp_downscale_plan_apply_cube(gpp_downscale_plan* plan, const float* values, int ne, float* out, int mem);
/* gpp_simple_gradient / gpp_full_gradient with the plan's geometries and downscaler (elev_gradient / laf_gradient NULL: term absent) */
int gpp_downscale_plan_simple_gradient(gpp_downscale_plan* plan, const float* values, int nt, float elev_gradient, float* out, int mem);
int gpp_downscale_plan_full_gradient(gpp_downscale_plan* plan, const float* values, int nt, const float* elev_gradient,
                                     const float* laf_gradient, float* out, int mem);
/* The gradient methods on gridpp's cube layout: values [Y * X][ne] -> out [locations][ne]; plane e is gpp_simple_gradient /
 * gpp_full_gradient of plane e, bit for bit.  A gradient is NULL (term absent), one field [Y * X] shared by the members (`*_members` 1) or a
 * cube [Y * X][ne] (`*_members` ne); any other count is GPP_EINVAL.  NULL handles, a negative ne, an empty input grid (all NaN), no
 * location or no member (nothing to do) and GPP_ASYNC as gpp_downscale_plan_apply_cube. */
int gpp_downscale_plan_simple_gradient_cube(gpp_downscale_plan* plan, const float* values, int ne, float elev_gradient, float* out, int mem);
int gpp_downscale_plan_full_gradient_cube(gpp_downscale_plan* plan, const float* values, int ne, const float* elev_gradient, int elev_members,
                                          const float* laf_gradient, int laf_members, float* out, int mem);
/* gpp_downscale_probability / gpp_mask_threshold_downscale with the nearest input cells of a plan whose output is a Grid, bit for bit
 * (RandomChoice draws anew every call) and without a search.  GPP_EINVAL before any device work: a NULL handle, a plan built for Points,
 * "Coordinate types must be the same" (a Bilinear plan may span two), then the checks of the direct entries in their order.  A Bilinear
 * plan extracts the nearest grid points of its records on the first such call and keeps them: 4 more bytes per location in `bytes`. */
int gpp_downscale_plan_probability(gpp_downscale_plan* plan, const float* values, int ne, const float* threshold, int comparison_operator,
                                   float* out, int mem);
int gpp_downscale_plan_mask_threshold(gpp_downscale_plan* plan, const float* ivalues_true, const float* ivalues_false,
                                      const float* threshold_values, int ne, const float* threshold, int comparison_operator, int statistic,
                                      float quantile, float* out, int mem);
/* any pointer may be NULL; cells: points of the input grid; bytes: the HBM the plan holds; distorted: locations whose weights leave [0, 1] */
int gpp_downscale_plan_info(const gpp_downscale_plan* plan, long long* locations, long long* cells, int* downscaler, long long* bytes,
                            long long* distorted);
int gpp_downscale_plan_destroy(gpp_downscale_plan* plan);

#ifdef __cplusplus
}
#endif
#endif
