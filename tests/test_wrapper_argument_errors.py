"""CPU: what the wrappers that have no *_api.py file of their own do with their arguments before any device work -- one table of calls.

Every row carries one literal expectation: the exception type and its exact text; for empty inputs the shape of the float32 array
that comes back; or NO_DEVICE for a valid call, which passes every check and reaches the library ("no HIP device visible" where none
is; where one is, the call simply works).  The rows named *_first have two failing checks and pin which one is raised."""
import numpy as np
import pytest

NO_DEVICE = object()
# the library's own refusal, or the HIP runtime's where an older entry point meets it first in an allocation
NO_DEVICE_TEXT = "no HIP device visible|no ROCm-capable device is detected"


@pytest.fixture(scope="module")
def gridpp():
    import __graft_entry__ as g
    g.build()
    import gridpp_amd
    return gridpp_amd


class Case:
    """the arguments the rows share: a 3 x 4 grid, 5 points and fields on them"""

    def __init__(self, gp):
        lons, lats = np.meshgrid(np.arange(4) * 0.1, 60 + np.arange(3) * 0.1)
        self.g = gp.Grid(lats, lons, np.zeros((3, 4)), np.full((3, 4), 0.5))
        self.gc = gp.Grid(lats, lons, np.zeros((3, 4)), np.full((3, 4), 0.5), gp.Cartesian)
        self.g0 = gp.Grid()
        self.p = gp.Points(60 + np.arange(5) * 0.05, np.arange(5) * 0.07, np.zeros(5), np.zeros(5))
        self.pc = gp.Points(60 + np.arange(5) * 0.05, np.arange(5) * 0.07, np.zeros(5), np.zeros(5), gp.Cartesian)
        self.p0 = gp.Points([], [])
        self.v = np.arange(12, dtype=np.float32).reshape(3, 4)      # a field on the grid
        self.vt = np.zeros((4, 3), np.float32)                      # ... of the wrong shape
        self.c = np.zeros((3, 4, 2), np.float32)                    # an ensemble on the grid
        self.pv = np.arange(5, dtype=np.float32)                    # values at the points
        self.pe = np.zeros((5, 2), np.float32)                      # an ensemble at the points
        self.st = gp.BarnesStructure(10000)


Z = np.zeros
RE, VE, TE = RuntimeError, ValueError, TypeError
GRID_VALUES = "Grid size is not the same as values"
OI_TYPES = "bgrid must be a Grid or Points, points a Points"
OI_COORDS = "Both background and observations points must be of same coordinate type (lat/lon or x/y)"

# (id, call(gridpp, case), expectation)
ROWS = [
    # nearest
    ("nearest_rank", lambda gp, k: gp.nearest(k.g, k.p, Z(3)), (RE, "values must have 2 or 3 dimensions")),
    ("nearest_rank_points", lambda gp, k: gp.nearest(k.p, k.p, Z((2, 2, 2))), (RE, "values must have 1 or 2 dimensions")),
    ("nearest_size", lambda gp, k: gp.nearest(k.g, k.p, k.vt), (VE, GRID_VALUES)),
    ("nearest_size_levels", lambda gp, k: gp.nearest(k.g, k.p, Z((2, 4, 3))), (VE, GRID_VALUES)),
    ("nearest_size_points", lambda gp, k: gp.nearest(k.p, k.g, Z(4)), (VE, "Points size is not the same as values")),
    ("nearest_no_rows_to_read", lambda gp, k: gp.nearest(k.g, k.p, Z((0, 4))), (VE, GRID_VALUES)),
    ("nearest_size_first", lambda gp, k: gp.nearest(k.g, k.p0, k.vt), (VE, GRID_VALUES)),
    ("nearest_empty_output", lambda gp, k: gp.nearest(k.g, k.p0, k.v), (0,)),
    ("nearest_empty_output_no_rows", lambda gp, k: gp.nearest(k.g, k.p0, Z((0, 4))), (0,)),
    ("nearest_no_levels", lambda gp, k: gp.nearest(k.g, k.p, Z((0, 3, 4))), (0, 5)),
    ("nearest_empty_list", lambda gp, k: gp.nearest(k.g, k.p0, []), (0,)),
    ("nearest_valid", lambda gp, k: gp.nearest(k.g, k.p, k.v), NO_DEVICE),
    ("nearest_valid_points", lambda gp, k: gp.nearest(k.p, k.g, k.pv), NO_DEVICE),
    # bilinear
    ("bilinear_input", lambda gp, k: gp.bilinear(k.p, k.p, k.pv), (TE, "bilinear: the input must be a Grid")),
    ("bilinear_input_first", lambda gp, k: gp.bilinear(k.p, k.p, Z((2, 2, 2, 2))), (TE, "bilinear: the input must be a Grid")),
    ("bilinear_rank", lambda gp, k: gp.bilinear(k.g, k.p, Z(3)), (RE, "bilinear: values must be 2-D or 3-D")),
    ("bilinear_empty_list", lambda gp, k: gp.bilinear(k.g, k.p0, []), (RE, "bilinear: values must be 2-D or 3-D")),
    ("bilinear_size", lambda gp, k: gp.bilinear(k.g, k.p, k.vt), (VE, GRID_VALUES)),
    ("bilinear_no_rows_to_read", lambda gp, k: gp.bilinear(k.g, k.g, Z((2, 0, 4))), (VE, GRID_VALUES)),
    ("bilinear_size_first", lambda gp, k: gp.bilinear(k.g, k.p0, k.vt), (VE, GRID_VALUES)),
    ("bilinear_empty_output", lambda gp, k: gp.bilinear(k.g, k.g0, k.v), (0, 0)),
    ("bilinear_no_levels", lambda gp, k: gp.bilinear(k.g, k.g, Z((0, 3, 4))), (0, 3, 4)),
    ("bilinear_valid", lambda gp, k: gp.bilinear(k.g, k.p, k.v), NO_DEVICE),
    # gridding, gridding_nearest
    ("gridding_rank", lambda gp, k: gp.gridding(k.g, k.p, Z((5, 1)), 1000, 0, gp.Mean), (RE, "values must have 1 dimensions, got 2")),
    ("gridding_size", lambda gp, k: gp.gridding(k.g, k.p, Z(4), 1000, 0, gp.Mean), (VE, "Points size is not the same as values")),
    ("gridding_radius", lambda gp, k: gp.gridding(k.g, k.p, k.pv, -1, 0, gp.Mean), (VE, "radius must be >= 0")),
    ("gridding_radius_nan", lambda gp, k: gp.gridding(k.g, k.p, k.pv, np.nan, 0, gp.Mean), (VE, "radius must be >= 0")),
    ("gridding_min_num", lambda gp, k: gp.gridding(k.g, k.p, k.pv, 1000, -1, gp.Mean), (VE, "min_num must be >= 0")),
    ("gridding_size_first", lambda gp, k: gp.gridding(k.g, k.p, Z(4), -1, -1, gp.Mean), (VE, "Points size is not the same as values")),
    ("gridding_radius_first", lambda gp, k: gp.gridding(k.g, k.p, k.pv, -1, -1, gp.Mean), (VE, "radius must be >= 0")),
    ("gridding_empty_grid", lambda gp, k: gp.gridding(k.g0, k.p, k.pv, 1000, 0, gp.Mean), (0, 0)),
    ("gridding_empty_points_output", lambda gp, k: gp.gridding(k.p0, k.p, k.pv, 1000, 0, gp.Mean), (0,)),
    ("gridding_valid", lambda gp, k: gp.gridding(k.g, k.p, k.pv, 1000, 0, gp.Mean), NO_DEVICE),
    ("gridding_nearest_rank", lambda gp, k: gp.gridding_nearest(k.g, k.p, Z((5, 1)), 0, gp.Mean), (RE, "values must have 1 dimensions, got 2")),
    ("gridding_nearest_size", lambda gp, k: gp.gridding_nearest(k.g, k.p, Z(6), 0, gp.Mean), (VE, "Points size is not the same as values")),
    ("gridding_nearest_min_num", lambda gp, k: gp.gridding_nearest(k.g, k.p, k.pv, -1, gp.Mean), (VE, "min_num must be >= 0")),
    ("gridding_nearest_size_first", lambda gp, k: gp.gridding_nearest(k.g, k.p, Z(6), -1, gp.Mean), (VE, "Points size is not the same as values")),
    ("gridding_nearest_all_empty", lambda gp, k: gp.gridding_nearest(k.g0, k.p0, [], 0, gp.Mean), (0, 0)),
    ("gridding_nearest_valid", lambda gp, k: gp.gridding_nearest(k.g, k.p, k.pv, 1, gp.Mean), NO_DEVICE),
    # fill, fill_missing
    ("fill_rank", lambda gp, k: gp.fill(k.g, Z(3), k.p, np.ones(5), 0, True), (RE, "values must have 2 dimensions, got 1")),
    ("fill_size", lambda gp, k: gp.fill(k.g, k.vt, k.p, np.ones(5), 0, True), (VE, GRID_VALUES)),
    ("fill_radii", lambda gp, k: gp.fill(k.g, k.v, k.p, np.ones(4), 0, True), (VE, "Points size is not the same as radii size")),
    ("fill_size_first", lambda gp, k: gp.fill(k.g, k.vt, k.p, np.ones(4), 0, True), (VE, GRID_VALUES)),
    ("fill_no_rows", lambda gp, k: gp.fill(k.g, Z((0, 4)), k.p, np.ones(5), 0, True), (0, 4)),
    ("fill_one_empty_row", lambda gp, k: gp.fill(k.g, [[]], k.p, np.ones(5), 0, True), (VE, GRID_VALUES)),
    ("fill_empty_list", lambda gp, k: gp.fill(k.g, [], k.p, np.ones(5), 0, True), (0, 0)),
    ("fill_valid", lambda gp, k: gp.fill(k.g, k.v, k.p, np.ones(5), 0, True), NO_DEVICE),
    ("fill_missing_rank", lambda gp, k: gp.fill_missing(Z(3)), (RE, "values must have 2 dimensions, got 1")),
    ("fill_missing_rank3", lambda gp, k: gp.fill_missing(k.c), (RE, "values must have 2 dimensions, got 3")),
    ("fill_missing_empty", lambda gp, k: gp.fill_missing([[]]), (1, 0)),
    ("fill_missing_empty_list", lambda gp, k: gp.fill_missing([]), (0, 0)),
    ("fill_missing_no_columns", lambda gp, k: gp.fill_missing(Z((3, 0))), (3, 0)),
    ("fill_missing_valid", lambda gp, k: gp.fill_missing(k.v), NO_DEVICE),
    # doping_square, doping_circle
    ("doping_square_rank", lambda gp, k: gp.doping_square(k.g, Z(3), k.p, k.pv, [1] * 5), (RE, "observations must have 2 dimensions, got 1")),
    ("doping_square_size", lambda gp, k: gp.doping_square(k.g, k.vt, k.p, k.pv, [1] * 5), (VE, "Grid size is not the same as observations")),
    ("doping_square_obs_rank", lambda gp, k: gp.doping_square(k.g, k.v, k.p, k.pe, [1] * 5), (RE, "observations must have 1 dimensions, got 2")),
    ("doping_square_obs", lambda gp, k: gp.doping_square(k.g, k.v, k.p, Z(4), [1] * 5), (VE, "Points size is not the same as observations size")),
    ("doping_square_halfwidth", lambda gp, k: gp.doping_square(k.g, k.v, k.p, k.pv, [1] * 4), (VE, "Points size is not the same as halfwidth size")),
    ("doping_square_obs_first", lambda gp, k: gp.doping_square(k.g, k.v, k.p, Z(4), [1] * 4), (VE, "Points size is not the same as observations size")),
    ("doping_square_no_rows", lambda gp, k: gp.doping_square(k.g, Z((0, 4)), k.p, k.pv, [1] * 5), (0, 4)),
    ("doping_square_valid", lambda gp, k: gp.doping_square(k.g, k.v, k.p, k.pv, [1] * 5), NO_DEVICE),
    ("doping_circle_size", lambda gp, k: gp.doping_circle(k.g, k.vt, k.p, k.pv, np.ones(5)), (VE, "Grid size is not the same as observations")),
    ("doping_circle_obs", lambda gp, k: gp.doping_circle(k.g, k.v, k.p, Z(6), np.ones(5)), (VE, "Points size is not the same as observations size")),
    ("doping_circle_radii", lambda gp, k: gp.doping_circle(k.g, k.v, k.p, k.pv, np.ones(6)), (VE, "Points size is not the same as radii size")),
    ("doping_circle_size_first", lambda gp, k: gp.doping_circle(k.g, k.vt, k.p, Z(6), np.ones(6)), (VE, "Grid size is not the same as observations")),
    ("doping_circle_empty_list", lambda gp, k: gp.doping_circle(k.g, [], k.p, k.pv, np.ones(5)), (0, 0)),
    ("doping_circle_valid", lambda gp, k: gp.doping_circle(k.g, k.v, k.p, k.pv, np.ones(5), 100.0), NO_DEVICE),
    # neighbourhood_search
    ("search_rank", lambda gp, k: gp.neighbourhood_search(Z(3), k.v, 1, 0, 1, 0.5), (RE, "array must have 2 dimensions, got 1")),
    ("search_rank_search_array", lambda gp, k: gp.neighbourhood_search(k.v, k.c, 1, 0, 1, 0.5), (RE, "search_array must have 2 dimensions, got 3")),
    ("search_size", lambda gp, k: gp.neighbourhood_search(k.v, k.vt, 1, 0, 1, 0.5), (VE, "search_array must either be the same size as array")),
    ("search_targets", lambda gp, k: gp.neighbourhood_search(k.v, k.v, 1, 2, 1, 0.5), (VE, "Search_target_min must be smaller than search_target_max")),
    ("search_halfwidth", lambda gp, k: gp.neighbourhood_search(k.v, k.v, -1, 0, 1, 0.5), (VE, "halfwidth must be positive")),
    ("search_apply_array", lambda gp, k: gp.neighbourhood_search(k.v, k.v, 1, 0, 1, 0.5, Z((4, 3), np.int32)),
     (VE, "apply_array must either be empty or same size as array")),
    ("search_size_first", lambda gp, k: gp.neighbourhood_search(k.v, k.vt, -1, 2, 1, 0.5), (VE, "search_array must either be the same size as array")),
    ("search_targets_first", lambda gp, k: gp.neighbourhood_search(k.v, k.v, -1, 2, 1, 0.5, Z((4, 3))),
     (VE, "Search_target_min must be smaller than search_target_max")),
    ("search_empty", lambda gp, k: gp.neighbourhood_search([[]], [[]], 1, 0, 1, 0.5), (1, 0)),
    ("search_empty_list", lambda gp, k: gp.neighbourhood_search([], [], 1, 0, 1, 0.5), (0, 0)),
    ("search_valid", lambda gp, k: gp.neighbourhood_search(k.v, k.v, 1, 0, 1, 0.5), NO_DEVICE),
    ("search_valid_apply_array", lambda gp, k: gp.neighbourhood_search(k.v, k.v, 1, 0, 1, 0.5, np.ones((3, 4))), NO_DEVICE),
    ("search_valid_empty_apply_array", lambda gp, k: gp.neighbourhood_search(k.v, k.v, 1, 0, 1, 0.5, [[]]), NO_DEVICE),
    # calc_gradient
    ("gradient_rank", lambda gp, k: gp.calc_gradient(Z(3), k.v, gp.LinearRegression, 1), (RE, "base must have 2 dimensions, got 1")),
    ("gradient_rank_values", lambda gp, k: gp.calc_gradient(k.v, k.c, gp.LinearRegression, 1), (RE, "values must have 2 dimensions, got 3")),
    ("gradient_halfwidth", lambda gp, k: gp.calc_gradient(k.v, k.v, gp.MinMax, 0), (VE, "Halwidth cannot be <= 0; must be positive integer")),
    ("gradient_min_range", lambda gp, k: gp.calc_gradient(k.v, k.v, gp.MinMax, 1, 2, -1), (VE, "min_range must be >= 0")),
    ("gradient_num_min", lambda gp, k: gp.calc_gradient(k.v, k.v, gp.MinMax, 1, -1), (VE, "num_min must be >= 0")),
    ("gradient_no_size", lambda gp, k: gp.calc_gradient([], [], gp.MinMax, 1), (VE, "base input has no size")),
    ("gradient_size", lambda gp, k: gp.calc_gradient(k.v, k.vt, gp.MinMax, 1), (VE, "base is not the same size as values")),
    ("gradient_halfwidth_first", lambda gp, k: gp.calc_gradient(k.v, k.vt, gp.MinMax, 0, -1, -1), (VE, "Halwidth cannot be <= 0; must be positive integer")),
    ("gradient_no_size_first", lambda gp, k: gp.calc_gradient([], k.v, gp.MinMax, 1), (VE, "base input has no size")),
    ("gradient_valid", lambda gp, k: gp.calc_gradient(k.v, k.v, gp.LinearRegression, 1, 2, 0.0, -0.0065), NO_DEVICE),
    # neighbourhood, neighbourhood_brute_force, neighbourhood_quantile, neighbourhood_quantile_fast
    ("neighbourhood_rank", lambda gp, k: gp.neighbourhood(Z(3), 1, gp.Mean), (RE, "input must have 2 or 3 dimensions")),
    ("neighbourhood_halfwidth", lambda gp, k: gp.neighbourhood(k.v, -1, gp.Mean), (VE, "Half width must be > 0")),
    ("neighbourhood_quantile_statistic", lambda gp, k: gp.neighbourhood(k.v, 1, gp.Quantile),
     (VE, "Use neighbourhood_quantile for computing neighbourhood quantiles")),
    ("neighbourhood_halfwidth_first", lambda gp, k: gp.neighbourhood(k.v, -1, gp.Quantile), (VE, "Half width must be > 0")),
    ("neighbourhood_rank_first", lambda gp, k: gp.neighbourhood(Z((2, 2, 2, 2)), -1, gp.Mean), (RE, "input must have 2 or 3 dimensions")),
    ("neighbourhood_empty", lambda gp, k: gp.neighbourhood([[]], 1, gp.Mean), (0, 0)),
    ("neighbourhood_empty_list", lambda gp, k: gp.neighbourhood([], 1, gp.Mean), (0, 0)),
    ("neighbourhood_no_members", lambda gp, k: gp.neighbourhood(Z((3, 4, 0)), 1, gp.Mean), (0, 0)),
    ("neighbourhood_valid", lambda gp, k: gp.neighbourhood(k.v, 1, gp.Mean), NO_DEVICE),
    ("neighbourhood_valid_ensemble", lambda gp, k: gp.neighbourhood(k.c, 1, gp.Max), NO_DEVICE),
    ("brute_force_rank", lambda gp, k: gp.neighbourhood_brute_force(Z(3), 1, gp.Mean), (RE, "input must have 2 or 3 dimensions")),
    ("brute_force_halfwidth", lambda gp, k: gp.neighbourhood_brute_force(k.v, -1, gp.Mean), (VE, "Half width must be > 0")),
    ("brute_force_rank_first", lambda gp, k: gp.neighbourhood_brute_force(Z(3), -1, gp.Mean), (RE, "input must have 2 or 3 dimensions")),
    ("brute_force_empty", lambda gp, k: gp.neighbourhood_brute_force([[]], 1, gp.Mean), (0, 0)),
    ("brute_force_valid", lambda gp, k: gp.neighbourhood_brute_force(k.v, 1, gp.Median), NO_DEVICE),
    ("quantile_rank", lambda gp, k: gp.neighbourhood_quantile(Z(3), 0.5, 1), (RE, "input must have 2 or 3 dimensions")),
    ("quantile_halfwidth", lambda gp, k: gp.neighbourhood_quantile(k.v, 0.5, -1), (VE, "Half width must be > 0")),
    ("quantile_rank_first", lambda gp, k: gp.neighbourhood_quantile(Z(3), 0.5, -1), (RE, "input must have 2 or 3 dimensions")),
    ("quantile_empty", lambda gp, k: gp.neighbourhood_quantile([[]], 0.5, 1), (0, 0)),
    ("quantile_valid", lambda gp, k: gp.neighbourhood_quantile(k.c, 0.5, 1), NO_DEVICE),
    ("quantile_fast_rank", lambda gp, k: gp.neighbourhood_quantile_fast(Z(3), 0.5, 1, [0, 1]), (RE, "input must have 2 or 3 dimensions")),
    ("quantile_fast_halfwidth", lambda gp, k: gp.neighbourhood_quantile_fast(k.v, 0.5, -1, [0, 1]), (VE, "Half width must be > 0")),
    ("quantile_fast_quantile_rank", lambda gp, k: gp.neighbourhood_quantile_fast(k.v, [0.5], 1, [0, 1]), (RE, "quantile must have 2 dimensions, got 1")),
    ("quantile_fast_quantile_size", lambda gp, k: gp.neighbourhood_quantile_fast(k.v, k.vt, 1, [0, 1]),
     (VE, "Quantile must be the same size as input, or size (1, 1)")),
    ("quantile_fast_thresholds_rank", lambda gp, k: gp.neighbourhood_quantile_fast(k.v, 0.5, 1, [[0, 1]]), (RE, "thresholds must have 1 dimensions, got 2")),
    ("quantile_fast_halfwidth_first", lambda gp, k: gp.neighbourhood_quantile_fast(k.v, k.vt, -1, [[0, 1]]), (VE, "Half width must be > 0")),
    ("quantile_fast_quantile_first", lambda gp, k: gp.neighbourhood_quantile_fast(k.v, k.vt, 1, [[0, 1]]),
     (VE, "Quantile must be the same size as input, or size (1, 1)")),
    ("quantile_fast_empty", lambda gp, k: gp.neighbourhood_quantile_fast([[]], k.vt, 1, [[0, 1]]), (0, 0)),
    ("quantile_fast_valid", lambda gp, k: gp.neighbourhood_quantile_fast(k.v, 0.5, 1, [0, 5, 10]), NO_DEVICE),
    ("quantile_fast_valid_field", lambda gp, k: gp.neighbourhood_quantile_fast(k.c, np.full((3, 4), 0.5), 1, [0, 5, 10]), NO_DEVICE),
    ("quantile_fast_valid_one_by_one", lambda gp, k: gp.neighbourhood_quantile_fast(k.v, [[0.5]], 1, [0, 5, 10]), NO_DEVICE),
    # calc_statistic, calc_quantile
    ("statistic_rank", lambda gp, k: gp.calc_statistic(k.c, gp.Mean), (RE, "array must have 1 or 2 dimensions")),
    ("statistic_valid_scalar", lambda gp, k: gp.calc_statistic(1.0, gp.Mean), NO_DEVICE),     # (numpy makes it a vector of one)
    ("statistic_no_rows", lambda gp, k: gp.calc_statistic(Z((0, 3)), gp.Mean), (0,)),
    ("statistic_valid", lambda gp, k: gp.calc_statistic(k.pv, gp.Mean), NO_DEVICE),
    ("statistic_valid_rows", lambda gp, k: gp.calc_statistic(k.v, gp.Median), NO_DEVICE),
    ("quantile_of_rank", lambda gp, k: gp.calc_quantile(Z((2, 2, 2, 2)), 0.5), (RE, "array must have 1, 2 or 3 dimensions")),
    ("quantile_of_valid_scalar", lambda gp, k: gp.calc_quantile(1.0, 0.5), NO_DEVICE),
    ("quantile_of_size", lambda gp, k: gp.calc_quantile(k.c, Z((4, 3))), (VE, "Dimension mismatch between array and quantile")),
    ("quantile_of_scalar_for_cube", lambda gp, k: gp.calc_quantile(k.c, 0.5), (VE, "Dimension mismatch between array and quantile")),
    ("quantile_of_rank_first", lambda gp, k: gp.calc_quantile(Z((2, 2, 2, 2)), Z((4, 3))), (RE, "array must have 1, 2 or 3 dimensions")),
    ("quantile_of_no_rows", lambda gp, k: gp.calc_quantile(Z((0, 3)), 0.5), (0,)),
    ("quantile_of_no_cells", lambda gp, k: gp.calc_quantile(Z((0, 0, 3)), Z((0, 0))), (0, 0)),
    ("quantile_of_valid", lambda gp, k: gp.calc_quantile(k.pv, 0.5), NO_DEVICE),
    ("quantile_of_valid_rows", lambda gp, k: gp.calc_quantile(k.v, 0.5), NO_DEVICE),
    ("quantile_of_valid_cube", lambda gp, k: gp.calc_quantile(k.c, np.full((3, 4), 0.5)), NO_DEVICE),
    # optimal_interpolation, optimal_interpolation_full
    ("oi_max_points", lambda gp, k: gp.optimal_interpolation(k.g, k.v, k.p, k.pv, k.pv, k.pv, k.st, -1), (VE, "max_points must be >= 0")),
    ("oi_types", lambda gp, k: gp.optimal_interpolation(k.g, k.v, k.g, k.pv, k.pv, k.pv, k.st, 5), (TE, OI_TYPES)),
    ("oi_coordinates", lambda gp, k: gp.optimal_interpolation(k.g, k.v, k.pc, k.pv, k.pv, k.pv, k.st, 5), (VE, OI_COORDS)),
    ("oi_rank", lambda gp, k: gp.optimal_interpolation(k.g, Z(12), k.p, k.pv, k.pv, k.pv, k.st, 5), (RE, "background must have 2 dimensions, got 1")),
    ("oi_rank_points", lambda gp, k: gp.optimal_interpolation(k.p, k.v, k.p, k.pv, k.pv, k.pv, k.st, 5), (RE, "background must have 1 dimensions, got 2")),
    ("oi_size", lambda gp, k: gp.optimal_interpolation(k.g, k.vt, k.p, k.pv, k.pv, k.pv, k.st, 5),
     (VE, "input field (4, 3) is not the same size as the grid (3, 4)")),
    ("oi_obs_rank", lambda gp, k: gp.optimal_interpolation(k.g, k.v, k.p, k.pe, k.pv, k.pv, k.st, 5), (RE, "obs must have 1 dimensions, got 2")),
    ("oi_obs", lambda gp, k: gp.optimal_interpolation(k.g, k.v, k.p, Z(4), k.pv, k.pv, k.st, 5), (VE, "Observations (4) and points (5) size mismatch")),
    ("oi_ratios", lambda gp, k: gp.optimal_interpolation(k.g, k.v, k.p, k.pv, Z(4), k.pv, k.st, 5), (VE, "Ratios (4) and points (5) size mismatch")),
    ("oi_background", lambda gp, k: gp.optimal_interpolation(k.g, k.v, k.p, k.pv, k.pv, Z(6), k.st, 5), (VE, "Background (6) and points (5) size mismatch")),
    ("oi_structure", lambda gp, k: gp.optimal_interpolation(k.g, k.v, k.p, k.pv, k.pv, k.pv, None, 5),
     (RE, "structure must be one of the gridpp_amd structure functions")),
    ("oi_max_points_first", lambda gp, k: gp.optimal_interpolation(k.g, k.vt, k.g, k.pv, k.pv, k.pv, k.st, -1), (VE, "max_points must be >= 0")),
    ("oi_size_first", lambda gp, k: gp.optimal_interpolation(k.g, k.vt, k.p, Z(4), Z(4), k.pv, None, 5),
     (VE, "input field (4, 3) is not the same size as the grid (3, 4)")),
    ("oi_obs_first", lambda gp, k: gp.optimal_interpolation(k.g, k.v, k.p, Z(4), Z(3), Z(2), k.st, 5), (VE, "Observations (4) and points (5) size mismatch")),
    ("oi_valid", lambda gp, k: gp.optimal_interpolation(k.g, k.v, k.p, k.pv, np.ones(5), k.pv, k.st, 5), NO_DEVICE),
    ("oi_valid_points", lambda gp, k: gp.optimal_interpolation(k.p, k.pv, k.p, k.pv, np.ones(5), k.pv, k.st, 5), NO_DEVICE),
    ("oi_full_max_points", lambda gp, k: gp.optimal_interpolation_full(k.g, k.v, k.v, k.p, k.pv, k.pv, k.pv, k.pv, k.st, -1), (VE, "max_points must be >= 0")),
    ("oi_full_types", lambda gp, k: gp.optimal_interpolation_full(None, k.v, k.v, k.p, k.pv, k.pv, k.pv, k.pv, k.st, 5), (TE, OI_TYPES)),
    ("oi_full_bvariance_rank", lambda gp, k: gp.optimal_interpolation_full(k.g, k.v, Z(12), k.p, k.pv, k.pv, k.pv, k.pv, k.st, 5),
     (RE, "bvariance must have 2 dimensions, got 1")),
    ("oi_full_bvariance", lambda gp, k: gp.optimal_interpolation_full(k.g, k.v, k.vt, k.p, k.pv, k.pv, k.pv, k.pv, k.st, 5),
     (VE, "Input bvariance is not the same size as the grid")),
    ("oi_full_variance_rank", lambda gp, k: gp.optimal_interpolation_full(k.g, k.v, k.v, k.p, k.pv, k.pe, k.pv, k.pv, k.st, 5),
     (RE, "variance must have 1 dimensions, got 2")),
    ("oi_full_bvariance_at_points", lambda gp, k: gp.optimal_interpolation_full(k.g, k.v, k.v, k.p, k.pv, k.pv, k.pv, Z(4), k.st, 5),
     (VE, "Background variance and points size mismatch")),
    ("oi_full_bvariance_first", lambda gp, k: gp.optimal_interpolation_full(k.g, k.v, k.vt, k.p, Z(4), k.pv, k.pv, Z(4), k.st, 5),
     (VE, "Input bvariance is not the same size as the grid")),
    ("oi_full_background_first", lambda gp, k: gp.optimal_interpolation_full(k.g, k.v, k.v, k.p, k.pv, k.pv, Z(4), Z(4), k.st, 5),
     (VE, "Background (4) and points (5) size mismatch")),
    ("oi_full_valid", lambda gp, k: gp.optimal_interpolation_full(k.g, k.v, np.ones((3, 4)), k.p, k.pv, np.ones(5), k.pv, np.ones(5), k.st, 5), NO_DEVICE),
    # optimal_interpolation_ensi
    ("ensi_max_points", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.c, k.p, k.pv, k.pv, k.pe, k.st, -1), (VE, "max_points must be >= 0")),
    ("ensi_types", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.c, k.g, k.pv, k.pv, k.pe, k.st, 5), (TE, OI_TYPES)),
    ("ensi_rank", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.v, k.p, k.pv, k.pv, k.pe, k.st, 5), (RE, "background must have 3 dimensions, got 2")),
    ("ensi_rank_points", lambda gp, k: gp.optimal_interpolation_ensi(k.p, k.c, k.p, k.pv, k.pv, k.pe, k.st, 5), (RE, "background must have 2 dimensions, got 3")),
    ("ensi_coordinates", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.c, k.pc, k.pv, k.pv, k.pe, k.st, 5), (VE, OI_COORDS)),
    ("ensi_empty_grid", lambda gp, k: gp.optimal_interpolation_ensi(k.g0, Z((0, 0, 2)), k.p, k.pv, k.pv, k.pe, k.st, 5), (VE, "Grid size cannot be zero")),
    ("ensi_size", lambda gp, k: gp.optimal_interpolation_ensi(k.g, Z((4, 3, 2)), k.p, k.pv, k.pv, k.pe, k.st, 5), (VE, "Input field is not the same size as the grid")),
    ("ensi_obs_rank", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.c, k.p, k.pe, k.pv, k.pe, k.st, 5), (RE, "obs must have 1 dimensions, got 2")),
    ("ensi_sigmas_rank", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.c, k.p, k.pv, k.pe, k.pe, k.st, 5), (RE, "sigmas must have 1 dimensions, got 2")),
    ("ensi_background_rank", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.c, k.p, k.pv, k.pv, k.pv, k.st, 5),
     (RE, "background_at_points must have 2 dimensions, got 1")),
    ("ensi_obs", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.c, k.p, Z(4), k.pv, k.pe, k.st, 5), (VE, "Observations and points size mismatch")),
    ("ensi_sigmas", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.c, k.p, k.pv, Z(4), k.pe, k.st, 5), (VE, "Sigmas and points size mismatch")),
    ("ensi_background", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.c, k.p, k.pv, k.pv, Z((4, 2)), k.st, 5), (VE, "Background and points size mismatch")),
    ("ensi_members", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.c, k.p, k.pv, k.pv, Z((5, 3)), k.st, 5),
     (VE, "Ensemble members in gridded background is not the same as in the point background")),
    ("ensi_max_points_first", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.v, k.g, k.pv, k.pv, k.pe, k.st, -1), (VE, "max_points must be >= 0")),
    ("ensi_coordinates_first", lambda gp, k: gp.optimal_interpolation_ensi(k.g, Z((4, 3, 2)), k.pc, Z(4), k.pv, k.pe, k.st, 5), (VE, OI_COORDS)),
    ("ensi_obs_first", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.c, k.p, Z(4), Z(4), Z((4, 3)), k.st, 5), (VE, "Observations and points size mismatch")),
    ("ensi_no_points", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.c, k.p0, [], [], Z((0, 2)), k.st, 5), (3, 4, 2)),
    ("ensi_no_points_unchecked", lambda gp, k: gp.optimal_interpolation_ensi(k.g, Z((4, 3, 2)), k.p0, k.pv, k.pv, k.pv, None, 5), (4, 3, 2)),
    ("ensi_valid", lambda gp, k: gp.optimal_interpolation_ensi(k.g, k.c, k.p, k.pv, np.ones(5), k.pe, k.st, 5), NO_DEVICE),
    ("ensi_valid_points", lambda gp, k: gp.optimal_interpolation_ensi(k.p, k.pe, k.p, k.pv, np.ones(5), k.pe, k.st, 5), NO_DEVICE),
]


@pytest.fixture(scope="module")
def case(gridpp):
    return Case(gridpp)


@pytest.mark.parametrize("name,call,expected", ROWS, ids=[r[0] for r in ROWS])
def test_row(gridpp, case, name, call, expected):
    if expected is NO_DEVICE:
        if gridpp.device_count() > 0:
            call(gridpp, case)      # every check passed and the library did the work
        else:
            with pytest.raises(RuntimeError, match=NO_DEVICE_TEXT):
                call(gridpp, case)
    elif isinstance(expected[0], type):
        with pytest.raises(expected[0]) as e:
            call(gridpp, case)
        assert type(e.value) is expected[0] and str(e.value) == expected[1]
    else:
        out = call(gridpp, case)
        assert isinstance(out, np.ndarray) and out.shape == expected and out.dtype == np.float32


def test_every_function_has_its_rows():
    covered = {n for r in ROWS for n in r[1].__code__.co_names}
    for f in ("nearest", "bilinear", "gridding", "gridding_nearest", "fill", "fill_missing", "doping_square", "doping_circle",
              "neighbourhood_search", "calc_gradient", "neighbourhood", "neighbourhood_brute_force", "neighbourhood_quantile",
              "neighbourhood_quantile_fast", "calc_statistic", "calc_quantile", "optimal_interpolation", "optimal_interpolation_full",
              "optimal_interpolation_ensi"):
        assert f in covered
