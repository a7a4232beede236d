"""Case builders of the gridops edge suites (tests/test_gpu_gridops_edges.py on the GPU, tests/test_gridops_cases_oracle.py on the
CPU): deterministic inputs for fill_missing, calc_gradient, neighbourhood_search, fill and doping at the shapes and values where the
kernels of gridpp_amd/csrc/gridops.hip take another path or apply a tie rule, their references from the C oracle (a sequential loop
restatement that knows nothing of segments, bins or winners), and the constructions that show a case can tell a wrong kernel from a
right one.  Nothing here imports the GPU package."""
import functools
import math

import numpy as np

F = np.float32
NAN, INF = F(np.nan), F(np.inf)
MINMAX, LINREG = 0, 10          # gridpp.MinMax, gridpp.LinearRegression (checked by the GPU suite)


def _o():
    from oracle import oracle as O
    return O


# ---- fill_missing ---------------------------------------------------------------------------------------------------------------
FM_MAXX = 8192                  # gridops.hip: longest line of k_fill_missing_rows; anything longer goes to k_fill_missing_lines
FM_SHAPES = ((3, 255), (3, 256), (3, 257), (4, 511), (4, 512), (4, 513), (5, 1000), (1000, 5), (300, 300), (2, 8191), (2, 8192),
             (2, 8193), (8193, 2), (3, 8200))
FM_PATTERNS = ("random30", "long_run", "leading_run", "trailing_run", "missing_line", "single_valid", "segment_starts", "segment_ends",
               "inf_mixed")
FM_CASES = tuple("%s-%dx%d" % (p, y, x) for p in FM_PATTERNS for (y, x) in FM_SHAPES)
# one shape per pattern for the device-tensor input: every segment length and both kernels appear once
FM_DEVICE_CASES = ("random30-300x300", "long_run-2x8192", "leading_run-4x513", "trailing_run-1000x5", "missing_line-3x8200",
                   "single_valid-2x8191", "segment_starts-5x1000", "segment_ends-4x512", "inf_mixed-3x257")


def segment_length(n):
    """elements per thread of k_fill_missing_rows for a line of n elements"""
    return (n + 255) // 256


def _fm_lines(pattern, nlines, n, rng):
    """(nlines, n): the pattern along the second axis"""
    v = rng.normal(0, 3, (nlines, n)).astype(F)
    seg = segment_length(n)
    if pattern == "random30":
        v[rng.random(v.shape) < 0.3] = NAN
    elif pattern == "long_run":
        v[:, 10:n - 9] = NAN                       # 10 .. n - 10: longer than any segment
    elif pattern == "leading_run":
        for r in range(nlines):
            v[r, :n // 3 + 7 * (r % 4) + 1] = NAN        # the first element is missing: `last` = 0 points at it
            v[r, n // 2 + r % 4] = NAN                 # (an ordinary gap behind it still interpolates)
    elif pattern == "trailing_run":
        for r in range(nlines):
            v[r, n - n // 3 - 7 * (r % 4) - 1:] = NAN    # no `next`
            v[r, n // 4 + r % 4] = NAN
    elif pattern == "missing_line":
        v[rng.random(v.shape) < 0.3] = NAN
        v[0, :] = NAN
    elif pattern == "single_valid":
        keep = v.copy()
        v[:] = NAN
        for r in range(nlines):
            i = (0, n // 2, n - 1)[r % 3]
            v[r, i] = keep[r, i]
    elif pattern in ("segment_starts", "segment_ends"):
        # line r keeps one value every (1 + r % 3) segments: threads in between own a segment with no valid value
        keep = v.copy()
        v[:] = NAN
        for r in range(nlines):
            stride = seg * (1 + r % 3)
            first = 0 if pattern == "segment_starts" else seg - 1
            v[r, first::stride] = keep[r, first::stride]
    elif pattern == "inf_mixed":
        u = rng.random(v.shape)
        v[u < 0.1] = NAN
        v[(u >= 0.1) & (u < 0.2)] = INF
        v[(u >= 0.2) & (u < 0.3)] = -INF
        v[0, 0] = INF                              # `last` = 0 points at an inf
        v[-1, -1] = -INF
    else:
        raise KeyError(pattern)
    return v


@functools.lru_cache(maxsize=None)
def fill_missing_case(name):
    """the named field; the pattern runs along the longer axis (along the rows of a square field)"""
    pattern, shape = name.split("-")
    Y, X = (int(s) for s in shape.split("x"))
    rng = np.random.default_rng(FM_CASES.index(name) + 1)
    v = _fm_lines(pattern, Y, X, rng) if X >= Y else np.ascontiguousarray(_fm_lines(pattern, X, Y, rng).T)
    assert v.shape == (Y, X)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def fill_missing_reference(name):
    out = _o().fill_missing(fill_missing_case(name))
    out.setflags(write=False)
    return out


def fill_missing_known_answers():
    """[(name, input, expected)]: answers derived by hand.  With one row (one column) the other pass leaves every missing cell NaN, so
    the merge returns the row (column) result.  The ramp: 0 + (599 - 0) * k / 599 with 599 * k < 2^24 and an exact quotient."""
    ramp = np.full((1, 600), NAN, F)
    ramp[0, 0], ramp[0, 599] = 0, 599
    ramp_out = np.arange(600, dtype=F).reshape(1, 600)
    # leading run: 0 .. 299 missing -> NaN (interpolated from the missing element 0); 300 .. 599 = 2 k, with 450 .. 452 missing -> 2 k
    lead = (2 * np.arange(600)).astype(F).reshape(1, 600)
    lead[0, :300] = NAN
    lead_out = lead.copy()
    lead[0, 450:453] = NAN               # 898 + (906 - 898) * (k - 449) / 4
    # trailing run: 300 .. 599 missing -> NaN; 100 .. 103 missing between 99 and 104 -> k
    trail = np.arange(600, dtype=F).reshape(1, 600)
    trail[0, 300:] = NAN
    trail_out = trail.copy()
    trail[0, 100:104] = NAN              # 99 + (104 - 99) * (k - 99) / 5
    rows = [("ramp_row", ramp, ramp_out), ("leading_run_row", lead, lead_out), ("trailing_run_row", trail, trail_out)]
    cols = [(n.replace("row", "column"), np.ascontiguousarray(a.T), np.ascontiguousarray(b.T)) for n, a, b in rows]
    return rows + cols[:1]


# ---- calc_gradient --------------------------------------------------------------------------------------------------------------
GRAD_SHAPE = (37, 41)
# (halfwidth, num_min, min_range, default_gradient)
MINMAX_ROWS = {
    "hw1": (1, 0, math.nan, -0.0065),
    "hw2": (2, 3, 1.0, 0.0),
    "hw50": (50, 2, 0.0, 1.0),              # at least both dimensions: every cell sees the whole field
    "count4": (1, 4, 0.0, 0.25),            # corner windows hold 4 cells: count == num_min, or num_min - 1 next to a missing one
    "count6": (1, 6, 0.0, 0.25),            # edge windows hold 6
    "range3": (1, 0, 3.0, 9.0),             # |cmax - cmin| == min_range exactly on many cells: they take the default
    "range5": (2, 0, 5.0, 9.0),
}
TIE_SEED = 41


@functools.lru_cache(maxsize=None)
def minmax_tie_case():
    """base: integers 0 .. 5 with about 5 % NaN and a few inf (every window holds its maximum and its minimum many times);
    values: continuous with a few NaN"""
    rng = np.random.default_rng(TIE_SEED)
    Y, X = GRAD_SHAPE
    base = rng.integers(0, 6, (Y, X)).astype(F)
    base[rng.random((Y, X)) < 0.05] = NAN
    for (y, x), v in (((3, 4), INF), ((20, 30), -INF), ((36, 0), INF), ((11, 11), INF)):
        base[y, x] = v
    values = rng.normal(280, 3, (Y, X)).astype(F)
    values[rng.random((Y, X)) < 0.02] = NAN
    values[8, 8] = INF
    base.setflags(write=False)
    values.setflags(write=False)
    return base, values


@functools.lru_cache(maxsize=None)
def minmax_reference(row):
    base, values = minmax_tie_case()
    out = _o().calc_gradient(base, values, MINMAX, *MINMAX_ROWS[row])
    out.setflags(write=False)
    return out


def flip2(a):
    return np.ascontiguousarray(a[::-1, ::-1])


def minmax_last_tie_wins(row):
    """what a scan that keeps the LAST maximum / minimum (`>=`, or the window walked backwards) returns: the oracle on the fields
    flipped on both axes, flipped back"""
    base, values = minmax_tie_case()
    return flip2(_o().calc_gradient(flip2(base), flip2(values), MINMAX, *MINMAX_ROWS[row]))


def window_count(valid, hw):
    """number of valid cells in the (2 hw + 1)^2 window of every cell, clipped at the edges"""
    Y, X = valid.shape
    s = np.zeros((Y + 1, X + 1), np.int64)
    s[1:, 1:] = np.cumsum(np.cumsum(valid.astype(np.int64), 0), 1)
    y0, y1 = np.clip(np.arange(Y) - hw, 0, Y)[:, None], np.clip(np.arange(Y) + hw + 1, 0, Y)[:, None]
    x0, x1 = np.clip(np.arange(X) - hw, 0, X)[None, :], np.clip(np.arange(X) + hw + 1, 0, X)[None, :]
    return s[y1, x1] - s[y0, x1] - s[y1, x0] + s[y0, x0]


def finite(a):
    return np.isfinite(a)


BLOCK = (slice(5, 25), slice(5, 30))        # rows 5 .. 24, columns 5 .. 29 of constant base 3.0
BLOCK_INNER = (slice(7, 23), slice(7, 28))  # cells whose halfwidth-2 window lies inside the block
LINREG_DEFAULT = -777.0
LINREG_ROWS = {
    "hw1": (1, 0, math.nan, LINREG_DEFAULT),
    "block_hw2": (2, 0, math.nan, LINREG_DEFAULT),
    "block_hw2_range": (2, 2, 0.0, LINREG_DEFAULT),
    "hw60": (60, 2, 0.0, LINREG_DEFAULT),   # every cell has the same window: the whole field
    "count9": (1, 9, math.nan, LINREG_DEFAULT),   # a full interior window holds exactly 9; one missing cell makes it num_min - 1
    "count6": (1, 6, math.nan, LINREG_DEFAULT),   # edge windows
    "count4": (1, 4, 5.0, LINREG_DEFAULT),        # corner windows (the standard deviation of the complete one is 12.9)
}


@functools.lru_cache(maxsize=None)
def linreg_case():
    rng = np.random.default_rng(52)
    Y, X = GRAD_SHAPE
    base = rng.uniform(0, 1500, (Y, X)).astype(F)
    values = (280 - 0.0065 * base + rng.normal(0, 0.3, (Y, X))).astype(F)
    base[rng.random((Y, X)) < 0.04] = NAN
    values[rng.random((Y, X)) < 0.02] = NAN
    base[1, 2], base[30, 35] = INF, -INF
    base[BLOCK] = 3.0
    values[BLOCK] = (280 + rng.normal(0, 0.3, (Y, X))).astype(F)[BLOCK]
    base[0, 0:2], base[1, 0:2] = (10.0, 20.0), (30.0, 45.0)      # one corner window complete: count == 4
    values[0, 0:2], values[1, 0:2] = (279.0, 278.5), (281.0, 277.0)
    base[0, -2:], base[1, -2:] = (NAN, 20.0), (30.0, 45.0)       # and one with a missing cell: count == 3
    values[0, -2:], values[1, -2:] = (279.0, 278.5), (281.0, 277.0)
    base.setflags(write=False)
    values.setflags(write=False)
    return base, values


@functools.lru_cache(maxsize=None)
def linreg_reference(row):
    base, values = linreg_case()
    out = _o().calc_gradient(base, values, LINREG, *LINREG_ROWS[row])
    out.setflags(write=False)
    return out


# ---- neighbourhood_search -------------------------------------------------------------------------------------------------------
# (halfwidth, search_target_min, search_target_max, search_delta)
SEARCH_ROWS = {
    "nearest_ties": (1, 2.0, 3.0, 0.1),     # nothing in range: the nearest-target rule, with many equal distances
    "point_target": (2, 2.0, 2.0, 0.0),     # tmin == tmax, delta 0
    "hw0": (0, 0.5, 0.5, 0.1),              # the window is the cell itself
    "whole_field": (60, 2.0, 3.0, 0.2),
    "mixed": (2, 0.45, 0.55, 0.3),          # means of in-range cells next to nearest targets; `counter > 0` skips later cells
}
SEARCH_SEED = 61


@functools.lru_cache(maxsize=None)
def search_case():
    """(array, search, apply): search = k / 10, k = 0 .. 10, with a few inf and NaN; array continuous with a few NaN;
    apply = 0 (keep), 1 (search), 2 (neither)"""
    rng = np.random.default_rng(SEARCH_SEED)
    Y, X = GRAD_SHAPE
    search = (rng.integers(0, 11, (Y, X)).astype(F) / F(10)).astype(F)
    search[rng.random((Y, X)) < 0.03] = NAN
    search[2, 3], search[19, 19], search[36, 40] = INF, -INF, INF
    array = rng.normal(10, 4, (Y, X)).astype(F)
    array[rng.random((Y, X)) < 0.03] = NAN
    array[5, 5] = INF
    apply = rng.integers(0, 3, (Y, X)).astype(np.int32)
    for a in (array, search, apply):
        a.setflags(write=False)
    return array, search, apply


@functools.lru_cache(maxsize=None)
def search_reference(row, with_apply):
    array, search, apply = search_case()
    out = _o().neighbourhood_search(array, search, *SEARCH_ROWS[row], apply if with_apply else None)
    out.setflags(write=False)
    return out


def search_last_tie_wins(row):
    array, search, _ = search_case()
    return flip2(_o().neighbourhood_search(flip2(array), flip2(search), *SEARCH_ROWS[row]))


def differing_share(a, b):
    """share of cells where a and b differ (NaN equals NaN)"""
    return float(np.mean(~((a == b) | (np.isnan(a) & np.isnan(b)))))


# ---- fill, doping_circle, doping_square -----------------------------------------------------------------------------------------
CART_Y, CART_X, SPACING = 20, 25, 1000.0     # Cartesian grid: node (y, x) at 1000 (y - 10), 1000 (x - 12) metres, exact in float32
LAT0, LON0 = -10 * SPACING, -12 * SPACING    # (the interior node (10, 12) is the origin: there x +- radius is exact for a radius of 1000 + 1 ulp)
GEO_Y, GEO_X = 12, 15
CARTESIAN, GEODETIC = 1, 0
FILL_VALUE = -7.5
R_DIAGONAL = F(np.sqrt(F(2e6)))              # float32 distance between diagonal neighbours: sqrtf(1000^2 + 1000^2)


def node(y, x):
    return y * CART_X + x


def at(y, x):
    """(lat, lon) of the position (y, x) given in node units (fractions allowed)"""
    return LAT0 + np.asarray(y, np.float64) * SPACING, LON0 + np.asarray(x, np.float64) * SPACING


@functools.lru_cache(maxsize=None)
def grid_arrays(kind):
    """(lats, lons, elevs, ctype)"""
    if kind == "cart":
        lats, lons = np.meshgrid(LAT0 + np.arange(CART_Y) * SPACING, LON0 + np.arange(CART_X) * SPACING, indexing="ij")
        yy, xx = np.meshgrid(np.arange(CART_Y), np.arange(CART_X), indexing="ij")
        elev = (100 + 10 * (yy + xx)).astype(F)          # 100 .. 530, exact
        elev[10, 12] = elev[5, 5] = 300.0
        for y, x in ((4, 5), (15, 20), (15, 21), (0, 0)):
            elev[y, x] = NAN
        ct = CARTESIAN
    else:
        lats, lons = np.meshgrid(np.linspace(59, 59.5, GEO_Y), np.linspace(10, 11, GEO_X), indexing="ij")
        elev = np.random.default_rng(71).uniform(0, 600, (GEO_Y, GEO_X)).astype(F)
        elev[3, 3] = NAN
        ct = GEODETIC
    out = (lats.astype(F), lons.astype(F), elev)
    for a in out:
        a.setflags(write=False)
    return out + (ct,)


@functools.lru_cache(maxsize=None)
def background(kind):
    lats = grid_arrays(kind)[0]
    bg = np.random.default_rng(72).normal(100, 1, lats.shape).astype(F)     # never equal to an observation or the fill value
    bg.setflags(write=False)
    return bg


def _case(grid, lat, lon, radii=None, hw=None, elev=None, obs=None, med=math.nan, ops=("fill_in", "fill_out", "circle")):
    lat, lon = np.atleast_1d(np.asarray(lat, F)), np.atleast_1d(np.asarray(lon, F))
    n = lat.size
    c = dict(grid=grid, lat=lat, lon=lon, med=float(med), ops=tuple(ops),
             elev=np.full(n, NAN, F) if elev is None else np.asarray(elev, F).reshape(n),
             obs=np.arange(n, dtype=F) if obs is None else np.asarray(obs, F).reshape(n),
             radii=None if radii is None else np.broadcast_to(np.asarray(radii, F), (n,)).copy(),
             hw=None if hw is None else np.broadcast_to(np.asarray(hw, np.int32), (n,)).copy())
    return c


def _outside_points(far):
    """eight points beyond the four sides and the four corners of the Cartesian grid, `far` grid widths away (off the node
    lines, so that each has one nearest node)"""
    h, w = CART_Y - 1, CART_X - 1
    y = [-far * h, h + far * h, 0.37 * h, 0.61 * h, -far * h, -far * h, h + far * h, h + far * h]
    x = [0.43 * w, 0.57 * w, -far * w, w + far * w, -far * w, w + far * w, -far * w, w + far * w]
    lat, lon = at(y, x)
    return lat.astype(F), lon.astype(F)


@functools.lru_cache(maxsize=None)
def scatter_cases():
    """name -> case of fill (inside / outside), doping_circle and doping_square"""
    up = np.nextafter
    on = at(10, 12)                                      # the interior node (10, 12), at the origin
    far_lat, far_lon = _outside_points(10)
    near_lat, near_lon = _outside_points(0.15)
    geo_out = (np.array([59.25, 59.25, 40.0, 80.0, 20.0, 89.0], F), np.array([40.0, -20.0, 10.5, 10.5, -30.0, 170.0], F))
    rng = np.random.default_rng(73)
    K = {
        # exact radius: the axis neighbours sit ON the strict box at 1000; the diagonal ones at the float32 distance sqrtf(2e6)
        "radius_1000": _case("cart", *on, radii=1000.0),
        "radius_1000_up": _case("cart", *on, radii=up(F(1000), INF)),
        # away from the origin the box bounds x +- radius round back onto the neighbours (8000 + 1000.00006 = 9000 in float32): one node
        "radius_1000_up_rounds": _case("cart", *at(3, 20), radii=up(F(1000), INF)),
        "radius_1001": _case("cart", *at(3, 20), radii=1001.0),
        "radius_diag": _case("cart", *on, radii=R_DIAGONAL),
        "radius_diag_down": _case("cart", *on, radii=up(R_DIAGONAL, F(0))),
        # clamps of the bin index
        "far_small": _case("cart", far_lat, far_lon, radii=400.0),
        "far_reaching": _case("cart", far_lat, far_lon, radii=[193500.0, 192000.0, 242500.0, 241000.0, 310000.0, 309000.0, 308000.0, 307500.0]),
        "near_outside": _case("cart", near_lat, near_lon, radii=[3500.0, 4000.0, 4500.0, 5000.0, 6000.0, 6500.0, 7000.0, 7500.0]),
        "covers_all": _case("cart", *at(9.5, 12), radii=40000.0),
        "half_spacing": _case("cart", *at([10.5, 3], [12.5, 4.5]), radii=500.0),        # a cell centre, an edge midpoint (on the box)
        "half_spacing_on_node": _case("cart", *on, radii=500.0),
        "radius_0": _case("cart", *at([10, 10.5], [12, 12.5]), radii=0.0),
        "no_points": _case("cart", [], [], radii=[], hw=[], ops=("fill_in", "fill_out", "circle", "square")),
        "geo_far_small": _case("geo", *geo_out, radii=1000.0),
        "geo_covers_all": _case("geo", 59.25, 10.5, radii=3e7),
        "geo_far_covers_all": _case("geo", [-60.0], [-170.0], radii=3e7),
        "geo_half_spacing": _case("geo", 59.25, 10.5, radii=1200.0),
        "geo_mixed": _case("geo", 59 + 0.5 * (1.4 * rng.random(12) - 0.2), 10 + (1.4 * rng.random(12) - 0.2), radii=rng.uniform(0, 30000, 12).astype(F),
                           hw=rng.integers(0, 4, 12), elev=rng.uniform(0, 600, 12), med=150.0,
                           ops=("fill_in", "fill_out", "circle", "square")),
        "geo_no_points": _case("geo", [], [], radii=[], hw=[], ops=("fill_in", "fill_out", "circle", "square")),
    }
    # elevation rule with max_elev_diff = 50: points 0, 1 have no elevation (point 1 meets the NaN cell (4, 5)), points 2, 3 have one and
    # meet the NaN cells (15, 20), (15, 21), point 4 sits on the NaN cell (0, 0), point 5 differs from its own node by exactly 50
    # (written) and from the others by more
    e_lat, e_lon = at([4, 4, 15, 16, 0, 10], [4, 6, 19, 21, 0, 12])
    e_elev = np.array([np.nan, np.nan, 430.0, 100.0, 100.0, 250.0], F)
    e_obs = np.array([7, 8, 9, 10, 11, 12], F)
    K["elev_circle"] = _case("cart", e_lat, e_lon, radii=1001.0, elev=e_elev, obs=e_obs, med=50.0, ops=("circle",))
    K["elev_square"] = _case("cart", e_lat, e_lon, hw=1, elev=e_elev, obs=e_obs, med=50.0, ops=("square",))
    # max_elev_diff == 0: node (10, 12) and node (5, 5) have elevation 300; point 0 has exactly 300 (writes), point 1 one ulp more (does not)
    z_lat, z_lon = at([10, 5], [12, 5])
    z_elev = np.array([300.0, up(F(300), INF)], F)
    K["elev_zero_circle"] = _case("cart", z_lat, z_lon, radii=500.0, elev=z_elev, obs=[7, 8], med=0.0, ops=("circle",))
    K["elev_zero_square"] = _case("cart", z_lat, z_lon, hw=0, elev=z_elev, obs=[7, 8], med=0.0, ops=("square",))
    # doping_square
    K["square_hw0"] = _case("cart", *at([10.3, 2.4], [11.8, 7.3]), hw=0, ops=("square",))           # nearest: (10, 12), (2, 7)
    K["square_covers_all"] = _case("cart", *at(9.6, 12.2), hw=max(CART_Y, CART_X), ops=("square",))
    K["square_huge_hw"] = _case("cart", *at([0.3, 18.8], [0.2, 23.9]), hw=[3, 1 << 30], ops=("square",))   # hw + index stays below 2^31
    K["square_shared_cell"] = _case("cart", *at([10.3, 9.8, 2.4], [11.8, 12.1, 7.3]), hw=[2, 1, 0], ops=("square",))
    K["square_outside"] = _case("cart", near_lat, near_lon, hw=[2, 2, 2, 2, 3, 3, 3, 3], ops=("square",))
    K["square_far_outside"] = _case("cart", far_lat, far_lon, hw=2, ops=("square",))
    return K


def expected_hits():
    """hand-derived hit sets (flat node indices) of the single-point cases"""
    c = node(10, 12)
    plus = sorted([c, c - 1, c + 1, c - CART_X, c + CART_X])
    ring = sorted(plus + [c - CART_X - 1, c - CART_X + 1, c + CART_X - 1, c + CART_X + 1])
    everything = list(range(CART_Y * CART_X))
    far = node(3, 20)
    plus_far = sorted([far, far - 1, far + 1, far - CART_X, far + CART_X])
    return {"radius_1000": [c], "radius_1000_up": plus, "radius_1000_up_rounds": [far], "radius_1001": plus_far, "radius_diag": ring, "radius_diag_down": plus, "far_small": [],
            "covers_all": everything, "half_spacing": [], "half_spacing_on_node": [c], "radius_0": [], "no_points": [],
            "geo_far_small": [], "geo_covers_all": list(range(GEO_Y * GEO_X)), "geo_far_covers_all": list(range(GEO_Y * GEO_X)),
            "geo_half_spacing": [], "geo_no_points": []}


def oracle_sets(c):
    """(grid Pts, point Pts) of the oracle for a scatter case"""
    O = _o()
    lats, lons, elev, ct = grid_arrays(c["grid"])
    return O.Pts(lats.ravel(), lons.ravel(), elev.ravel(), None, ct), O.Pts(c["lat"], c["lon"], c["elev"], None, ct)


@functools.lru_cache(maxsize=None)
def scatter_reference(name, op):
    c = scatter_cases()[name]
    O = _o()
    g, p = oracle_sets(c)
    bg = background(c["grid"])
    if op == "fill_in":
        out = O.fill(g, bg, p, c["radii"], FILL_VALUE, False)
    elif op == "fill_out":
        out = O.fill(g, bg, p, c["radii"], FILL_VALUE, True)
    elif op == "circle":
        out = O.doping_circle(g, bg, p, c["obs"], c["radii"], c["med"])
    else:
        out = O.doping_square(g, bg.shape, bg, p, c["obs"], c["hw"], c["med"])
    out.setflags(write=False)
    return out


def hit_set(name, out, op):
    """flat indices of the cells an operation reached, from its output (the background never equals the fill value or an observation)"""
    bg = background(scatter_cases()[name]["grid"])
    changed = np.asarray(out) != bg
    return np.flatnonzero(~changed if op == "fill_out" else changed).tolist()
