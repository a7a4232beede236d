"""Fixtures of the local_distribution_correction edge suites (tests/test_gpu_ldc_edges.py on the GPU, tests/test_ldc_edge_cases_oracle.py
on the CPU) and the conditions that keep them from passing vacuously.  Every fixture is restated by tests/ldc_ref.py over the C oracle;
the restatement is computed once per (fixture, quantile pair) and handed out read-only.  Nothing here imports the GPU package.

What gridpp_amd/csrc/ldc.hip can get wrong and which fixture looks there:

    ladder      one column of cells per pair count, from 1 to 2 049: the lane edges of ldc_finish's strided loops (63 / 64 / 65, ...), the
                powers of two where the bitonic padding is empty, LDC_LDS_MAX (511 / 512 / 513: the hand-over from k_ldc_cell_lds to
                rocPRIM's segmented sort and k_ldc_cell_hbm, both launched in one call), 300 cells (a second workgroup of k_ldc_count /
                k_ldc_fill), and under GPP_CSR_CAP = 300 cells that are larger than a whole filling pass (chunks_of's q1 <= q0 branch)
    zero_rho    cells whose trimmed ref curve, fcst curve or both have a rho total of 0: their quantiles are NaN, the second interpolation
                must leave the bisection, and the project's rule for an undefined index (NaN, gridpp_amd/csrc/curve.h) decides the result
    thresholds  backgrounds one float around the double literals 0.01 and 0.1, -0, +inf, NaN, exactly on the branch-3 and 2a boundaries,
                counts of min_points and min_points - 1, and -0 / +inf / negative / NaN values at known (time, station) places of T = 4
    membership  stations at exactly the localization distance (kept on a diagonal, dropped by the open box on an axis) and one float beyond"""
import functools

import numpy as np

from tests import ldc_ref as R

F = np.float32
CARTESIAN = 1


def _o():
    from oracle import oracle as O
    return O


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


class Fixture:
    """A Cartesian grid (2-D lats = y, lons = x), stations (py, px), values (S) or (T, S), a background of the grid's shape, a scalar
    structure given as (kind, h, v, w, hmax) with an optional cross-validation distance, and the default quantiles and min_points."""

    def __init__(self, name, lats, lons, py, px, pobs, pbg, bg, structure=("Barnes", 2500.0, 0.0, 0.0, float("nan")), cv=None,
                 minq=0.2, maxq=0.8, min_points=0, gelev=None, pelev=None):
        self.name = name
        self.lats, self.lons = np.asarray(lats, np.float64), np.asarray(lons, np.float64)
        self.py, self.px = np.asarray(py, np.float64), np.asarray(px, np.float64)
        self.pobs, self.pbg, self.bg = np.array(pobs, F), np.array(pbg, F), np.array(bg, F)
        self.gelev = None if gelev is None else np.asarray(gelev, np.float64)
        self.pelev = None if pelev is None else np.asarray(pelev, np.float64)
        self.structure, self.cv = structure, cv
        self.minq, self.maxq, self.min_points = minq, maxq, min_points
        assert self.bg.shape == self.lats.shape == self.lons.shape and self.pobs.shape == self.pbg.shape
        assert self.pobs.shape[-1] == self.px.size == self.py.size
        _ro(self.pobs, self.pbg, self.bg)

    # ---- the restatement's side ----
    @functools.cached_property
    def oracle_structure(self):
        kind, h, v, w, hmax = self.structure
        st = _o().Struct(kind, h, v, w, hmax)
        return st if self.cv is None else st.cross_validation(self.cv)

    @functools.cached_property
    def oracle_points(self):
        O = _o()
        return O.Pts(self.lats, self.lons, self.gelev, ctype=CARTESIAN), O.Pts(self.py, self.px, self.pelev, ctype=CARTESIAN)

    @functools.cached_property
    def cands(self):
        g, p = self.oracle_points
        return R.candidates(_o(), g, p, self.oracle_structure)

    @functools.lru_cache(maxsize=None)
    def restate(self, minq=None, maxq=None):
        """-> (out, tags, counts, sums) of tests/ldc_ref.ldc, read-only"""
        sums = {}
        out, tags, counts = R.ldc(_o(), self.cands, self.bg, self.pobs, self.pbg, self.minq if minq is None else minq,
                                  self.maxq if maxq is None else maxq, self.min_points, sums=sums)
        _ro(out, tags, counts, *sums.values())
        return out, tags, counts, sums

    # ---- the device's side ----
    def device(self, gridpp):
        """-> (Grid, Points, structure) of the GPU package"""
        grid = gridpp.Grid(self.lats, self.lons, ((),) if self.gelev is None else self.gelev, ((),), gridpp.Cartesian)
        points = gridpp.Points(self.py, self.px, () if self.pelev is None else self.pelev, (), gridpp.Cartesian)
        kind, h, v, w, hmax = self.structure
        args = (h, v, w) if hmax != hmax else (h, v, w, hmax)
        st = getattr(gridpp, kind + "Structure")(*args)
        return grid, points, st if self.cv is None else gridpp.CrossValidation(st, self.cv)


# ---- 1. the count ladder ------------------------------------------------------------------------------------------------------------
LDS_MAX = 512                                   # LDC_LDS_MAX of gridpp_amd/csrc/ldc.hip
LADDER_COUNTS = (1, 2, 3, 4, 5, 9, 10, 11, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 514, 1023, 1024, 1025,
                 2047, 2048, 2049)
LADDER_ROWS = (0.005, 0.05, 0.3, 0.7, 1.5, 3, 6, 12, 25, 60)          # the background of a grid row
LADDER_SPACING, LADDER_CLUSTER = 40000.0, 3000.0                      # Barnes h = 2 500 reaches about 9.1 km: clusters never mix
LADDER_SEED = 1
LADDER_CAPS = (1000, 300)                       # GPP_CSR_CAP values: the 1 023+ cells exceed both, the 513+ cells the second
# the branches each quantile pair reaches on the ladder (measured on the CPU restatement, asserted by tests/test_ldc_edge_cases_oracle.py)
LADDER_QUANTILES = {
    (0.0, 1.0): {False: {R.B1, R.B3, R.B4}, True: {R.B1, R.B3, R.B4}},
    (0.1, 0.9): {False: {R.B1, R.B2B, R.B2C, R.B3, R.B4}, True: {R.B1, R.B2B, R.B2C, R.B3, R.B4}},
    (0.5, 0.5): {False: {R.B1, R.B2B, R.B2C}, True: {R.B1, R.B2B, R.B2C}},
    (0.3, 0.31): {False: {R.B1, R.B2B, R.B2C, R.B3, R.B4}, True: {R.B1, R.B2A, R.B2B, R.B2C, R.B3, R.B4}},
}


@functools.lru_cache(maxsize=None)
def _ladder_data():
    """stations, values and the column of every station -- the same draw for every view of the ladder"""
    rng = np.random.default_rng(LADDER_SEED)
    px, py, col = [], [], []
    for k, n in enumerate(LADDER_COUNTS):
        ang, rad = rng.uniform(0, 2 * np.pi, n), LADDER_CLUSTER * np.sqrt(rng.uniform(0, 1, n))
        px.append(k * LADDER_SPACING + rad * np.cos(ang))
        py.append(rad * np.sin(ang))
        col.append(np.full(n, k))
    S = sum(LADDER_COUNTS)
    pobs, pbg = rng.gamma(0.6, 3, S).astype(F), rng.gamma(0.6, 3, S).astype(F)
    return _ro(np.concatenate(px), np.concatenate(py), np.concatenate(col), pobs, pbg)


@functools.lru_cache(maxsize=None)
def ladder(rounded=False, columns=None, rows=None, permuted=False):
    """Column k holds LADDER_COUNTS[k] stations (T = 1: as many pairs), ten grid rows 1 m apart share a column's neighbours.
    rounded: the values to 0.5 mm (many tied zeros).  columns / rows: a sub-grid with the stations of its columns only, at the
    coordinates they have in the full ladder.  permuted: the stations (and their values) in another order."""
    px, py, col, pobs, pbg = _ladder_data()
    columns = tuple(range(len(LADDER_COUNTS))) if columns is None else tuple(columns)
    rows = tuple(range(len(LADDER_ROWS))) if rows is None else tuple(rows)
    if rounded:
        pobs, pbg = np.round(pobs * 2) / 2, np.round(pbg * 2) / 2
    keep = np.nonzero(np.isin(col, columns))[0]
    if permuted:
        keep = keep[np.random.default_rng(11).permutation(keep.size)]
    lons, lats = np.meshgrid(np.array(columns) * LADDER_SPACING, np.array(rows, np.float64))
    bg = np.repeat(np.array(LADDER_ROWS, F)[list(rows), None], len(columns), axis=1)
    fx = Fixture("ladder", lats, lons, py[keep], px[keep], pobs[keep], pbg[keep], bg, min_points=0)
    fx.columns, fx.rows = columns, rows
    fx.counts = np.array([LADDER_COUNTS[k] for k in columns])
    return fx


def ladder_columns(most):
    return tuple(k for k, n in enumerate(LADDER_COUNTS) if n <= most)


def sub_grid(full, fx):
    """the cells of a sub-ladder fx, taken from a (10, 30) result of the full ladder"""
    return np.asarray(full)[np.ix_(fx.rows, fx.columns)]


# ---- 2. zero rho ----------------------------------------------------------------------------------------------------------------------
ZERO_RHO = ("ref", "fcst", "both", "vertical")
ZERO_CV = 1000.0
_INSIDE = (2, 3, 4, 5, 6, 7)                    # the stations within the cross-validation distance: rho = 0
_MIDDLE = (3, 4, 5, 6, 7, 8)                    # the six middle values of ten, on the stations above
_SPREAD = (4, 5, 9, 10, 1, 2, 6, 7, 3, 8)       # the trimmed range [3, 8] holds 4 ... 7 of the four outer stations: rho > 0


@functools.lru_cache(maxsize=None)
def zero_rho(case):
    """A 2 x 2 grid 40 km wide; cell (0, 0) at the origin is the case, background 5.5, ten stations, T = 1, quantiles 0.2 / 0.8: ten
    pairs, trimmed to the sorted entries [2, 8).
      ref       CrossValidation(Barnes 2 500, 1 000).  Stations 2 ... 7 lie within 1 000 m (rho = 0) and hold pobs 3 ... 8: the trimmed
                ref curve has a rho total of 0, its quantiles are (0, NaN x 6).  The four stations 2 000 m away (rho = exp(-0.32)) hold
                pbackground 4 ... 7: the fcst curve (0, 3, ..., 8) has the quantiles (0, 0.2, 0.35, 0.5, 0.65, 0.8, 0.8), so 5.5 maps to
                q = 0.575, and the scan for q from the back of (0, NaN ...) meets no valid entry > q before 0 < q: undefined, NaN.
      fcst      the same with pobs and pbackground exchanged: q itself is NaN.
      both      every station within 1 000 m: both totals and sum_rho are 0, w0 = 0, and 0 * NaN is NaN.
      vertical  no CrossValidation: BarnesStructure(2 500, 10) with the stations 2 000 m above the cells -- the vertical factor
                exp(-20 000) underflows to exactly 0."""
    assert case in ZERO_RHO
    lons, lats = np.meshgrid([0.0, 40000.0], [0.0, 40000.0])
    bg = np.array([[5.5, 5.5], [0.05, 5.5]], F)
    near = [(100.0 * (k + 1), 0.0) for k in range(10)]
    xy = list(near)
    if case in ("ref", "fcst"):
        for k, at in zip((0, 1, 8, 9), ((2000.0, 0.0), (0.0, 2000.0), (-2000.0, 0.0), (0.0, -2000.0))):
            xy[k] = at
    px, py = np.array([a for a, _ in xy]), np.array([b for _, b in xy])
    middle = np.arange(1.0, 11.0)               # station k holds k + 1: stations 2 ... 7 hold 3 ... 8
    assert tuple(middle[list(_INSIDE)]) == _MIDDLE
    spread = np.array(_SPREAD, np.float64)
    pobs, pbg = (spread, middle) if case == "fcst" else (middle, spread)
    if case == "vertical":
        return Fixture("zero-rho-" + case, lats, lons, py, px, pobs, pbg, bg, structure=("Barnes", 2500.0, 10.0, 0.0, float("nan")),
                       gelev=np.zeros((2, 2)), pelev=np.full(10, 2000.0))
    return Fixture("zero-rho-" + case, lats, lons, py, px, pobs, pbg, bg, cv=ZERO_CV)


# ---- 3. thresholds ------------------------------------------------------------------------------------------------------------------
F001, F01 = F(0.01), F(0.1)
THRESHOLD_T, THRESHOLD_MIN_POINTS = 4, 9
THRESHOLD_COLUMNS = ("dry", "half", "wet", "few")


@functools.lru_cache(maxsize=None)
def thresholds():
    """Four columns of cells 40 km apart, each with its own stations within 100 m; nine rows 1 m apart; T = 4; quantiles 0 / 1 (the
    curves end at the largest kept value); min_points = 9.
      dry   3 stations, pobs = 0 (one of them -0), pbackground in [0, 0.02] with the largest exactly float32(0.02): 12 pairs,
            ref_last = 0, 3 fcst_last = 0.06.  Backgrounds: float32(0.01) (< the double 0.01: branch 1), the next float up (2a),
            float32(0.1) (> the double 0.1: 2c), the next float down (2b), -0 (branch 1, result +0), +inf and NaN (kept as they are),
            0.05 (2a), 0.07 (2b)
      half  3 stations, pobs = 0, pbackground <= 0.5 with the largest exactly 0.5: 3 fcst_last = 1.5 exactly.  Backgrounds: 1.5 (not
            below 3 fcst_last: 2c), the next float down (2a), the next float up (2c), then ordinary values
      wet   3 stations, gamma values; of the 12 (time, station) entries three are dropped -- pbackground[2, s1] = +inf,
            pobs[3, s2] = -1, pbackground[0, s2] = NaN -- and two are kept as +0: pobs[1, s0] = -0, pbackground[3, s0] = -0.  9 pairs =
            min_points.  Backgrounds: fcst_last (branch 3), the next float down (4), the next float up (3), then ordinary values
      few   2 stations, 8 pairs = min_points - 1: every cell keeps its background"""
    rng = np.random.default_rng(23)
    T = THRESHOLD_T
    sizes = dict(dry=3, half=3, wet=3, few=2)
    first, px, py = {}, [], []
    for k, name in enumerate(THRESHOLD_COLUMNS):
        first[name] = len(px)
        for s in range(sizes[name]):
            px.append(k * 40000.0 + 30.0 * s - 20.0)
            py.append(10.0 * s)
    S = len(px)
    pobs, pbg = rng.gamma(0.6, 3, (T, S)).astype(F), rng.gamma(0.6, 3, (T, S)).astype(F)
    d, h, w = first["dry"], first["half"], first["wet"]
    pobs[:, d:d + 3] = 0
    pobs[2, d + 1] = -0.0
    pbg[:, d:d + 3] = rng.uniform(0, 0.019, (T, 3))
    pbg[1, d + 2] = F(0.02)
    pobs[:, h:h + 3] = 0
    pbg[:, h:h + 3] = rng.uniform(0, 0.49, (T, 3))
    pbg[3, h] = 0.5
    pbg[2, w + 1], pobs[3, w + 2], pbg[0, w + 2] = np.inf, -1.0, np.nan
    pobs[1, w], pbg[3, w] = -0.0, -0.0
    kept = np.isfinite(pobs[:, w:w + 3]) & np.isfinite(pbg[:, w:w + 3]) & (pobs[:, w:w + 3] >= 0) & (pbg[:, w:w + 3] >= 0)
    fcst_last = pbg[:, w:w + 3][kept].max()
    up, down = (lambda v: np.nextafter(F(v), F(np.inf))), (lambda v: np.nextafter(F(v), F(-np.inf)))
    rows = 9
    bg = np.empty((rows, 4), F)
    bg[:, 0] = [F001, up(F001), F01, down(F01), -0.0, np.inf, np.nan, 0.05, 0.07]
    bg[:, 1] = [1.5, down(1.5), up(1.5), 0.05, 0.005, 3.0, 0.3, 1.0, 2.0]
    bg[:, 2] = [fcst_last, down(fcst_last), up(fcst_last), 0.3, 0.005, 1.0, 2.0, 0.05, 60.0]
    bg[:, 3] = [0.005, 0.05, 0.3, 1.5, 3.0, -0.0, np.inf, np.nan, 60.0]
    lons, lats = np.meshgrid(np.arange(4) * 40000.0, np.arange(rows, dtype=np.float64))
    fx = Fixture("thresholds", lats, lons, py, px, pobs, pbg, bg, minq=0.0, maxq=1.0, min_points=THRESHOLD_MIN_POINTS)
    fx.first, fx.fcst_last = first, fcst_last
    return fx


# the tag of every cell of `thresholds`, column by column, as its docstring derives them
THRESHOLD_TAGS = {
    "dry": (R.B1, R.B2A, R.B2C, R.B2B, R.B1, R.INVALID, R.INVALID, R.B2A, R.B2B),
    "half": (R.B2C, R.B2A, R.B2C, R.B2A, R.B1, R.B2C, R.B2A, R.B2A, R.B2C),
    "wet": (R.B3, R.B4, R.B3, R.B4, R.B1, R.B4, R.B4, R.B4, R.B3),
    "few": (R.FEW,) * 5 + (R.FEW, R.INVALID, R.INVALID, R.FEW),
}


# ---- 4. membership ------------------------------------------------------------------------------------------------------------------
MEMBER_XY = ((3000.0, 4000.0), (-3000.0, -4000.0), (5000.0, 0.0), (0.0, 5000.0), (4999.5, 0.0), (3000.5, 4000.0))


@functools.lru_cache(maxsize=None)
def membership(kind="Barnes"):
    """A 1 x 2 grid: cell 0 at the origin, cell 1 100 km away (no neighbour); six stations at MEMBER_XY, T = 2.
    Barnes: BarnesStructure(2 500, 0, 0, 5 000), whose localization distance is 5 000 m.
    Linear: LinearStructure(2 500), whose localization distance is 0 -- no cell has a neighbour."""
    rng = np.random.default_rng(31)
    px, py = np.array([a for a, _ in MEMBER_XY]), np.array([b for _, b in MEMBER_XY])
    pobs, pbg = rng.gamma(0.6, 3, (2, 6)).astype(F), rng.gamma(0.6, 3, (2, 6)).astype(F)
    structure = ("Barnes", 2500.0, 0.0, 0.0, 5000.0) if kind == "Barnes" else ("Linear", 2500.0, 0.0, 0.0, float("nan"))
    bg = np.array([[0.5 * float(pbg.max()), 0.05]], F)
    return Fixture("membership-" + kind, [[0.0, 0.0]], [[0.0, 100000.0]], py, px, pobs, pbg, bg, structure=structure, minq=0.0, maxq=1.0)
