"""Cases of the OI gain edge suites (tests/test_gpu_oi_gain_edges.py on the GPU, tests/test_oi_gain_cases_oracle.py on the CPU), the plain
references they are compared with, and the conditions that keep them from passing vacuously.  Nothing here imports the GPU package; what
is computed from the oracle is computed once per case and handed out read-only.

What gridpp_amd/csrc/oi_gain.hip can get wrong and which case looks there:

    chain / chain_permuted / cressman_chain
                twelve stations on a line whose well-trusted stations (ratio 0.05) sit next to poorly trusted ones (ratio 1): the
                Gauss-Jordan inversion of k_oi_gain_build leaves the diagonal at most steps (gj_pivot_order restates its pivot rule), so
                the re-ordering of the rows (M[j][mystep]), the slot a weight is written to (pj) and the rho it meets in a = w . g all
                differ from the identity.  The weights are pinned to 1e-9 max|w| against numpy.linalg.solve in double
    tile_shapes / line grids
                a 13 x 70 grid under every GPP_TILE_WSHIFT (tiles of 64 x 1 ... 1 x 64 cells: 13 is no multiple of a tile height, 70 a
                partial second tile of the widest), and grids of one row or one column (the ny < 2 || nx < 2 branch of gpp_tile_wshift)
    wide        max_points 62 on elevation and land-area fraction, selection sizes in every residue mod 8 and 62 itself: the slot loop of
                k_oi_gain_apply_wide (eight at a time, past n) and its lane clamp at 15 ... 129 fields, against apply_reference
    sizes       Points backgrounds of 1, 63, 64 and 65 points and max_points 32, the last size on the 32-slot lists"""
import functools

import numpy as np

F = np.float32
GEODETIC, CARTESIAN = 0, 1
WEIGHT_RTOL = 1e-9          # |dw| <= WEIGHT_RTOL max|w| per cell: see tests/test_gpu_oi_gain_edges.py for the derivation
MIN_MARGIN, MAX_COND = 0.03, 200.0
MIN_OFF_DIAGONAL_SHARE = 0.25


def _o():
    from oracle import oracle as O
    return O


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def gj_pivot_order(A):
    """The pivot rule of k_oi_gain_build in float64: at step k the unused row with the largest |entry| in column k, the lowest row on a
    tie; every other row takes the unscaled pivot row with the multiplier entry / pivot.
    -> (pivot rows in the order of the steps, per step the relative margin (|winner| - |runner-up|) / |winner|; 1 at the last step)"""
    M = np.array(A, np.float64)
    n = M.shape[0]
    assert M.shape == (n, n)
    used = np.zeros(n, bool)
    order, margins = [], []
    for k in range(n):
        col = np.where(used, -1.0, np.abs(M[:, k]))
        p = int(np.argmax(col))                     # (the first of equal entries: the lowest row)
        runner = np.delete(col, p).max() if n > 1 else -1.0
        margins.append(1.0 if runner < 0 else (col[p] - runner) / col[p])
        f = M[:, k] / M[p, k]
        f[p] = 0.0
        M -= np.outer(f, M[p])
        used[p] = True
        order.append(p)
    return order, margins


class Case:
    """A background (a 2-D grid: lats = y, lons = x of the same 2-D shape; or 1-D: Points), stations, float32 ratios, a scalar structure
    (kind, h, v, w) and max_points."""

    def __init__(self, name, lats, lons, plat, plon, ratios, structure, max_points, gelev=None, glaf=None, pelev=None, plaf=None,
                 ctype=CARTESIAN):
        self.name, self.ctype, self.structure, self.max_points = name, ctype, structure, int(max_points)
        self.lats, self.lons = np.asarray(lats, np.float64), np.asarray(lons, np.float64)
        self.plat, self.plon = np.asarray(plat, np.float64), np.asarray(plon, np.float64)
        self.ratios = np.array(ratios, F)
        opt = lambda a: None if a is None else np.asarray(a, np.float64)
        self.gelev, self.glaf, self.pelev, self.plaf = opt(gelev), opt(glaf), opt(pelev), opt(plaf)
        self.shape, self.S = self.lats.shape, self.plat.size
        self.cells = int(np.prod(self.shape))
        assert self.lons.shape == self.shape and self.plon.size == self.S == self.ratios.size
        _ro(self.lats, self.lons, self.plat, self.plon, self.ratios)

    def __repr__(self):
        return self.name

    # ---- the oracle's side ----
    @functools.cached_property
    def oracle_points(self):
        O = _o()
        flat = lambda a: None if a is None else a.ravel()
        return (O.Pts(self.lats.ravel(), self.lons.ravel(), flat(self.gelev), flat(self.glaf), self.ctype),
                O.Pts(self.plat, self.plon, self.pelev, self.plaf, self.ctype))

    @functools.cached_property
    def oracle_structure(self):
        kind, h, v, w = self.structure
        return _o().Barnes(h, v, w) if kind == "Barnes" else _o().Struct(kind, h, v, w)

    @staticmethod
    def _pt(P, i):
        return (P.x[i], P.y[i], P.z[i], P.elevs[i], P.lafs[i])

    def _corr(self, p1, p2, background):
        st = self.oracle_structure
        return st.corr(p1, p2) if self.structure[0] == "Barnes" else st.corr(p1, p2, background)

    @functools.cached_property
    def selections(self):
        """-> (per cell the tuple of selected observation indices, ascending; per cell whether the cut straddles a tie).
        Barnes: O.oi_selection.  Another kernel (O.oi_selection is Barnes only): the reference's rule (oi.cpp:229-255) restated over the
        oracle's radius query and correlation, for cases with at most max_points stations -- nothing is cut, no tie can matter."""
        O = _o()
        og, op = self.oracle_points
        ones = np.ones(self.S, F)
        sels, ties = [], np.zeros(self.cells, bool)
        if self.structure[0] == "Barnes":
            for cell in range(self.cells):
                sel, ties[cell] = O.oi_selection(og, cell, op, ones, ones, self.oracle_structure, self.max_points)
                sels.append(tuple(sorted(int(i) for i in sel)))
        else:
            assert self.S <= self.max_points
            loc = self.oracle_structure.localization_distance()
            for cell in range(self.cells):
                near = O.get_neighbours(op, og.lats[cell], og.lons[cell], loc)
                sels.append(tuple(int(i) for i in near if self._corr(self._pt(og, cell), self._pt(op, i), True) > 0))
        return sels, _ro(ties)[0]

    @functools.cached_property
    def counts(self):
        return _ro(np.array([len(s) for s in self.selections[0]], np.int32).reshape(self.shape))[0]

    @functools.cached_property
    def groups(self):
        """distinct non-empty selection -> its cells"""
        out = {}
        for cell, sel in enumerate(self.selections[0]):
            if sel:
                out.setdefault(sel, []).append(cell)
        return out

    @functools.cached_property
    def station_corr(self):
        """corr(obs_i, obs_j) of every pair of stations, float32 values in a double matrix (small cases only)"""
        assert self.S <= 64
        op = self.oracle_points[1]
        return _ro(np.array([[self._corr(self._pt(op, i), self._pt(op, j), False) for j in range(self.S)] for i in range(self.S)],
                            np.float64))[0]

    def matrix(self, sel):
        """P + R of a selection in the gain's row order (ascending observation index): float32 correlations and ratios, in double"""
        sel = list(sel)
        return self.station_corr[np.ix_(sel, sel)] + np.diag(self.ratios[sel].astype(np.float64))

    def rho(self, cell, sel):
        """g of a cell: its float32 correlations with the selected observations, in double"""
        og, op = self.oracle_points
        return np.array([self._corr(self._pt(og, cell), self._pt(op, i), True) for i in sel], np.float64)

    @functools.cached_property
    def pivots(self):
        """distinct selection -> (pivot order, margins, cond(P + R))"""
        return {sel: gj_pivot_order(self.matrix(sel)) + (float(np.linalg.cond(self.matrix(sel))),) for sel in self.groups}

    @functools.cached_property
    def reference_weights(self):
        """(cells, max_points) weights w = solve((P + R)^T, g) in double, 0 behind the selection; (cells,) a = w . g"""
        w, a = np.zeros((self.cells, self.max_points)), np.zeros(self.cells)
        for sel, cells in self.groups.items():
            At = self.matrix(sel).T
            G = np.stack([self.rho(cell, sel) for cell in cells], axis=1)
            W = np.linalg.solve(At, G)
            w[cells, :len(sel)] = W.T
            a[cells] = (W * G).sum(axis=0)
        return _ro(w, a)

    def fields(self, E, seed=0):
        """-> background shape + (E,), pobs (S, E), pbackground (S, E), float32, read-only"""
        rng = np.random.default_rng([seed, E, self.S, self.cells])
        return _ro(rng.normal(0, 1, self.shape + (E,)).astype(F), rng.normal(0, 1, (self.S, E)).astype(F),
                   rng.normal(0, 1, (self.S, E)).astype(F))

    def oracle_analysis(self, bg, pobs, pbg, allow=True, variance=False):
        """one field by the oracle's optimal_interpolation (unit variances: ratios = obs_variance) -> analysis [, variance]"""
        O = _o()
        og, op = self.oracle_points
        ones_g, ones_p = np.ones(self.cells, F), np.ones(self.S, F)
        if self.structure[0] == "Barnes":
            out, var = O.oi_full(og, np.ravel(bg), ones_g, op, pobs, self.ratios, pbg, ones_p, self.oracle_structure, self.max_points, allow)
        else:
            out, var = O.oi_full_generic(og, np.ravel(bg), ones_g, op, pobs, self.ratios, pbg, ones_p, self.oracle_structure,
                                         self.max_points, allow)
        out, var = out.reshape(self.shape), var.reshape(self.shape)
        return (out, var) if variance else out

    # ---- the device's side ----
    def device(self, gridpp):
        """-> (Grid or Points, Points, structure) of the GPU package, built anew"""
        e = lambda a: () if a is None else a
        if len(self.shape) == 2:
            bgrid = gridpp.Grid(self.lats, self.lons, ((),) if self.gelev is None else self.gelev, ((),) if self.glaf is None else self.glaf,
                                self.ctype)
        else:
            bgrid = gridpp.Points(self.lats, self.lons, e(self.gelev), e(self.glaf), self.ctype)
        points = gridpp.Points(self.plat, self.plon, e(self.pelev), e(self.plaf), self.ctype)
        kind, h, v, w = self.structure
        return bgrid, points, getattr(gridpp, kind + "Structure")(h, v, w)


# ---- the plain reference of an apply ---------------------------------------------------------------------------------------------------
def apply_reference(counts, indices, weights, bg, pobs, pbg, allow):
    """gain.apply in numpy from the gain's OWN selection and weights (it tests the apply kernels, not the build):
    d = float64(pobs) - float64(pbg); inc = float32(sum w d); the clamp of oi.cpp:318-334 on inc with the float32 extremes of the selected d;
    want = float32(bg) + inc in float32.  bg: cells x E (any leading shape), pobs / pbg: (S, E).
    -> (want, tolerance per element = spacing(|inc|) + spacing(|want|), changed: the elements an analysis touches -- the others pass through)"""
    E = bg.shape[-1]
    K = indices.shape[-1]
    n, idx, w = counts.reshape(-1), indices.reshape(-1, K), weights.reshape(-1, K)
    b = np.asarray(bg, F).reshape(-1, E)
    d = np.asarray(pobs, F).astype(np.float64) - np.asarray(pbg, F).astype(np.float64)
    acc = np.zeros(b.shape, np.float64)
    hi, lo = np.full(b.shape, -np.inf, F), np.full(b.shape, np.inf, F)
    for k in range(int(n.max(initial=0))):
        on = (k < n)[:, None]
        dk = d[np.where(k < n, idx[:, k], 0)]
        acc += np.where(on, w[:, k, None] * dk, 0.0)
        hi, lo = np.where(on, np.maximum(hi, dk.astype(F)), hi), np.where(on, np.minimum(lo, dk.astype(F)), lo)
    inc = acc.astype(F)
    if not allow:
        inc = np.select([(hi > 0) & (inc > hi), (hi < 0) & (inc > 0), (lo < 0) & (inc < lo), (lo > 0) & (inc < 0)], [hi, hi, lo, lo], inc)
    changed = (n > 0)[:, None] & np.isfinite(b)
    with np.errstate(invalid="ignore"):
        want = np.where(changed, b + inc, b).astype(F)
        tol = np.spacing(np.abs(inc)).astype(np.float64) + np.spacing(np.abs(np.where(changed, want, 0))).astype(np.float64)
    return want.reshape(bg.shape), tol.reshape(bg.shape), changed.reshape(bg.shape)


# ---- A. pivots that leave the diagonal -----------------------------------------------------------------------------------------------
CHAIN_STATIONS, CHAIN_SPACING, CHAIN_H = 12, 5000.0, 10000.0
CHAIN_RATIOS = (1.0, 0.05, 0.05, 0.05, 1.0, 1.0, 1.0, 0.05, 0.05, 0.05, 1.0, 0.05)   # by position along the line
CHAIN_GRID = (24, 40)
CHAIN_PERMUTATION = (1, 5, 0, 2, 11, 4, 8, 3, 6, 7, 9, 10)    # position along the line -> station index


def _chain_grid():
    """24 x 40 cells around the line y = 0, x = 0 ... 55 km: Barnes(10 000) reaches 36.46 km, the corners are 60 km from the nearest station"""
    lons, lats = np.meshgrid(np.linspace(-42000.0, 97000.0, CHAIN_GRID[1]), np.linspace(-45500.0, 44500.0, CHAIN_GRID[0]))
    return lats, lons


@functools.lru_cache(maxsize=None)
def chain(permuted=False):
    """Twelve stations 5 km apart on a line, BarnesStructure(10 000), ratios CHAIN_RATIOS along the line (stretches of three well-trusted
    stations between poorly trusted ones; found by a search over patterns with gj_pivot_order: with 0.05 at the even positions and at
    position 1 the stretches at the far end of the line win off-diagonal steps by 1.2 % only), max_points 12 = every station: no cut, no
    tie.  A cell selects the stations within 36.46 km, a stretch of the line.
    permuted: the station at position k of the line has index CHAIN_PERMUTATION[k]: the rows of P + R are not in geometric order."""
    lats, lons = _chain_grid()
    pos = np.arange(CHAIN_STATIONS)
    index = np.array(CHAIN_PERMUTATION) if permuted else pos
    px, ratios = np.empty(CHAIN_STATIONS), np.empty(CHAIN_STATIONS, F)
    px[index], ratios[index] = pos * CHAIN_SPACING, np.array(CHAIN_RATIOS, F)
    return Case("chain-permuted" if permuted else "chain", lats, lons, np.zeros(CHAIN_STATIONS), px, ratios,
                ("Barnes", CHAIN_H, 0.0, 0.0), CHAIN_STATIONS)


CRESSMAN = (30000.0, 300.0, 1.5)
CRESSMAN_SEED = 11482          # found by a search over seeds with gj_pivot_order (on the CPU): the conditions are asserted, not assumed
CRESSMAN_FULL_ORDER = [0, 1, 2, 3, 4, 5, 6, 9, 8, 7, 10, 11]


@functools.lru_cache(maxsize=None)
def cressman_chain():
    """The line of `chain` under CressmanStructure(30 000, 300, 1.5) with elevations and land-area fractions.  The vertical and laf factors
    are Cressman functions of SIGNED differences (structure.cpp:35-44: 0 for d >= L, (L^2 - d^2) / (L^2 + d^2) otherwise, which is
    NEGATIVE for d < -L).  Nine stations lie at 0 ... 100 m, three at 380 ... 450 m, the cells at 150 ... 300 m: a cell selects stations
    of both kinds, and for a low station i and a high one j corr(i, j) < 0 = corr(j, i) -- P is not symmetric.  Ratios 0.05 or 1."""
    lats, lons = _chain_grid()
    rng = np.random.default_rng(CRESSMAN_SEED)
    pelev = np.round(rng.uniform(0, 100, CHAIN_STATIONS))
    high = rng.choice(CHAIN_STATIONS, 3, replace=False)
    pelev[high] = np.round(rng.uniform(380, 450, 3))
    plaf = np.round(rng.uniform(0, 1, CHAIN_STATIONS), 2)
    ratios = np.where(rng.integers(0, 2, CHAIN_STATIONS) == 1, 1.0, 0.05).astype(F)
    gelev, glaf = rng.uniform(150, 300, CHAIN_GRID), rng.uniform(0, 1, CHAIN_GRID)
    return Case("cressman-chain", lats, lons, np.zeros(CHAIN_STATIONS), np.arange(CHAIN_STATIONS) * CHAIN_SPACING, ratios,
                ("Cressman",) + CRESSMAN, CHAIN_STATIONS, gelev=gelev, glaf=glaf, pelev=pelev, plaf=plaf)


# ---- B. tile shapes ------------------------------------------------------------------------------------------------------------------
TILE_SHIFTS = (0, 1, 2, 3, 4, 5, 6)          # GPP_TILE_WSHIFT: tiles of (64 >> w) x (1 << w) cells
TILE_GRID, TILE_STATIONS, TILE_H, TILE_MAX_POINTS = (13, 70), 120, 1500.0, 10
LINE_GRIDS = ((1, 70), (1, 9), (70, 1))


def _box_case(name, shape, S, h, max_points, seed):
    """a Cartesian grid of 1 km cells and S stations drawn uniformly from the box around it"""
    Y, X = shape
    rng = np.random.default_rng(seed)
    lons, lats = np.meshgrid(np.arange(X) * 1000.0, np.arange(Y) * 1000.0)
    px, py = rng.uniform(-3000.0, X * 1000.0 + 2000.0, S), rng.uniform(-3000.0, Y * 1000.0 + 2000.0, S)
    return Case(name, lats, lons, py, px, rng.uniform(0.1, 1, S).astype(F), ("Barnes", h, 0.0, 0.0), max_points)


@functools.lru_cache(maxsize=None)
def tile_shapes():
    """13 x 70 cells of 1 km, 120 stations, BarnesStructure(1 500) (it reaches 5.5 km), max_points 10"""
    return _box_case("tile-shapes", TILE_GRID, TILE_STATIONS, TILE_H, TILE_MAX_POINTS, 41)


@functools.lru_cache(maxsize=None)
def line_grid(shape):
    """a grid of one row or one column (gpp_tile_wshift: 1 x 64 tiles from 64 columns on, 8 x 8 tiles below)"""
    assert shape in LINE_GRIDS
    return _box_case("line-%dx%d" % shape, shape, 40, 2000.0, 10, 43 + shape[0] + shape[1])


# ---- C. field counts and selection sizes ---------------------------------------------------------------------------------------------
WIDE_FIELDS = (15, 16, 63, 64, 65, 128, 129)
WIDE_MAX_POINTS = 62


def _parity_case(name, seed, Y, X, S, structure, max_points, stretch=1.0):
    from tests.test_gpu_oi_parity import make_case
    c = make_case(seed, Y, X, S, with_elev=True)
    return Case(name, c["lats"], c["lons"] * stretch, c["plat"], c["plon"], c["ratios"], structure, max_points, c["gelev"], c["glaf"], c["pelev"],
                c["plaf"], GEODETIC)


@functools.lru_cache(maxsize=None)
def wide():
    """the 48 x 48 / 300-station case of tests/test_gpu_oi_gain_parity.py, BarnesStructure(10 000, 200, 0.5), max_points 62, with the grid
    stretched to 1.6 degrees of longitude: the stations stay within one degree, the structure reaches 36 km, and the eastern columns are
    cells without a selection (the unstretched grid has none)"""
    return _parity_case("wide", 11, 48, 48, 300, ("Barnes", 10000.0, 200.0, 0.5), WIDE_MAX_POINTS, stretch=1.6)


def wide_background(E):
    """fields of wide() with a NaN and an inf in the background at the last field and at field 64 (where there is one), each at a cell
    with a selection and at a cell without"""
    case = wide()
    bg, pobs, pbg = case.fields(E, seed=5)
    bg = bg.copy()
    # innovations of mostly one sign per field, the sign alternating from field to field, as in tests/test_gpu_oi_gain_parity.py: with
    # white noise the clamp of oi.cpp:318-334 binds at 3 elements in 10 000, with these at about 50
    sign = np.where(np.arange(E) % 2 == 0, 1.0, -1.0).astype(F)
    pobs = _ro((pbg + sign * np.abs(pobs) - F(0.2) * sign).astype(F))[0]
    with_sel, without = np.argwhere(case.counts > 0), np.argwhere(case.counts == 0)
    for e in sorted({E - 1, 64} & set(range(E))):
        (y0, x0), (y1, x1) = with_sel[7 + e], with_sel[-(11 + e)]
        bg[y0, x0, e], bg[y1, x1, e] = np.nan, np.inf
        if len(without):
            (y2, x2), (y3, x3) = without[0], without[-1]
            bg[y2, x2, e], bg[y3, x3, e] = np.inf, np.nan
    return _ro(bg)[0], pobs, pbg


# ---- D. sizes ------------------------------------------------------------------------------------------------------------------------
POINT_COUNTS = (1, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def points_background(n):
    """a Points background of n points (tiles of 64 consecutive points: one partial tile, exactly one, one and a point), 150 stations"""
    rng = np.random.default_rng(100 + n)
    S = 150
    return Case("points-%d" % n, rng.random(n), rng.random(n), rng.random(S), rng.random(S), rng.uniform(0.1, 1, S).astype(F),
                ("Barnes", 12000.0, 0.0, 0.0), 12, ctype=GEODETIC)


@functools.lru_cache(maxsize=None)
def max_points_32():
    """the case of wide() on a 20 x 24 grid with max_points 32: the last size that builds on the 32-slot lists"""
    return _parity_case("max-points-32", 11, 20, 24, 300, ("Barnes", 10000.0, 200.0, 0.5), 32)
