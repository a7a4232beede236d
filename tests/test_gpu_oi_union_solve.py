"""The solve side of k_oi_union (csrc/oi_union.h: elimination, export, late columns, the pivot test, and the ownership mask of the bulk
disc in front of them) against the CPU oracle on single tiles whose union is BUILT: every case first derives each cell's selection in numpy (within the
localization radius, the max_points largest rho, ties to the lower index), from it the core size c (observations every updating cell of
the tile selected), the number of extras nE (selected by some cell only) and the largest extras count of a cell, and asserts the values
the case was built for -- a case cannot pass without reaching its edge.

Geometry: 8 x 8 cells 100 m apart (one tile) at 0.5 N 0.5 E, BarnesStructure(1000): localization radius R = 3 645 m.  Core observations lie
within 2 km of the tile centre, inside R of every cell.  An extras observation sits at R + s from the centre in direction theta: it reaches
the cells whose offset from the centre along theta exceeds s, i.e. whole columns (rows) from one side -- the circle bends by 17 m over the
tile, the cuts lie 50 m from the nearest cell, and the derivation asserts that no cell is within 10 m of R of any observation (float32
coordinates on the sphere carry 0.5 m).  Cells that two sides would reach together are taken out with a NaN background where a case needs
few extras per cell.

With max_points <= 32 a cell holds c + (its extras) <= 32 observations, so of nE in {1, 5, 12} x u in {30, 31, 32, 33, 36, 40} the unions with
c = u - nE > 31 do not exist on the 32-column form: nE = 1 with u >= 33 and nE = 5 with u = 40.  Every other combination is a case.

Tolerances as tests/test_gpu_oi_union_valu.py: RTOL 1e-5 over a floor of 1e-3, NaN pattern equal; "same bits" is np.array_equal."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-5
H = 1000.0
DX = 100.0
LAT0 = LON0 = 0.5
RE = 6.378137e6
M_PER_DEG = RE * np.pi / 180.0


def _check(out, ref):
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert (np.isnan(out) == np.isnan(ref)).all()
    m = ~np.isnan(ref)
    err = np.max(np.abs(out[m].astype(np.float64) - ref[m]) / np.maximum(np.abs(ref[m]), 1e-3)) if m.any() else 0.0
    print("max rel err %.3g" % err)
    assert err < RTOL


def _latlon(x, y):
    """metres east / north of the tile's first cell -> degrees"""
    return LAT0 + np.asarray(y, np.float64) / M_PER_DEG, LON0 + np.asarray(x, np.float64) / (M_PER_DEG * np.cos(np.deg2rad(LAT0)))


def _xyz(lat, lon):
    """the library's coordinates: float32 degrees, double trigonometry, float32 store"""
    la, lo = np.deg2rad(np.asarray(lat, np.float32).astype(np.float64)), np.deg2rad(np.asarray(lon, np.float32).astype(np.float64))
    return np.stack([np.cos(la) * np.cos(lo) * RE, np.cos(la) * np.sin(lo) * RE, np.sin(la) * RE], -1).astype(np.float32).astype(np.float64)


def _radius(h=H):
    from oracle import oracle as O
    return O.Barnes(h).localization_distance()


# ---- building a tile ---------------------------------------------------------------------------------------------------------------------
LEFT, RIGHT, BOTTOM, TOP = 180.0, 0.0, 270.0, 90.0


def _side(theta, depths, spread=1.0):
    """extras observations from one side: the k-th reaches the first depths[k] + 1 columns (rows) from that side; `spread` degrees apart"""
    n = len(depths)
    return [(theta + spread * (k - 0.5 * (n - 1)), 300.0 - 100.0 * d) for k, d in enumerate(depths)]


def _tile_case(ncore, extras, nan_cells=(), seed=0, n=8):
    """n x n cells, ncore observations every cell reaches, the extras as (theta, s) pairs; nan_cells: (x, y) cells without a background"""
    rng = np.random.default_rng(9000 + seed)
    R = _radius()
    xs, ys = np.meshgrid(np.arange(n) * DX, np.arange(n) * DX)      # [y][x]
    lats, lons = _latlon(xs, ys)
    ctr = 0.5 * (n - 1) * DX
    r, t = 2000.0 * np.sqrt(rng.random(ncore)), 2 * np.pi * rng.random(ncore)
    ox, oy = list(ctr + r * np.cos(t)), list(ctr + r * np.sin(t))
    for theta, s in extras:
        ox.append(ctr + (R + s) * np.cos(np.deg2rad(theta)))
        oy.append(ctr + (R + s) * np.sin(np.deg2rad(theta)))
    order = rng.permutation(len(ox))                                 # (the extras anywhere among the observation indices)
    plat, plon = _latlon(np.array(ox)[order], np.array(oy)[order])
    S = len(ox)
    bg = rng.normal(0, 1, (n, n)).astype(np.float32)
    for x, y in nan_cells:
        bg[y, x] = np.nan
    obs, pbg = rng.normal(0, 1, S).astype(np.float32), rng.normal(0, 1, S).astype(np.float32)
    ratios = rng.uniform(0.1, 1, S).astype(np.float32)
    return dict(lats=lats, lons=lons, plat=plat, plon=plon, bg=bg, obs=obs, pbg=pbg, ratios=ratios)


def _selections(c, mp, h=H):
    """per cell (flat index): the set of observation indices oi.cpp:229-273 selects; None for a cell without a valid background"""
    R = _radius(h)
    g, o = _xyz(c["lats"].ravel(), c["lons"].ravel()), _xyz(c["plat"], c["plon"])
    d = np.sqrt(((g[:, None, :] - o[None, :, :]) ** 2).sum(-1))
    assert np.abs(d - R).min() > 10.0, "a cell within 10 m of the localization radius of an observation: the selection is not decided by the geometry"
    rho = np.exp(-0.5 * (d / h) ** 2)
    sel = []
    for i, b in enumerate(c["bg"].ravel()):
        if not np.isfinite(b):
            sel.append(None)
            continue
        idx = np.nonzero(d[i] <= R)[0]
        idx = idx[np.lexsort((idx, -rho[i, idx]))][:mp]
        sel.append(frozenset(idx.tolist()))
    return sel


def _union(sel):
    """(c, nE, smallest and largest extras count of a cell) over the cells of `sel` that update"""
    live = [s for s in sel if s]
    core, union = frozenset.intersection(*live), frozenset.union(*live)
    m = [len(s) - len(core) for s in live]
    return len(core), len(union) - len(core), min(m), max(m)


def _oracle(c, mp, h=H):
    from oracle import oracle as O
    og, op = O.Pts(c["lats"].ravel(), c["lons"].ravel()), O.Pts(c["plat"], c["plon"])
    return O.oi(og, c["bg"].ravel(), op, c["obs"], c["ratios"], c["pbg"], O.Barnes(h), mp).reshape(c["bg"].shape)


def _run_twice(c, mp, h=H):
    """two calls on one pair of handles: the first call's analysis; the second must return the same bits.  The tile was not declined."""
    import gridpp_amd as gridpp
    grid, points, st = gridpp.Grid(c["lats"], c["lons"]), gridpp.Points(c["plat"], c["plon"]), gridpp.BarnesStructure(h)
    out = np.asarray(gridpp.optimal_interpolation(grid, c["bg"], points, c["obs"], c["ratios"], c["pbg"], st, mp))
    s = gridpp.oi_last_stats()
    print(s)
    assert s["union_kernel_ms"] > 0 and s["fallback_tiles"] == 0 and s["solves"] == 1, s      # one tile, one shared factorisation
    out2 = np.asarray(gridpp.optimal_interpolation(grid, c["bg"], points, c["obs"], c["ratios"], c["pbg"], st, mp))
    assert np.array_equal(out, out2, equal_nan=True)
    return out


# ---- core only: c = 1 ... 32 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", range(1, 33))
def test_core_only(c):
    """every column count of the elimination: both alignments of the first broadcast pair behind a column, u < 32 and u = 32, the last
    export column"""
    case = _tile_case(c, [], seed=c)
    assert _union(_selections(case, 32)) == (c, 0, 0, 0)
    _check(_run_twice(case, 32), _oracle(case, 32))


# ---- extras -------------------------------------------------------------------------------------------------------------------------------
CORNERS = ((0, 0), (7, 0), (0, 7), (7, 7))
# nE -> {u -> (extras, cells without a background, largest extras count of a cell)}
_E1 = _side(LEFT, [2])
_E5 = _side(LEFT, [0, 1, 2]) + _side(RIGHT, [0, 1])
# (u = 36 with five extras: c = 31, one extra per cell at most -- the four sides one column / row deep without the corners, and one from the
#  south-west that reaches cell (1, 1) alone once the five cells before it have no background)
_E5_ONE = _side(LEFT, [0]) + _side(RIGHT, [0]) + _side(BOTTOM, [0]) + _side(TOP, [0]) + [(225.0, 320.0)]
_E5_ONE_NAN = CORNERS + ((1, 0), (0, 1), (2, 0), (0, 2))
_E12 = _side(LEFT, [0, 0, 1, 1, 2, 2]) + _side(RIGHT, [0, 0, 1, 1, 2, 2])
# (u = 40: c = 28, four extras per cell at most -- three per side, the corners without a background: three per cell)
_E12_SIDES = _side(LEFT, [0, 0, 0]) + _side(RIGHT, [0, 0, 0]) + _side(BOTTOM, [0, 0, 0]) + _side(TOP, [0, 0, 0])
EXTRAS = {
    (1, 30): (_E1, (), 1),          # c = 29 = 4 k + 1 with ONE extras row: the per-cell finish reads past d' (the three zeros behind it)
    (1, 31): (_E1, (), 1),
    (1, 32): (_E1, (), 1),
    (5, 31): (_E5, (), 3),
    (5, 32): (_E5, (), 3),
    (5, 33): (_E5, (), 3),          # one late column
    (5, 36): (_E5_ONE, _E5_ONE_NAN, 1),   # four late columns
    (12, 31): (_E12, (), 6),
    (12, 32): (_E12, (), 6),
    (12, 33): (_E12, (), 6),
    (12, 36): (_E12, (), 6),
    (12, 40): (_E12_SIDES, CORNERS, 3),   # eight late columns
}


@functools.lru_cache(maxsize=None)
def _extras_case(nE, u):
    extras, nan_cells, mmax = EXTRAS[(nE, u)]
    case = _tile_case(u - nE, extras, nan_cells, seed=100 * nE + u)
    # (a cell has no extras, a cell has the largest count the case was built for; c is even and odd over the cases)
    assert _union(_selections(case, 32)) == (u - nE, nE, 0, mmax)
    return case


@functools.lru_cache(maxsize=None)
def _extras_plain(nE, u):
    return _run_twice(_extras_case(nE, u), 32)


def test_extras_cover_their_edges():
    cs = [u - nE for nE, u in EXTRAS]
    assert any(c % 2 == 0 for c in cs) and any(c % 2 == 1 for c in cs)                 # the padding element of B's odd stride: written / not needed
    assert {max(0, u - 32) for _, u in EXTRAS} >= {0, 1, 4, 8}                          # late columns
    assert any(nE == 1 and (u - nE) % 4 == 1 for nE, u in EXTRAS)                       # the read past the last row of B
    assert max(m for _, _, m in EXTRAS.values()) == 6


@pytest.mark.parametrize("nE,u", sorted(EXTRAS))
def test_extras(nE, u):
    case = _extras_case(nE, u)
    _check(_extras_plain(nE, u), _oracle(case, 32))


@pytest.mark.parametrize("nE,u", sorted(EXTRAS))
def test_extras_with_variance(nE, u):
    """the same tiles with a variance output: the analysis has the same bits with and without"""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c = _extras_case(nE, u)
    S = c["plat"].size
    bvar, bvp = np.random.default_rng(u).uniform(0.5, 2, c["bg"].shape).astype(np.float32), np.ones(S, np.float32)
    grid, points, st = gridpp.Grid(c["lats"], c["lons"]), gridpp.Points(c["plat"], c["plon"]), gridpp.BarnesStructure(H)
    out, var = gridpp.optimal_interpolation_full(grid, c["bg"], bvar, points, c["obs"], c["ratios"], c["pbg"], bvp, st, 32)
    s = gridpp.oi_last_stats()
    assert s["union_kernel_ms"] > 0 and s["fallback_tiles"] == 0 and s["solves"] == 1, s
    out, var = np.asarray(out), np.asarray(var)
    assert np.array_equal(_extras_plain(nE, u), out, equal_nan=True)
    og, op = O.Pts(c["lats"].ravel(), c["lons"].ravel()), O.Pts(c["plat"], c["plon"])
    ref, rvar = O.oi_full(og, c["bg"].ravel(), bvar.ravel(), op, c["obs"], c["ratios"], c["pbg"], bvp, O.Barnes(H), 32)
    _check(out, ref.reshape(out.shape))
    _check(var, rvar.reshape(var.shape))
    out2, var2 = gridpp.optimal_interpolation_full(grid, c["bg"], bvar, points, c["obs"], c["ratios"], c["pbg"], bvp, st, 32)
    assert np.array_equal(out, np.asarray(out2), equal_nan=True) and np.array_equal(var, np.asarray(var2), equal_nan=True)


# ---- the 48- and 64-column forms ------------------------------------------------------------------------------------------------------------
def test_max_points_40_with_late_columns():
    """48 register columns + late columns: c = 37, twelve extras (three per cell at most: 40 observations), u = 49 -- one late column"""
    case = _tile_case(37, _E12_SIDES, CORNERS, seed=40)
    assert _union(_selections(case, 40)) == (37, 12, 0, 3)
    _check(_run_twice(case, 40), _oracle(case, 40))


def test_max_points_56_at_the_row_limit():
    """64 register columns: its 62 rows all fit the registers (this form has no late columns), so the case fills them -- c = 50, twelve
    extras, six of them in a cell (56 observations), u = 62: elimination and export of the last column the form has"""
    case = _tile_case(50, _E12, (), seed=56)
    assert _union(_selections(case, 56)) == (50, 12, 0, 6)
    _check(_run_twice(case, 56), _oracle(case, 56))


# ---- spatially varying Barnes: a declined tile through the list passes -------------------------------------------------------------------
def test_spatially_varying_barnes_declined_tile_through_the_list_passes():
    """a length-scale FIELD (the same 1 000 m everywhere, so that the selection stays the one derived here) takes the tile to k_oi_union_sp;
    seven extras in the cells of column 0 are one more than a cell may have: the tile is declined, and its 4-cell items -- columns 0..3 of a
    row hold six extras at most -- are finished by the list passes k_oi_union<true, true, 32, SP>: nothing is left to k_oi"""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c = _tile_case(20, _side(LEFT, [0, 0, 1, 1, 2, 2, 3]) + _side(RIGHT, [0, 1]), seed=77)
    sel = _selections(c, 32)
    assert _union(sel) == (20, 9, 0, 7)
    for i in range(0, 64, 4):                                     # the 4-cell items: four consecutive cells of a row
        cc, nE, _, mmax = _union(sel[i:i + 4])
        assert nE <= 12 and mmax <= 6 and cc + nE <= 40
    hf = np.full((8, 8), H, np.float32)
    z = np.zeros_like(hf)
    grid, points = gridpp.Grid(c["lats"], c["lons"]), gridpp.Points(c["plat"], c["plon"])
    st = gridpp.BarnesStructure(grid, hf, z, z)
    out = np.asarray(gridpp.optimal_interpolation(grid, c["bg"], points, c["obs"], c["ratios"], c["pbg"], st, 32))
    s = gridpp.oi_last_stats()
    print(s)
    assert s["union_kernel_ms"] > 0 and s["fallback_tiles"] == 1 and s["fallback_subtiles"] == 0, s
    S = c["plat"].size
    og, op = O.Pts(c["lats"].ravel(), c["lons"].ravel()), O.Pts(c["plat"], c["plon"])
    R = np.float32(O.structure_localization("Barnes", H, 0.0013))
    par = lambda n: [np.full(n, H, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.full(n, R, np.float32)]
    ref, _ = O.oi_full_generic(og, c["bg"].ravel(), np.ones(64, np.float32), op, c["obs"], c["ratios"], c["pbg"], np.ones(S, np.float32),
                               O.Struct("Barnes", H), 32, True, par(64), par(S))
    _check(out, np.asarray(ref).reshape(8, 8))
    out2 = np.asarray(gridpp.optimal_interpolation(grid, c["bg"], points, c["obs"], c["ratios"], c["pbg"], st, 32))
    assert np.array_equal(out, out2, equal_nan=True)


# ---- a pivot that is not positive -----------------------------------------------------------------------------------------------------------
def test_non_positive_pivot():
    """two observations at the same place with ratio 0: their rows of P + R are equal, the second one's pivot is 1 - 1 * 1 = 0.  The
    factorisation reports it, the call is redone with the pivoted LU, which meets the same zero: the library raises, as the oracle does and
    as it did before the elimination's reads changed.  The next call is clean."""
    import gridpp_amd as gridpp
    from oracle import oracle as O
    c = _tile_case(6, [], seed=5)
    for k in ("plat", "plon"):
        c[k][1] = c[k][0]
    c["ratios"][:2] = 0.0
    assert _union(_selections(c, 32)) == (6, 0, 0, 0)
    with pytest.raises(O.OracleSingular):
        _oracle(c, 32)
    grid, points, st = gridpp.Grid(c["lats"], c["lons"]), gridpp.Points(c["plat"], c["plon"]), gridpp.BarnesStructure(H)
    with pytest.raises(RuntimeError, match="singular"):
        gridpp.optimal_interpolation(grid, c["bg"], points, c["obs"], c["ratios"], c["pbg"], st, 32)
    ok = _tile_case(6, [], seed=5)
    _check(_run_twice(ok, 32), _oracle(ok, 32))
