"""k_oi_union with fewer vector instructions per tile (csrc/oi_union.h, csrc/oi_common.h) against the CPU oracle, at the smallest shapes where
each change can go wrong:

- slot ownership during the bulk disc: candidates usable for part of a tile, NaN backgrounds, a vertical factor that underflows to zero
  (the rescaled exponential at its cut), the 48- and 64-column forms, and the masks the bulk disc leaves behind meeting evictions and
  slot recycling;
- ring candidates left as soon as no cell has them inside its threshold, with equal rho (the lower observation index wins);
- 1 - K G^T accumulated only when a variance is asked for: the analysis has the same bits with and without;
- unions beyond 32 rows (late columns) through the shared factorisation.

Tolerances as tests/test_gpu_oi_tile_path.py: RTOL 1e-5 over a floor of 1e-3, NaN pattern equal; "same bits" is np.array_equal."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-5


def _check(out, ref):
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert (np.isnan(out) == np.isnan(ref)).all()
    m = ~np.isnan(ref)
    err = np.max(np.abs(out[m].astype(np.float64) - ref[m]) / np.maximum(np.abs(ref[m]), 1e-3)) if m.any() else 0.0
    print("max rel err %.3g" % err)
    assert err < RTOL


def _fields(rng, shape, S):
    bg = rng.normal(0, 1, shape).astype(np.float32)
    return bg, rng.normal(0, 1, S).astype(np.float32), rng.normal(0, 1, S).astype(np.float32), rng.uniform(0.1, 1, S).astype(np.float32)


def _oracle(c, h, mp, v=0):
    from oracle import oracle as O
    og = O.Pts(np.ravel(c["lats"]), np.ravel(c["lons"]), None if c["ge"] is None else np.ravel(c["ge"]))
    op = O.Pts(c["plat"], c["plon"], c["pe"])
    return O.oi(og, c["bg"].ravel(), op, c["obs"], c["ratios"], c["pbg"], O.Barnes(h, v, 0), mp).reshape(c["bg"].shape)


def _run_twice(c, h, mp, v=0):
    """two calls on one Grid handle: the first call's analysis and statistics; the second call must return the same bits"""
    import gridpp_amd as gridpp
    grid = gridpp.Grid(c["lats"], c["lons"]) if c["ge"] is None else gridpp.Grid(c["lats"], c["lons"], c["ge"])
    points = gridpp.Points(c["plat"], c["plon"]) if c["pe"] is None else gridpp.Points(c["plat"], c["plon"], c["pe"])
    st = gridpp.BarnesStructure(h, v) if v else gridpp.BarnesStructure(h)
    out = np.asarray(gridpp.optimal_interpolation(grid, c["bg"], points, c["obs"], c["ratios"], c["pbg"], st, mp))
    s = gridpp.oi_last_stats()
    print(s)
    assert s["union_kernel_ms"] > 0      # (the tile kernel ran)
    out2 = np.asarray(gridpp.optimal_interpolation(grid, c["bg"], points, c["obs"], c["ratios"], c["pbg"], st, mp))
    assert np.array_equal(out, out2, equal_nan=True)
    return out, s


# ---- sparse observations: bulk candidates some cells of a tile cannot use ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sparse_case(variant):
    """37 x 53 cells over one degree (8 x 8 tiles of ~20 km), 60 observations, BarnesStructure(2000): the localization radius is ~7 km, so
    a candidate is usable for part of a tile only and most cells stay below max_points."""
    rng = np.random.default_rng(7301)
    Y, X, S = 37, 53, 60
    lats, lons = np.meshgrid(np.linspace(0, 1, Y), np.linspace(0, 1, X), indexing="ij")
    plat, plon = rng.random(S), rng.random(S)
    bg, obs, pbg, ratios = _fields(rng, (Y, X), S)
    ge = pe = None
    if variant == "nan":        # 20 % NaN backgrounds; tile (2, 5) keeps ONE valid cell, beside an observation so that it has something to do
        bg[rng.random(bg.shape) < 0.2] = np.nan
        keep = bg[19, 42] if np.isfinite(bg[19, 42]) else np.float32(0.25)
        bg[16:24, 40:48] = np.nan
        bg[19, 42] = keep
        plat[0], plon[0] = lats[19, 42] + 0.01, lons[19, 42] - 0.01
    if variant == "elev":       # elevations over 4 km against v = 200 m: beyond 15 v the vertical factor is 0 in float32
        ge = rng.uniform(0, 4000, (Y, X)).astype(np.float32)
        pe = rng.uniform(0, 4000, S).astype(np.float32)
    return dict(lats=lats, lons=lons, plat=plat, plon=plon, bg=bg, obs=obs, ratios=ratios, pbg=pbg, ge=ge, pe=pe)


@pytest.mark.parametrize("variant", ["plain", "nan", "elev"])
def test_bulk_candidates_usable_for_part_of_a_tile(variant):
    c = _sparse_case(variant)
    v = 200 if variant == "elev" else 0
    out, s = _run_twice(c, 2000, 30, v)
    ref = _oracle(c, 2000, 30, v)
    _check(out, ref)
    changed = np.isfinite(ref) & (ref != c["bg"])
    assert 0 < changed.sum() < changed.size      # (some cells updated, some out of every observation's reach)


@pytest.mark.parametrize("mp", [40, 55])
def test_bulk_candidates_usable_for_part_of_a_tile_wider_forms(mp):
    """the same geometry on the 48-column (max_points 40) and the 64-column form (55)"""
    c = _sparse_case("plain")
    out, s = _run_twice(c, 2000, mp)
    _check(out, _oracle(c, 2000, mp))


# ---- dense observations: all slots in use, equal rho, late columns ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_case(dup):
    """32 x 32 cells over 0.01 x 0.01 degrees inside 3 000 observations over the unit square; dup: 200 of them once more at identical
    coordinates under higher indices."""
    rng = np.random.default_rng(7302)
    S = 3000
    lats, lons = np.meshgrid(np.linspace(0.5, 0.51, 32), np.linspace(0.5, 0.51, 32), indexing="ij")
    plat, plon = rng.random(S), rng.random(S)
    if dup:
        # (the 200 nearest to the grid, so that the copies are among the candidates the cells choose from)
        near = np.argsort((plat - 0.505) ** 2 + (plon - 0.505) ** 2)[:200]
        plat, plon = np.concatenate([plat, plat[near]]), np.concatenate([plon, plon[near]])
        S += 200
    bg, obs, pbg, ratios = _fields(rng, (32, 32), S)
    return dict(lats=lats, lons=lons, plat=plat, plon=plon, bg=bg, obs=obs, ratios=ratios, pbg=pbg, ge=None, pe=None)


def test_all_slots_in_use():
    """more candidates than max_points around every tile: evictions, slots >= 32, recycling of the slots no cell holds any more -- the masks
    of the bulk disc meet the eviction path"""
    c = _dense_case(False)
    out, s = _run_twice(c, 10000, 30)
    _check(out, _oracle(c, 10000, 30))


def test_ring_candidates_with_equal_rho():
    """duplicated observations: equal rho in the rings behind the bulk disc, where a candidate no cell has inside its threshold is left
    early; the lower observation index wins, as in the oracle"""
    c = _dense_case(True)
    out, s = _run_twice(c, 10000, 30)
    _check(out, _oracle(c, 10000, 30))


@pytest.mark.parametrize("mp", [30, 47])
def test_late_columns(mp):
    """a longer length scale: the rho values of a tile's cells lie closer together, the unions exceed 32 rows -- columns 32.. wait in LDS
    during the elimination (47: the 48-column form).  The shared factorisation really ran: not every tile was declined."""
    c = _dense_case(False)
    out, s = _run_twice(c, 20000, mp)
    assert s["fallback_tiles"] < 16, s
    _check(out, _oracle(c, 20000, mp))


# ---- with and without a variance output -----------------------------------------------------------------------------------------------
def test_analysis_has_the_same_bits_with_and_without_variance():
    import gridpp_amd as gridpp
    from oracle import oracle as O
    rng = np.random.default_rng(7303)
    Y, X, S = 37, 53, 400
    lats, lons = np.meshgrid(np.linspace(0, 1, Y), np.linspace(0, 1, X), indexing="ij")
    plat, plon = rng.random(S), rng.random(S)
    bg, obs, pbg, ratios = _fields(rng, (Y, X), S)
    # (background variance at the points 1: optimal_interpolation_full then works with the ratios optimal_interpolation is given)
    bvar, bvp = rng.uniform(0.5, 2, (Y, X)).astype(np.float32), np.ones(S, np.float32)
    grid, points, st = gridpp.Grid(lats, lons), gridpp.Points(plat, plon), gridpp.BarnesStructure(10000)
    plain = np.asarray(gridpp.optimal_interpolation(grid, bg, points, obs, ratios, pbg, st, 30))
    s = gridpp.oi_last_stats()
    assert s["union_kernel_ms"] > 0
    # (fresh handles: a repeated call with the same points and structure may skip the first pass when most of its tiles were declined before --
    #  the variance call has to run the tile kernel itself)
    grid, points = gridpp.Grid(lats, lons), gridpp.Points(plat, plon)
    out, var = gridpp.optimal_interpolation_full(grid, bg, bvar, points, obs, ratios, pbg, bvp, st, 30)
    s = gridpp.oi_last_stats()
    print(s)
    assert s["union_kernel_ms"] > 0
    out, var = np.asarray(out), np.asarray(var)
    assert np.array_equal(plain, out, equal_nan=True)
    og, op = O.Pts(lats.ravel(), lons.ravel()), O.Pts(plat, plon)
    ref, rvar = O.oi_full(og, bg.ravel(), bvar.ravel(), op, obs, ratios, pbg, bvp, O.Barnes(10000), 30)
    _check(out, ref.reshape(Y, X))
    _check(var, rvar.reshape(Y, X))
    out2, var2 = gridpp.optimal_interpolation_full(grid, bg, bvar, points, obs, ratios, pbg, bvp, st, 30)
    assert np.array_equal(out, np.asarray(out2), equal_nan=True) and np.array_equal(var, np.asarray(var2), equal_nan=True)
