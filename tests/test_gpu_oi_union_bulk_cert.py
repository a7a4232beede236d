"""The certificate of the bulk disc in k_oi_union (csrc/oi_union.h, `cert`): when no record of the bulk disc can be farther from any active
cell of the item than the cells' smallest near_r (a few ulps inside the localization radius R) and than 12 h, every per-candidate test of the
bulk evaluations has one answer per lane, and a second form of the loop leaves them out.  Every case here is built for one side of that
decision and asserts the `bulk_certified` count it was built for, so it cannot pass without reaching its edge; every case runs a second time
under GPP_OI_NO_BULK_CERT, which must report bulk_certified == 0 and return THE SAME BITS.

Geometry as tests/test_gpu_oi_union_solve.py (its helpers, copied): one tile of 8 x 8 cells 100 m apart, BarnesStructure(1000), R = 3 645 m,
core observations within 2 km of the tile centre.  The case builders, their numpy derivations and the oracle calls need no GPU (they are
cached functions the tests call first).

Tolerances as there: RTOL 1e-5 over a floor of 1e-3 against the CPU oracle, NaN pattern equal; "same bits" is np.array_equal(equal_nan=True)."""
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
OVERRIDE = "GPP_OI_NO_BULK_CERT"


def _check(out, ref):
    out = np.asarray(out)
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert (np.isnan(out) == np.isnan(ref)).all()
    m = ~np.isnan(ref)
    err = np.max(np.abs(out[m].astype(np.float64) - ref[m]) / np.maximum(np.abs(ref[m]), 1e-3)) if m.any() else 0.0
    print("max rel err %.3g" % err)
    assert err < RTOL


def _latlon(x, y, lat0=LAT0, lon0=LON0):
    """metres east / north of the tile's first cell -> degrees"""
    return lat0 + np.asarray(y, np.float64) / M_PER_DEG, lon0 + np.asarray(x, np.float64) / (M_PER_DEG * np.cos(np.deg2rad(lat0)))


def _xyz(lat, lon):
    """the library's coordinates: float32 degrees, double trigonometry, float32 store"""
    la, lo = np.deg2rad(np.asarray(lat, np.float32).astype(np.float64)), np.deg2rad(np.asarray(lon, np.float32).astype(np.float64))
    return np.stack([np.cos(la) * np.cos(lo) * RE, np.cos(la) * np.sin(lo) * RE, np.sin(la) * RE], -1).astype(np.float32).astype(np.float64)


def _barnes(*st):
    from oracle import oracle as O
    return O.Barnes(*st)


LEFT, RIGHT = 180.0, 0.0


def _side(theta, depths, spread=1.0):
    """extras observations from one side: the k-th reaches the first depths[k] + 1 columns (rows) from that side; `spread` degrees apart"""
    n = len(depths)
    return [(theta + spread * (k - 0.5 * (n - 1)), 300.0 - 100.0 * d) for k, d in enumerate(depths)]


def _tile_case(ncore, extras, nan_cells=(), seed=0, ny=8, nx=8, rmin=0.0, rmax=2000.0, st=(H,), lat0=LAT0, lon0=LON0, shuffle=True):
    """ny x nx cells, ncore observations rmin .. rmax from the centre of the grid (uniform over the annulus), the extras as (theta, s) pairs at
    R + s from it; nan_cells: (x, y) cells without a background"""
    rng = np.random.default_rng(9000 + seed)
    R = _barnes(*st).localization_distance()
    xs, ys = np.meshgrid(np.arange(nx) * DX, np.arange(ny) * DX)      # [y][x]
    lats, lons = _latlon(xs, ys, lat0, lon0)
    cx, cy = 0.5 * (nx - 1) * DX, 0.5 * (ny - 1) * DX
    r, t = np.sqrt(rmin ** 2 + (rmax ** 2 - rmin ** 2) * rng.random(ncore)), 2 * np.pi * rng.random(ncore)
    ox, oy = list(cx + r * np.cos(t)), list(cy + r * np.sin(t))
    for theta, s in extras:
        ox.append(cx + (R + s) * np.cos(np.deg2rad(theta)))
        oy.append(cy + (R + s) * np.sin(np.deg2rad(theta)))
    order = rng.permutation(len(ox)) if shuffle else np.arange(len(ox))   # (the extras anywhere among the observation indices)
    plat, plon = _latlon(np.array(ox)[order], np.array(oy)[order], lat0, lon0)
    S = len(ox)
    bg = rng.normal(0, 1, (ny, nx)).astype(np.float32)
    for x, y in nan_cells:
        bg[y, x] = np.nan
    obs, pbg = rng.normal(0, 1, S).astype(np.float32), rng.normal(0, 1, S).astype(np.float32)
    ratios = rng.uniform(0.1, 1, S).astype(np.float32)
    return dict(lats=lats, lons=lons, plat=plat, plon=plon, bg=bg, obs=obs, pbg=pbg, ratios=ratios, st=tuple(st), elevs=None, pelevs=None)


def _dist(c):
    """(cells, observations) chord distances, and the localization radius of the case's structure"""
    g, o = _xyz(c["lats"].ravel(), c["lons"].ravel()), _xyz(c["plat"], c["plon"])
    d = np.sqrt(((g[:, None, :] - o[None, :, :]) ** 2).sum(-1))
    R = _barnes(*c["st"]).localization_distance()
    assert np.abs(d - R).min() > 10.0, "a cell within 10 m of the localization radius of an observation: the selection is not decided by the geometry"
    return d, R


def _selections(c, mp):
    """per cell (flat index): the set of observation indices oi.cpp:229-273 selects (horizontal factor only); None for a cell without a valid background"""
    d, R = _dist(c)
    rho = np.exp(-0.5 * (d / c["st"][0]) ** 2)
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
    """(c, nE, largest extras count of a cell) over the cells of `sel` that update"""
    live = [s for s in sel if s]
    core, union = frozenset.intersection(*live), frozenset.union(*live)
    return len(core), len(union) - len(core), max(len(s) - len(core) for s in live)


def _oracle(c, mp):
    from oracle import oracle as O
    ge = None if c["elevs"] is None else c["elevs"].ravel()
    og, op = O.Pts(c["lats"].ravel(), c["lons"].ravel(), ge), O.Pts(c["plat"], c["plon"], c["pelevs"])
    return O.oi(og, c["bg"].ravel(), op, c["obs"], c["ratios"], c["pbg"], O.Barnes(*c["st"]), mp).reshape(c["bg"].shape)


def _run(c, mp):
    """the call, and the same call under GPP_OI_NO_BULK_CERT: no item certified there, the same bits.  Returns the analysis and the statistics of
    the plain call."""
    import gridpp_amd as gridpp
    if c["elevs"] is None:
        grid, points = gridpp.Grid(c["lats"], c["lons"]), gridpp.Points(c["plat"], c["plon"])
    else:
        grid, points = gridpp.Grid(c["lats"], c["lons"], c["elevs"]), gridpp.Points(c["plat"], c["plon"], c["pelevs"])
    st = gridpp.BarnesStructure(*c["st"])
    assert OVERRIDE not in gridpp.active_overrides()
    out = np.asarray(gridpp.optimal_interpolation(grid, c["bg"], points, c["obs"], c["ratios"], c["pbg"], st, mp))
    s = gridpp.oi_last_stats()
    print(s)
    assert s["union_kernel_ms"] > 0, s
    gridpp.set_path_override(OVERRIDE, "1")
    try:
        assert OVERRIDE in gridpp.active_overrides()
        out0 = np.asarray(gridpp.optimal_interpolation(grid, c["bg"], points, c["obs"], c["ratios"], c["pbg"], st, mp))
        s0 = gridpp.oi_last_stats()
    finally:
        gridpp.set_path_override(OVERRIDE, None)
    print(s0)
    # (not the number of factorisations: a geometry whose tile was declined is remembered, and its second call may go to k_oi at once)
    assert s0["bulk_certified"] == 0 and s0["cells_updated"] == s["cells_updated"], (s, s0)
    assert np.array_equal(out, out0, equal_nan=True)
    return out, s


def _one_tile(s, certified):
    assert s["fallback_tiles"] == 0 and s["solves"] == 1 and s["bulk_certified"] == (1 if certified else 0), s


# ---- 1. certified, core only ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _core_case(mp):
    c = _tile_case(30, [], seed=1)
    d, R = _dist(c)
    assert d.max() < R - 1000.0                                   # every observation far inside the radius of every cell
    if mp >= 30:
        assert _union(_selections(c, mp)) == (30, 0, 0)
    return c, _oracle(c, mp)


@pytest.mark.parametrize("mp", [1, 5, 30, 32])
def test_certified_core_only(mp):
    """max_points 1 and 5: the bulk disc holds fewer records than the tile has (the rings take the rest); 30: exactly max_points; 32: all of them
    with cnt < max_points at the end"""
    c, ref = _core_case(mp)
    out, s = _run(c, mp)
    _one_tile(s, True)
    _check(out, ref)


# ---- 2. fewer observations than max_points --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _few_case():
    c = _tile_case(7, [], seed=2)
    assert _union(_selections(c, 30)) == (7, 0, 0)
    return c, _oracle(c, 30)


def test_fewer_observations_than_max_points():
    c, ref = _few_case()
    out, s = _run(c, 30)
    _one_tile(s, True)
    _check(out, ref)


# ---- 3. the radius straddled ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _straddle_case():
    c = _tile_case(10, _side(LEFT, [0, 1, 2]) + _side(RIGHT, [0, 1]), seed=3)
    assert c["plat"].size == 15                                   # S < max_points: the bulk disc holds every record
    d, R = _dist(c)
    rejected = (d > R).any(0)                                     # observations some cell rejects by the radius ...
    assert rejected.sum() == 5 and ((d <= R).any(0) & rejected).sum() == 5   # ... and some cell takes
    assert _union(_selections(c, 30)) == (10, 5, 3)
    return c, _oracle(c, 30)


def test_radius_straddled():
    c, ref = _straddle_case()
    out, s = _run(c, 30)
    _one_tile(s, False)
    _check(out, ref)


# ---- 4. the underflow bound ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _underflow_case():
    st = (100.0, 0.0, 0.0, 5000.0)                                # hmax = 50 h: the radius does not cut what underflows
    c = _tile_case(24, [], seed=4, rmin=1000.0, rmax=2000.0, st=st)
    d, R = _dist(c)
    assert R == np.inf                                            # (its min_rho exp(-1250) is 0: every pair is inside the radius)
    v = d / st[0]
    rho = np.exp(-0.5 * v * v).astype(np.float32)
    assert (rho == 0).any() and (rho > 0).any() and v.min() < 10.0 and v.max() > 20.0
    assert (rho > 0).any(1).all()                                 # every cell updates
    return c, _oracle(c, 30)


def test_underflow_bound():
    """observations 1 .. 2 km from the tile centre at h = 100 m: v runs from 5 to 25 over the cells, rho underflows to 0 for part of the pairs
    (the cells' selections differ by more than the shared factorisation holds: the tile is declined, its parts are not certified either)"""
    c, ref = _underflow_case()
    out, s = _run(c, 30)
    assert s["solves"] >= 1 and s["bulk_certified"] == 0, s
    _check(out, ref)


@functools.lru_cache(maxsize=None)
def _twelve_h_case(rmin, rmax):
    st = (100.0, 0.0, 0.0, 1400.0)                                # a FINITE radius of 14 h (the case above has an infinite one, which fails the
    c = _tile_case(24, [], seed=4, rmin=rmin, rmax=rmax, st=st)   #  certificate by itself): here the 12 h bound alone decides
    d, R = _dist(c)
    assert abs(R - 1400.0) < 0.01 and d.max() < R - 100.0
    rho = np.exp(-0.5 * (d / st[0]) ** 2).astype(np.float32)
    assert rho.min() > 1.2e-38                                    # no pair underflows, none is subnormal
    return c, _oracle(c, 30), d.max() / st[0]


def test_twelve_h_bound():
    """every pair inside R and inside near_r with room to spare; v reaches 12.9 in the first case (not certified: beyond 12 h) and 8.5 in the
    control (certified)"""
    c, ref, vmax = _twelve_h_case(650.0, 800.0)
    assert 12.5 < vmax < 13.0
    out, s = _run(c, 30)
    _one_tile(s, False)
    _check(out, ref)
    c, ref, vmax = _twelve_h_case(200.0, 400.0)
    assert vmax < 9.0
    out, s = _run(c, 30)
    _one_tile(s, True)
    _check(out, ref)


# ---- 5. inactive lanes ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nan_case():
    c = _tile_case(30, [], nan_cells=((0, 0), (3, 4), (7, 7), (6, 1), (2, 2)), seed=1)
    return c, _oracle(c, 30)


def test_inactive_lanes_nan_backgrounds():
    c, ref = _nan_case()
    assert np.isnan(ref).sum() == 5
    out, s = _run(c, 30)
    _one_tile(s, True)
    assert s["cells_updated"] == 59
    _check(out, ref)


@functools.lru_cache(maxsize=None)
def _partial_case():
    c = _tile_case(30, [], nan_cells=((10, 4), (0, 2)), seed=5, ny=5, nx=11)
    d, R = _dist(c)
    assert d.max() < R - 1000.0
    return c, _oracle(c, 30)


def test_inactive_lanes_partial_tiles():
    c, ref = _partial_case()
    out, s = _run(c, 30)
    assert s["fallback_tiles"] == 0 and s["solves"] >= 2 and s["bulk_certified"] == s["solves"] and s["cells_updated"] == 53, s
    _check(out, ref)


# ---- 6. the third axis ------------------------------------------------------------------------------------------------------------------------
LAT3, LON3 = 35.264, 45.0                                         # |x| = |y| = |z|


@functools.lru_cache(maxsize=None)
def _third_axis_case():
    """returns (the case with the mirrored clusters and the far points, the control without them, the oracle's analysis of both)"""
    ctl = _tile_case(20, [], seed=6, rmin=1000.0, rmax=2000.0, lat0=LAT3, lon0=LON3, shuffle=False)
    g = _xyz(ctl["lats"].ravel(), ctl["lons"].ravel())
    assert np.abs(np.abs(g) / RE - 1 / np.sqrt(3)).max() < 1e-3
    rng = np.random.default_rng(96)
    ctr = 0.5 * 7 * DX
    mlat, mlon = [], []
    for k in range(3):
        r, t = 400.0 * np.sqrt(rng.random(12)), 2 * np.pi * rng.random(12)
        la, lo = _latlon(ctr + r * np.cos(t), ctr + r * np.sin(t), LAT3, LON3)
        la, lo = ((la, 180.0 - lo), (la, -lo), (-la, lo))[k]      # (-x, y, z), (x, -y, z), (x, y, -z)
        mlat.append(la); mlon.append(lo)
    mlat, mlon = np.concatenate(mlat), np.concatenate(mlon)
    # each cluster, seen along the axis it was mirrored on, lies within 500 m of the tile centre -- and half the globe away on that axis
    gc, m = g.mean(0), _xyz(mlat, mlon)
    for k in range(3):
        mk, keep = m[12 * k:12 * k + 12], [a for a in range(3) if a != k]
        assert np.sqrt(((mk[:, keep] - gc[keep]) ** 2).sum(-1)).max() < 500.0
        assert np.abs(mk[:, k] + gc[k]).max() < 500.0
    flat, flon = np.array([90.0, -90.0, 0.0, 0.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.0, 90.0, 180.0, 270.0])
    n = mlat.size + flat.size
    c = dict(ctl)
    c["plat"], c["plon"] = np.concatenate([ctl["plat"], mlat, flat]), np.concatenate([ctl["plon"], mlon, flon])
    for k in ("obs", "pbg"):
        c[k] = np.concatenate([ctl[k], rng.normal(0, 1, n).astype(np.float32)])
    c["ratios"] = np.concatenate([ctl["ratios"], rng.uniform(0.1, 1, n).astype(np.float32)])
    d, R = _dist(c)
    assert d[:, :20].max() < R - 500.0 and d[:, 20:].min() > 1e6
    ref, ref_ctl = _oracle(c, 30), _oracle(ctl, 30)
    assert np.array_equal(ref, ref_ctl)                           # the mirrored clusters and the far points reach no cell
    return c, ctl, ref, ref_ctl


def test_third_axis():
    """whichever axis the bins drop, one mirrored cluster projects onto the tile, nearer in projection than the real observations: a certificate
    that looked at the projection alone would hand its twelve records (rho = 0) to every cell and evict real observations"""
    import gridpp_amd as gridpp
    c, ctl, ref, ref_ctl = _third_axis_case()
    out, s = _run(c, 30)
    _one_tile(s, False)
    _check(out, ref)
    out_ctl, s_ctl = _run(ctl, 30)
    _one_tile(s_ctl, True)
    _check(out_ctl, ref_ctl)
    assert gridpp.active_overrides() == []


# ---- 7. the gate: elevation factor -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gate_case():
    c = _tile_case(30, [], seed=1, st=(H, 200.0))
    rng = np.random.default_rng(97)
    c["elevs"], c["pelevs"] = rng.uniform(0, 300, c["bg"].shape).astype(np.float32), rng.uniform(0, 300, 30).astype(np.float32)
    return c, _oracle(c, 30)


def test_gate_elevation_factor():
    c, ref = _gate_case()
    out, s = _run(c, 30)
    assert s["solves"] >= 1 and s["bulk_certified"] == 0, s
    _check(out, ref)


# ---- 8. the wider forms -----------------------------------------------------------------------------------------------------------------------
WIDE = {40: 45, 50: 55}                                           # max_points -> observations


@functools.lru_cache(maxsize=None)
def _wide_case(mp):
    """max_points observations within 1 km of the centre and five more 2.5 km from it (at R - 1 145 m): every cell is at most 1 495 m from
    the former and at least 2 005 m from the latter, so all cells select the same max_points -- one tile, one factorisation without extras"""
    n = WIDE[mp]
    c = _tile_case(mp, [(72.0 * k + 10.0, -1145.0) for k in range(n - mp)], seed=mp, rmax=1000.0)
    d, R = _dist(c)
    assert c["plat"].size == n and d.max() < R - 500.0
    assert _union(_selections(c, mp)) == (mp, 0, 0)
    return c, _oracle(c, mp)


@pytest.mark.parametrize("mp", sorted(WIDE))
def test_wider_forms(mp):
    """48 register columns (max_points 40) and 64 (max_points 50)"""
    c, ref = _wide_case(mp)
    out, s = _run(c, mp)
    _one_tile(s, True)
    _check(out, ref)


# ---- 9. many tiles ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _many_case():
    rng = np.random.default_rng(99)
    n, S = 64, 300
    xs, ys = np.meshgrid(np.arange(n) * DX, np.arange(n) * DX)
    lats, lons = _latlon(xs, ys)
    ext = (n - 1) * DX
    plat, plon = _latlon(rng.uniform(-2000.0, ext + 2000.0, S), rng.uniform(-2000.0, ext + 2000.0, S))
    c = dict(lats=lats, lons=lons, plat=plat, plon=plon, bg=rng.normal(0, 1, (n, n)).astype(np.float32), obs=rng.normal(0, 1, S).astype(np.float32),
             pbg=rng.normal(0, 1, S).astype(np.float32), ratios=rng.uniform(0.1, 1, S).astype(np.float32), st=(H,), elevs=None, pelevs=None)
    return c, _oracle(c, 30)


def test_many_tiles():
    c, ref = _many_case()
    out, s = _run(c, 30)
    assert 0 < s["bulk_certified"] <= s["solves"], s
    _check(out, ref)
