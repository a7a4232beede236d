"""The per-tile bookkeeping of k_oi_union's first pass (csrc/oi_union.h, round 7) against the CPU oracle, at the places where it can go wrong:

A  the extent of a tile and what hangs on it (the square of phase 1, the wave-level prune, the row gaps of phase 2): partial tiles, tiles
   with few or no valid cells, the extreme tile shapes, 1-D point sets, every pair of bin axes, the skip flags of a remembered list,
   the three kernel forms;
B  the per-lane mask of the slots a cell holds instead of reading the slots back from LDS: slots >= 32, equal-rho evictions, slot
   recycling when all are allocated, the 48- and 64-column forms;
C  phase 2, when the square of phase 1 covers its reach and when it does not.

Tolerances and tie-break as tests/test_gpu_oi_parity.py (RTOL 1e-5 over a floor of 1e-3); "same bits" is np.array_equal."""
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


def _oracle(lats, lons, plat, plon, bg, obs, ratios, pbg, h, mp, ge=None, gl=None, pe=None, pl=None, v=0, w=0):
    from oracle import oracle as O
    og = O.Pts(np.ravel(lats), np.ravel(lons), None if ge is None else np.ravel(ge), None if gl is None else np.ravel(gl))
    op = O.Pts(plat, plon, pe, pl)
    return O.oi(og, bg.ravel(), op, obs, ratios, pbg, O.Barnes(h, v, w), mp).reshape(bg.shape)


def _grid_case(seed, Y, X, S, lat=(0.0, 1.0), lon=(0.0, 1.0), obs_lat=None, obs_lon=None):
    rng = np.random.default_rng(seed)
    lats, lons = np.meshgrid(np.linspace(lat[0], lat[1], Y), np.linspace(lon[0], lon[1], X), indexing="ij")
    ol, oo = obs_lat or lat, obs_lon or lon
    plat, plon = ol[0] + (ol[1] - ol[0]) * rng.random(S), oo[0] + (oo[1] - oo[0]) * rng.random(S)
    bg, obs, pbg, ratios = _fields(rng, (Y, X), S)
    return lats, lons, plat, plon, bg, obs, ratios, pbg


def _run(case, h, mp, grid=None):
    import gridpp_amd as gridpp
    lats, lons, plat, plon, bg, obs, ratios, pbg = case
    grid = grid or gridpp.Grid(lats, lons)
    out = np.asarray(gridpp.optimal_interpolation(grid, bg, gridpp.Points(plat, plon), obs, ratios, pbg, gridpp.BarnesStructure(h), mp))
    return out, gridpp.oi_last_stats()


# ---- A: tile extents --------------------------------------------------------------------------------------------------------------
def test_a_a_partial_tiles():
    """37 x 53: 8 x 8 tiles, partial ones on both edges; 35 tiles, so the last workgroup holds one.  A second call on the same handle gives
    the same bits."""
    import gridpp_amd as gridpp
    case = _grid_case(7101, 37, 53, 400)
    grid = gridpp.Grid(case[0], case[1])
    out, s = _run(case, 10000, 30, grid)
    print(s)
    assert s["union_kernel_ms"] > 0
    _check(out, _oracle(*case, 10000, 30))
    out2, s2 = _run(case, 10000, 30, grid)
    assert np.array_equal(out, out2, equal_nan=True)


def test_a_b_tiles_with_few_or_no_valid_cells():
    """20 % NaN backgrounds, one tile without a valid cell and one with a single one (its extent is a point)."""
    case = list(_grid_case(7102, 37, 53, 400))
    rng = np.random.default_rng(1)
    bg = case[4]
    bg[rng.random(bg.shape) < 0.2] = np.nan
    bg[0:8, 0:8] = np.nan                          # tile (0, 0): nothing to do
    keep = bg[19, 42] if np.isfinite(bg[19, 42]) else np.float32(0.25)
    bg[16:24, 40:48] = np.nan
    bg[19, 42] = keep                              # tile (2, 5): one cell
    out, s = _run(case, 10000, 30)
    print(s)
    assert s["union_kernel_ms"] > 0
    _check(out, _oracle(*case, 10000, 30))


@pytest.mark.parametrize("shape,dlat", [((3, 200), 1.0), ((3, 200), 0.24), ((200, 3), 1.0)], ids=["1x64", "2x32", "64x1"])
def test_a_c_extreme_tile_shapes(shape, dlat):
    """Strongly anisotropic grids (gpp_tile_wshift): three rows 0.5 degrees apart over 200 columns take tiles of 1 x 64 cells, three rows
    0.12 degrees apart (24 column steps) tiles of 2 x 32, three columns under 200 rows tiles of 64 x 1."""
    Y, X = shape
    case = _grid_case(7103 + Y, Y, X, 300, lat=(0.0, dlat), obs_lat=(-0.1, dlat + 0.1), obs_lon=(-0.1, 1.1))
    out, s = _run(case, 10000, 30)
    print(s)
    assert s["union_kernel_ms"] > 0
    _check(out, _oracle(*case, 10000, 30))


def test_a_d_point_set_of_130_points():
    """A 1-D background (Points): runs of 64 consecutive points -- two full runs and one of two points."""
    import gridpp_amd as gridpp
    rng = np.random.default_rng(7104)
    t = np.linspace(0, 1, 130)
    blat, blon = 0.2 + 0.6 * t, 0.5 + 0.3 * np.sin(3 * t)      # (a curve: consecutive points are neighbours)
    S = 300
    plat, plon = rng.random(S), rng.random(S)
    bg, obs, pbg, ratios = _fields(rng, (130,), S)
    out = gridpp.optimal_interpolation(gridpp.Points(blat, blon), bg, gridpp.Points(plat, plon), obs, ratios, pbg, gridpp.BarnesStructure(10000), 30)
    s = gridpp.oi_last_stats()
    print(s)
    assert s["union_kernel_ms"] > 0
    _check(out, _oracle(blat, blon, plat, plon, bg, obs, ratios, pbg, 10000, 30))
    for mp in (40, 55):      # the 48- and 64-column forms on the same run tiling
        out = gridpp.optimal_interpolation(gridpp.Points(blat, blon), bg, gridpp.Points(plat, plon), obs, ratios, pbg, gridpp.BarnesStructure(20000), mp)
        _check(out, _oracle(blat, blon, plat, plon, bg, obs, ratios, pbg, 20000, mp))


def test_a_e_every_pair_of_bin_axes():
    """The extent of a tile is taken along the two axes the observation index is binned on.  Geodetic grids
    around (lat 0, lon 0): x is flat, bins on (y, z); (lat 0, lon 90): y is flat, (x, z); lat 85: z is flat, (x, y)."""
    import gridpp_amd as gridpp
    seen = set()
    for k, (la, lo) in enumerate([(0.0, 0.0), (0.0, 90.0), (85.0, 10.0)]):
        span_lon = 0.5 / max(np.cos(np.radians(la)), 0.05)
        case = _grid_case(7105 + k, 24, 24, 200, lat=(la - 0.25, la + 0.25), lon=(lo - span_lon / 2, lo + span_lon / 2))
        out, s = _run(case, 10000, 30)
        assert s["union_kernel_ms"] > 0
        _check(out, _oracle(*case, 10000, 30))
        axes = gridpp.obs_index_axes(gridpp.Points(case[2], case[3]))
        print((la, lo), axes, s)
        seen.add(axes)
    assert len(seen) >= 2, seen


def test_a_f_one_handle_from_call_to_call_and_across_the_kernel_forms():
    """The third call on a handle runs with the remembered list of declined tiles and with the skip flags in play (smooth terrain above,
    rough terrain below: the rough tiles are declined): the same bits as the first call.  Then the same Grid handle at max_points 40: the 48-column form."""
    import gridpp_amd as gridpp
    rng = np.random.default_rng(7106)
    Y, X, S = 120, 80, 120
    lats, lons = np.meshgrid(np.linspace(60, 60.5, Y), np.linspace(10, 10 + 2 / 3.0, X), indexing="ij")
    ge, gl = rng.uniform(0, 1000, (Y, X)).astype(np.float32), rng.uniform(0, 1, (Y, X)).astype(np.float32)
    ge[:96] = 100.0; gl[:96] = 0.5
    plat, plon = 60 + 0.5 * rng.random(S), 10 + 2 / 3.0 * rng.random(S)
    pe, pl = rng.uniform(0, 1000, S).astype(np.float32), rng.uniform(0, 1, S).astype(np.float32)
    pe[plat < 60.4] = 100.0; pl[plat < 60.4] = 0.5
    bg, obs, pbg, ratios = _fields(rng, (Y, X), S)
    grid, points, st = gridpp.Grid(lats, lons, ge, gl), gridpp.Points(plat, plon, pe, pl), gridpp.BarnesStructure(8000.0, 200.0, 0.5)
    outs, stats = [], []
    for _ in range(3):
        outs.append(np.asarray(gridpp.optimal_interpolation(grid, bg, points, obs, ratios, pbg, st, 30)))
        stats.append(gridpp.oi_last_stats())
    print(stats)
    assert stats[0]["union_kernel_ms"] > 0 and stats[0]["fallback_tiles"] > 0      # (there IS a list to remember)
    assert np.array_equal(outs[0], outs[2], equal_nan=True) and np.array_equal(outs[0], outs[1], equal_nan=True)
    _check(outs[0], _oracle(lats, lons, plat, plon, bg, obs, ratios, pbg, 8000.0, 30, ge, gl, pe, pl, 200.0, 0.5))
    out40 = gridpp.optimal_interpolation(grid, bg, points, obs, ratios, pbg, st, 40)
    _check(out40, _oracle(lats, lons, plat, plon, bg, obs, ratios, pbg, 8000.0, 40, ge, gl, pe, pl, 200.0, 0.5))


# ---- B: slot ownership ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [0.01, 0.02, 0.025])
def test_b_a_unions_beyond_32_slots(span):
    """16 x 16 cells inside 2 000 clustered observations.  The union of a tile grows with the tile's size against the distance of the
    30th nearest observation (0.07 of the domain for 2 000 of them).  Measured with a GPP_UNION_STATS build: insertions behind the bulk
    disc 2.8, 7.2 and 27 per tile for the three sizes -- on top of the ~30 slots of the bulk disc, i.e. slots 32 .. 39, the high half of
    the mask, are live in the scan and the classification; at 0.025 three of the four tiles end with more than 12 extras and are declined."""
    rng = np.random.default_rng(7110)
    S = 2000
    centres = rng.random((20, 2))
    which = rng.integers(0, 20, S)
    plat = np.clip(centres[which, 0] + rng.normal(0, 0.08, S), 0, 1)
    plon = np.clip(centres[which, 1] + rng.normal(0, 0.08, S), 0, 1)
    lats, lons = np.meshgrid(np.linspace(0.5, 0.5 + span, 16), np.linspace(0.5, 0.5 + span, 16), indexing="ij")
    bg, obs, pbg, ratios = _fields(rng, (16, 16), S)
    case = (lats, lons, plat, plon, bg, obs, ratios, pbg)
    out, s = _run(case, 10000, 30)
    print(span, s)
    _check(out, _oracle(*case, 10000, 30))


def test_b_b_equal_rho_evictions():
    """Every observation position three times: the worst kept rho of a cell is shared by several slots, and the eviction goes by the
    observation index (the `multi` path of run_chunk and end_bulk)."""
    rng = np.random.default_rng(7111)
    ulat, ulon = rng.random(120), rng.random(120)
    plat, plon = np.tile(ulat, 3), np.tile(ulon, 3)
    lats, lons = np.meshgrid(np.linspace(0, 1, 32), np.linspace(0, 1, 32), indexing="ij")
    bg, obs, pbg, ratios = _fields(rng, (32, 32), 360)
    case = (lats, lons, plat, plon, bg, obs, ratios, pbg)
    for mp in (20, 7):     # (7: the cut falls inside a triple)
        out, s = _run(case, 15000, mp)
        print(mp, s)
        _check(out, _oracle(*case, 15000, mp))


def test_b_c_all_slots_allocated():
    """The cell spacing of B-a's largest grid on 32 x 32 cells (16 tiles) inside the same clustered observations: the scan of a tile wants
    ~57 candidates in all (GPP_UNION_STATS build: 27 insertions per tile behind a bulk disc of ~30), more than the 40 slots -- `alloc ==
    FULL` recycles the slots no cell holds any more (live_mask: the wave-OR of the masks).  Some tiles fit after that, some are declined."""
    rng = np.random.default_rng(7110)
    S = 2000
    centres = rng.random((20, 2))
    which = rng.integers(0, 20, S)
    plat = np.clip(centres[which, 0] + rng.normal(0, 0.08, S), 0, 1)
    plon = np.clip(centres[which, 1] + rng.normal(0, 0.08, S), 0, 1)
    hi = 0.5 + 0.025 * 31 / 15
    lats, lons = np.meshgrid(np.linspace(0.5, hi, 32), np.linspace(0.5, hi, 32), indexing="ij")
    bg, obs, pbg, ratios = _fields(rng, (32, 32), S)
    case = (lats, lons, plat, plon, bg, obs, ratios, pbg)
    out, s = _run(case, 10000, 30)
    print(s)
    ntiles = 16
    # (measured on an MI355X with seed 7110: 9 of the 16 tiles declined, 7 kept, 151 factorisations)
    assert s["union_kernel_ms"] > 0 and 0 < s["fallback_tiles"] < ntiles, s
    _check(out, _oracle(*case, 10000, 30))


@pytest.mark.parametrize("mp", [40, 55])
def test_b_d_48_and_64_column_forms(mp):
    """WCAP 56 and 64: the same mask, 64 bits wide; every observation is in range of every cell of the 24 x 24 grid."""
    case = _grid_case(7113 + mp, 24, 24, 150)
    out, s = _run(case, 40000, mp)
    print(s)
    _check(out, _oracle(*case, 40000, mp))


# ---- C: phase 2 -------------------------------------------------------------------------------------------------------------------
def test_c_phase_two_loads_records_when_phase_one_cannot_cover_the_reach():
    """Fifty observations and a length scale longer than the domain: fewer than max_points observations in the square of phase 1, the
    thresholds stay at the localization radius, phase 2 has to fetch the rest."""
    case = _grid_case(7120, 64, 64, 50)
    out, s = _run(case, 60000, 30)
    print(s)
    _check(out, _oracle(*case, 60000, 30))


def test_c_phase_two_is_left_when_phase_one_covered_the_reach():
    """Dense observations: the 30th nearest lies well inside the square of phase 1."""
    case = _grid_case(7121, 64, 64, 2000)
    out, s = _run(case, 10000, 30)
    print(s)
    _check(out, _oracle(*case, 10000, 30))
