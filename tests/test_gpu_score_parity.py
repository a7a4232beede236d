"""GPU: gridpp.neighbourhood_score and the vector gridpp.calc_score against the numpy restatement of tests/score_ref.py
(tests/test_score_restatement.py pins its calc_score to the reference's known answers; its neighbourhood_score is composed from
oracle.gridding_nearest and oracle.neighbourhood, which other tests pin).

Bit for bit (NaNs in the same places), no tolerance: the counts of a window are exact integers on both sides (the library counts
bytes, the oracle adds zeros and ones in a double summed-area table, exact far beyond any window here), and from the counts on both
sides do the same float and double operations in the same order -- (float)((double)n / area), then calc_score with the reference's
promotions; the library is built with -ffp-contract=off and correctly rounded division.

W x C is the tile of the fused kernel (GPP_SCORE_TILE_COLS columns of a strip, GPP_SCORE_TILE_ROWS rows of a chunk), MAXHW the largest
half width it takes (GPP_SCORE_FUSED_MAXHW): the shapes and half widths below sit on both sides of each.  Every case runs from numpy
arrays on the path the library picks, and again from a torch tensor under GPP_SCORE_GENERAL, the override that forces the general
path; the two runs must agree with each other as well.  The packing bound of the fused kernel ((2 hw + 1)^2 < 65536) lies far beyond
MAXHW, so a window with 65535 or more counted cells of one category exists only at a half width that takes the general path by the
library's own rule (hw > MAXHW): test_a_window_of_more_than_65535_counted_cells."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests import score_ref as R

pytestmark = pytest.mark.gpu

from gridpp_amd import _capi   # noqa: E402

W, CH, MAXHW = _capi.SCORE_TILE_COLS, _capi.SCORE_TILE_ROWS, _capi.SCORE_FUSED_MAXHW
YS = (1, CH - 1, CH, CH + 1, 2 * CH + 3)
XS = (1, W - 1, W, W + 1, 2 * W + 3)
HWS = (1, 2, MAXHW, MAXHW + 1, 2 * W + 2 * CH + 9)   # the last one is larger than both sides of every grid here
CASES = [(Y, X, obs, (iy + ix + io) % 2 == 0) for iy, Y in enumerate(YS) for ix, X in enumerate(XS) for io, obs in enumerate(R.OBS_SETS)]
LENGTHS = (0, 1, 63, 64, 65, 257, 100003)


@pytest.fixture(scope="module")
def gridpp():
    import gridpp_amd
    if gridpp_amd.device_count() == 0:
        pytest.fail("no HIP device visible")
    return gridpp_amd


@contextlib.contextmanager
def general_path():
    lib = _capi.lib()
    assert lib.gpp_set_path_override(b"GPP_SCORE_GENERAL", b"1") == _capi.GPP_OK
    try:
        buf = C.create_string_buffer(256)
        assert lib.gpp_active_overrides(buf, 256) >= 1 and b"GPP_SCORE_GENERAL" in buf.value
        yield
    finally:
        lib.gpp_set_path_override(b"GPP_SCORE_GENERAL", None)


def handles(gridpp, lats, lons, plat, plon, geodetic):
    from oracle import oracle as O
    ctype, otype = (gridpp.Geodetic, O.Geodetic) if geodetic else (gridpp.Cartesian, O.Cartesian)
    zy, zp = np.zeros_like(lats), np.zeros_like(plat)
    grid = gridpp.Grid(lats, lons, zy, zy, ctype)
    points = gridpp.Points(plat, plon, zp, zp, ctype)
    return grid, points, O.Pts(lats.ravel(), lons.ravel(), ctype=otype), O.Pts(plat, plon, ctype=otype)


def check_all(gridpp, grid, points, og, op, fcst, ref, half_widths, ref_grid=None):
    """every half width and every metric: numpy on the picked path, torch under GPP_SCORE_GENERAL, the restatement"""
    import torch
    dev = torch.from_numpy(fcst).cuda()
    if ref_grid is None:
        ref_grid = R.gridded(og, op, ref, fcst.shape)   # once for all half widths
    for hw in half_widths:
        a, b, c, d = R.hoods(og, op, fcst, ref, hw, R.THRESHOLD, ref_grid)
        for metric in R.METRICS:
            want = R.calc_score_table(a, b, c, d, metric)
            got = gridpp.neighbourhood_score(grid, points, fcst, ref, hw, metric, R.THRESHOLD)
            assert isinstance(got, np.ndarray) and got.dtype == np.float32
            R.same_bits(got, want)
            with general_path():
                general = gridpp.neighbourhood_score(grid, points, dev, ref, hw, metric, R.THRESHOLD)
            assert isinstance(general, torch.Tensor) and general.is_cuda and general.dtype == torch.float32
            general = general.cpu().numpy()
            R.same_bits(general, want)
            R.same_bits(general, got)
    assert gridpp.active_overrides() == []


@pytest.mark.parametrize("Y,X,obs,geodetic", CASES, ids=["%dx%d-%s-%s" % (c[0], c[1], c[2], "geo" if c[3] else "cart") for c in CASES])
def test_neighbourhood_score_parity(gridpp, Y, X, obs, geodetic):
    lats, lons, plat, plon, ref, fcst = R.case_inputs(Y, X, geodetic, obs, seed=1000 * Y + X)
    grid, points, og, op = handles(gridpp, lats, lons, plat, plon, geodetic)
    check_all(gridpp, grid, points, og, op, fcst, ref, HWS)


def test_the_cases_cover_what_they_should():
    assert len(CASES) == 225 and {c[2] for c in CASES} == set(R.OBS_SETS)
    for obs in R.OBS_SETS:
        assert {c[3] for c in CASES if c[2] == obs} == {True, False}
    assert HWS[-1] > max(YS) and HWS[-1] > max(XS) and HWS[2] == MAXHW and HWS[3] == MAXHW + 1
    # contents: what the names promise
    _, _, _, _, ref, fcst = R.case_inputs(33, 65, True, "sprinkled", 1)
    assert np.isnan(ref).any() and np.isposinf(ref).any() and np.isneginf(ref).any()
    assert np.isnan(fcst).any() and np.isposinf(fcst).any() and np.isneginf(fcst).any()
    _, _, _, _, ref, fcst = R.case_inputs(33, 65, True, "at_threshold", 1)
    assert (ref == np.float32(R.THRESHOLD)).any() and (fcst == np.float32(R.THRESHOLD)).any()
    _, _, _, _, ref, fcst = R.case_inputs(33, 65, True, "above", 1)
    assert ref.min() > R.THRESHOLD and fcst.min() > R.THRESHOLD
    _, _, _, _, ref, fcst = R.case_inputs(33, 65, True, "below", 1)
    assert ref.max() < R.THRESHOLD and fcst.max() < R.THRESHOLD
    assert R.case_inputs(33, 65, True, "none", 1)[4].size == 0 and R.case_inputs(33, 65, True, "one", 1)[4].size == 1


def test_several_observations_per_cell_straddle_the_threshold(gridpp):
    """the gridded means fall on both sides of the threshold, so a cell's category hangs on the mean's last bits"""
    from oracle import oracle as O
    lats, lons, plat, plon, ref, fcst = R.case_inputs(33, 65, False, "several", seed=5)
    og, op = O.Pts(lats.ravel(), lons.ravel(), ctype=O.Cartesian), O.Pts(plat, plon, ctype=O.Cartesian)
    g = O.gridding_nearest(og, op, ref, 1, R.Mean)
    assert (g > R.THRESHOLD).sum() > 100 and (g <= R.THRESHOLD).sum() > 100


def test_a_window_of_more_than_65535_counted_cells(gridpp):
    """260 x 260 cells, all of category a, half width 130: the windows around the centre hold all 67 600 cells, more than a 16-bit lane
    of the fused kernel could count; hw > MAXHW takes the general path, whose counters are 32 bits wide.  One observation per cell, 180 m
    from its node on the 1 km grid: the gridded reference is known without the oracle's linear scan over 67 600 x 67 600 pairs."""
    Y = X = 260
    lats, lons = R.geometry(Y, X, False)
    plat, plon = (lats + np.float32(100)).ravel(), (lons - np.float32(150)).ravel()
    ref, fcst = np.full(Y * X, 2, np.float32), np.full((Y, X), 3, np.float32)
    fcst[0, :7] = 0          # a few c cells, so that the scores are not all trivial
    grid, points, og, op = handles(gridpp, lats, lons, plat, plon, False)
    ref_grid = ref.reshape(Y, X)
    a = R.hoods(og, op, fcst, ref, 130, R.THRESHOLD, ref_grid)[0]
    assert a[130, 130] * np.float32(Y * X) >= 65535
    assert 130 > MAXHW
    check_all(gridpp, grid, points, og, op, fcst, ref, (130,), ref_grid)


def test_float64_forecast_is_rounded_like_the_typemap(gridpp):
    lats, lons, plat, plon, ref, fcst = R.case_inputs(33, 65, True, "tenth", seed=9)
    grid, points, og, op = handles(gridpp, lats, lons, plat, plon, True)
    wide = fcst.astype(np.float64) + 1e-12          # rounds back to fcst
    assert np.array_equal(wide.astype(np.float32), fcst)
    want = R.neighbourhood_score(og, op, fcst, ref, 3, R.Ets, R.THRESHOLD)
    R.same_bits(gridpp.neighbourhood_score(grid, points, wide, ref, 3, gridpp.Ets, R.THRESHOLD), want)


def vectors(n, seed, nans):
    rng = np.random.default_rng(seed)
    ref, fcst = rng.random(n).astype(np.float32), rng.random(n).astype(np.float32)
    if nans and n:
        ref[rng.random(n) < 0.2] = np.nan
        fcst[rng.random(n) < 0.2] = np.nan
        ref[rng.random(n) < 0.05] = np.inf
        fcst[rng.random(n) < 0.05] = -np.inf
    return ref, fcst


@pytest.mark.parametrize("nans", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("n", LENGTHS)
def test_vector_calc_score(gridpp, n, nans):
    import torch
    ref, fcst = vectors(n, 7 + n, nans)
    if nans and n >= 63:
        assert np.isnan(ref).any() and np.isnan(fcst).any() and (np.isnan(ref) & ~np.isnan(fcst)).any() and (~np.isnan(ref) & np.isnan(fcst)).any()
    dref, dfcst = torch.from_numpy(ref).cuda(), torch.from_numpy(fcst).cuda()
    for metric in R.METRICS:
        want = R.calc_score_vec(ref, fcst, 0.4, 0.4, metric)
        for r, f in ((ref, fcst), (dref, dfcst), (list(ref), list(fcst))) if n <= 257 else ((ref, fcst), (dref, dfcst)):
            got = gridpp.calc_score(r, f, 0.4, metric)
            assert isinstance(got, float)
            R.same_bits(np.float32(got), want)
            R.same_bits(np.float32(gridpp.calc_score(r, f, 0.4, 0.4, metric)), want)
        want = R.calc_score_vec(ref, fcst, 0.4, 0.6, metric)
        R.same_bits(np.float32(gridpp.calc_score(ref, fcst, 0.4, 0.6, metric)), want)
        R.same_bits(np.float32(gridpp.calc_score(dref, dfcst, 0.4, 0.6, metric)), want)
    if n > 1:   # a longer ref: the first len(fcst) elements count
        R.same_bits(np.float32(gridpp.calc_score(ref, fcst[:n - 1], 0.4, gridpp.Ets)), R.calc_score_vec(ref[:n - 1], fcst[:n - 1], 0.4, 0.4, R.Ets))


def test_known_answers_of_the_reference(gridpp):
    k = R.KNOWN
    for name, row in k["expected"].items():
        for t, threshold in enumerate(k["thresholds"]):
            got = gridpp.calc_score(k["obs"], k["fcst"], threshold, getattr(gridpp, name))
            np.testing.assert_almost_equal(got, np.nan if row[t] is None else row[t], R.GOLDEN["decimals"])


def test_counts_saturate_at_two_to_the_24(gridpp):
    """2^24 + 3 elements, all in category a: the reference's `float a++` stops at 16777216, and Pc and Ts come from that a.  Three counts
    in 2^24 do not move a score by a float's last bit, so a second table shows the clamp in the value: 2^24 + 2^20 a elements and 2^24 c
    elements give Ts = 2^24 / (2^24 + 2^24) = 0.5 exactly, where the unclamped counts would give 0.515."""
    import torch
    n = (1 << 24) + 3
    m, c = (1 << 24) + (1 << 20), 1 << 24
    ref = torch.ones(m + c, device="cuda")
    fcst = torch.ones(m + c, device="cuda")
    for metric in (R.Pc, R.Ts):
        R.same_bits(np.float32(gridpp.calc_score(ref[:n], fcst[:n], 0.5, metric)), R.score_of_counts((n, 0, 0, 0), metric))
        assert gridpp.calc_score(ref[:n], fcst[:n], 0.5, metric) == 1
    fcst[m:] = 0
    for metric in R.METRICS:
        R.same_bits(np.float32(gridpp.calc_score(ref, fcst, 0.5, metric)), R.score_of_counts((m, 0, c, 0), metric))
    assert gridpp.calc_score(ref, fcst, 0.5, R.Ts) == 0.5
    assert gridpp.calc_score(ref, fcst, 0.5, 0.5, R.Pc) == 0.5
