"""GPU: get_optimal_threshold and metric_optimizer_curve (gridpp_amd/csrc/metric_optimizer.hip) against the brute-force restatement
tests/metric_optimizer_ref.py, bit for bit with NaN matching NaN -- all six metrics at n = 1 .. 1025 and thresholds 0.5, 2 and 4 on
continuous and on heavily tied forecasts; the same under GPP_MO_TILE at one tile - 1, one tile, one tile + 1 and three tiles + 1, so that
the carry of the counts, the key behind a workgroup's last element and a run of equal scores all cross workgroups, and at two full default
tiles + 1; the defined corners (two runs with the best score, a best run at either end, one plateau, adjacent floats, NaN and infinities,
a threshold above every ref); the invariant that ties the result to calc_score; the curve at T around the group size and beyond one batch;
tensors, views and float64; and repeated calls around release_workspaces()."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

from tests import metric_optimizer_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
SMALL_TILES = (8, 300)   # 8: one element per lane, eight lanes at work; 300: two per lane, the last lane of a tile half full


@pytest.fixture(scope="module")
def amd():
    import gridpp_amd
    assert gridpp_amd.device_count() > 0
    return gridpp_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@contextlib.contextmanager
def tile(amd, items):
    amd.set_path_override("GPP_MO_TILE", str(items))
    try:
        assert "GPP_MO_TILE" in amd.active_overrides()
        yield
    finally:
        amd.set_path_override("GPP_MO_TILE", None)


@functools.lru_cache(maxsize=None)
def data(n, halves):
    ref, fcst = R.case(n, halves, 7000 + 2 * n + halves)
    ref.setflags(write=False)
    fcst.setflags(write=False)
    return ref, fcst


@functools.lru_cache(maxsize=None)
def expected(n, halves, threshold, metric):
    ref, fcst = data(n, halves)
    return R.get_optimal_threshold(ref, fcst, threshold, metric)


def sweep(amd, sizes):
    """every case of `sizes` through the library -> (got, want), one value per (n, halves, threshold)"""
    out = {}
    for metric in R.METRICS:
        got, want = [], []
        for n in sizes:
            for halves in (False, True):
                ref, fcst = data(n, halves)
                for t in R.THRESHOLDS:
                    got.append(amd.get_optimal_threshold(ref, fcst, t, metric))
                    want.append(expected(n, halves, t, metric))
        out[metric] = (np.array(got, F), np.array(want, F))
    return out


# ---- equality with the restatement --------------------------------------------------------------------------------------------------------
def test_every_metric_and_size(amd):
    assert not amd.active_overrides()
    for metric, (got, want) in sweep(amd, R.SIZES).items():
        print("metric %d: %d values, %d NaN expected" % (metric, want.size, np.isnan(want).sum()))
        R.same_bits(got, want)


def test_the_cases_are_not_mostly_nan():
    """on the sizes from 63 up at most a tenth of the expected values may be NaN: else the test above would compare NaN with NaN"""
    for metric in R.METRICS:
        want = np.array([expected(n, h, t, metric) for n in R.SIZES if n >= 63 for h in (False, True) for t in R.THRESHOLDS], F)
        print("metric %d: %d NaN of %d" % (metric, np.isnan(want).sum(), want.size))
        assert np.isnan(want).sum() <= 0.1 * want.size, metric


@pytest.mark.parametrize("items", SMALL_TILES)
def test_small_tiles_cross_workgroups(amd, items):
    sizes = (items - 1, items, items + 1, 3 * items + 1)
    with tile(amd, items):
        for metric, (got, want) in sweep(amd, sizes).items():
            R.same_bits(got, want)
    assert not amd.active_overrides()
    for n in sizes:   # and the same values with the default tile: the result does not depend on the override
        ref, fcst = data(n, True)
        R.same_bits(amd.get_optimal_threshold(ref, fcst, 2.0, amd.Ets), expected(n, True, 2.0, R.Ets))


def test_one_element_per_workgroup(amd):
    with tile(amd, 1):
        for metric in R.METRICS:
            for halves in (False, True):
                ref, fcst = data(65, halves)
                R.same_bits([amd.get_optimal_threshold(ref, fcst, t, metric) for t in R.THRESHOLDS], [expected(65, halves, t, metric) for t in R.THRESHOLDS])


def test_two_default_tiles_and_one_element(amd):
    from gridpp_amd import _capi
    n = 2 * _capi.MO_TILE_ITEMS + 1
    for metric in (R.Ets, R.Bias):
        for halves in (False, True):
            ref, fcst = data(n, halves)
            want = expected(n, halves, 2.0, metric)
            assert halves or np.isfinite(want)
            R.same_bits(amd.get_optimal_threshold(ref, fcst, 2.0, metric), want)


# ---- defined corners ------------------------------------------------------------------------------------------------------------------------
# ref against the threshold 0.5 in the order of fcst: 0 0 1 1 0 0 1 1.  Pc at the plateaus = 5 6 5 4 5 6 5 4 eighths: two separated best runs.
TWO_RUNS = np.array([0, 0, 1, 1, 0, 0, 1, 1], F)


def both(amd, ref, fcst, threshold, metric):
    got, want = amd.get_optimal_threshold(ref, fcst, threshold, metric), R.get_optimal_threshold(ref, fcst, threshold, metric)
    R.same_bits(got, want)
    return got


def test_the_lower_of_two_best_runs_wins(amd):
    fcst = np.arange(1, 9, dtype=F)
    assert both(amd, TWO_RUNS, fcst, 0.5, amd.Pc) == 2.5
    order = np.array([5, 2, 7, 0, 3, 6, 1, 4])   # the same pairs unsorted
    assert both(amd, TWO_RUNS[order], fcst[order], 0.5, amd.Pc) == 2.5
    # a best run of two plateaus with equal scores (a NaN ref between them changes no count), then a lower one, then the best again
    ref = np.array([0, 0, np.nan, 1, 1, 0, 0, 1, 1], F)
    assert both(amd, ref, np.arange(1, 10, dtype=F), 0.5, amd.Pc) == 3.0   # [2, 4)
    with tile(amd, 1):
        assert both(amd, ref, np.arange(1, 10, dtype=F), 0.5, amd.Pc) == 3.0
        assert both(amd, TWO_RUNS, fcst, 0.5, amd.Pc) == 2.5


def test_a_best_run_at_either_end_is_filtered(amd):
    assert np.isnan(both(amd, [0, 1, 1, 1], [1, 2, 3, 4], 0.5, amd.Pc))      # Pc = 4 2 1 0 quarters: the best is s(u_0)
    assert np.isnan(both(amd, [0, 0, 0, 0], [1, 2, 3, 4], 0.5, amd.Pc))      # Pc = 1 2 3 4 quarters: the best is s(u_m-1)
    assert both(amd, [0, 0, 0, 1], [1, 2, 3, 4], 0.5, amd.Pc) == 3.5         # Pc = 2 3 4 3 quarters


def test_one_plateau(amd):
    for metric in R.METRICS:
        assert np.isnan(both(amd, [0, 3, 3], [2, 2, 2], 1.5, metric))
        assert np.isnan(both(amd, [3], [2], 1.5, metric))


def test_adjacent_floats(amd):
    one = F(1)
    up1 = np.nextafter(one, F(2))
    up2 = np.nextafter(up1, F(2))
    tail = [3, 4, 5, 6, 7]
    # lo = 1, hi = the next float: the midpoint is a tie and rounds to the even mantissa, 1
    assert both(amd, TWO_RUNS, np.array([0.5, one, up1] + tail, F), 0.5, amd.Pc) == one
    # lo = the float after 1 (odd mantissa), hi = the next: the tie rounds up to hi, and the rule gives lo
    got = both(amd, TWO_RUNS, np.array([one, up1, up2] + tail, F), 0.5, amd.Pc)
    assert got == up1 and got != up2


def test_nan_and_infinities(amd):
    rng = np.random.default_rng(99)
    n = 200
    ref, fcst = (a.copy() for a in R.case(n, False, 4242))
    ref[rng.random(n) < 0.1] = np.nan
    u = rng.random(n)
    fcst[u < 0.08] = np.nan
    fcst[(u >= 0.08) & (u < 0.16)] = np.inf
    fcst[(u >= 0.16) & (u < 0.24)] = -np.inf
    fcst[(u >= 0.24) & (u < 0.27)] = -0.0
    fcst[(u >= 0.27) & (u < 0.30)] = 0.0
    ref[5], fcst[5] = np.inf, -1.0
    ref[6], fcst[6] = -np.inf, 1.0
    valid = 0
    for items in (2048, 16):
        with tile(amd, items):
            for metric in R.METRICS:
                for t in R.THRESHOLDS:
                    valid += np.isfinite(both(amd, ref, fcst, t, metric))
    assert valid >= 18
    for metric in R.METRICS:   # nothing finite in fcst: no plateau
        assert np.isnan(both(amd, [1, 2, 3, 4], [np.nan, np.inf, -np.inf, np.nan], 1.5, metric))
    # the signs of zero are one plateau, and it is +0
    got = both(amd, [0, 0, 0, 0, 1, 1], [-1, -0.0, 0.0, -0.0, 1, 2], 0.5, amd.Pc)
    assert got == 0.5 and not np.signbit(got)                                # Pc = 3 6 5 4 sixths at -1, 0, 1, 2: [0, 1)


def test_a_threshold_above_every_ref(amd):
    ref, fcst = data(257, False)
    for metric in R.METRICS:
        assert np.isnan(both(amd, ref, fcst, 1000.0, metric))
        both(amd, ref, fcst, float(ref.max()), metric)
        both(amd, ref, fcst, np.nan, metric)


# ---- the invariant ------------------------------------------------------------------------------------------------------------------------------
def test_the_result_attains_the_largest_score_of_calc_score(amd):
    """for every valid result x: calc_score(ref, fcst, t, x, metric) = the largest valid calc_score(ref, fcst, t, u_k, metric) -- both
    sides through k_score_counts, nothing of the restatement"""
    checked = 0
    for n in (63, 64, 65, 255):
        for halves in (False, True):
            ref, fcst = data(n, halves)
            for metric in R.METRICS:
                for t in R.THRESHOLDS:
                    x = amd.get_optimal_threshold(ref, fcst, t, metric)
                    if not np.isfinite(x):
                        continue
                    scores = np.array([amd.calc_score(ref, fcst, t, float(u), metric) for u in R.plateaus(fcst)], F)
                    assert F(amd.calc_score(ref, fcst, t, x, metric)) == scores[np.isfinite(scores)].max(), (n, halves, metric, t)
                    checked += 1
    print("%d valid results checked" % checked)
    assert checked == 144   # every one of these cases has a valid result (tests/metric_optimizer_ref.py on the same data)


# ---- the curve ----------------------------------------------------------------------------------------------------------------------------------
def test_curve_sizes_order_and_dropped_thresholds(amd):
    from gridpp_amd import _capi
    G = _capi.MO_GROUP
    ref, fcst = data(257, False)
    pool = np.array([2.0, 1000.0, 0.5, 4.0, np.nan, 1.0, 3.0, -5.0, 2.5, 0.25], F)   # 1000, NaN and -5 give no valid result
    for T in (1, G - 1, G, G + 1, 2 * G + 1, 70):   # 70: more than one batch of launches
        thresholds = np.resize(pool, T)
        for metric in (amd.Ets, amd.Bias, amd.Pc):
            curve_ref, curve_fcst = amd.metric_optimizer_curve(ref, fcst, thresholds, metric)
            single = np.array([amd.get_optimal_threshold(ref, fcst, t, metric) for t in thresholds], F)
            keep = np.isfinite(single)
            assert T < 5 or (keep.any() and not keep.all())
            R.same_bits(curve_ref, single[keep])
            R.same_bits(curve_fcst, thresholds[keep])
            assert curve_ref.dtype == F and curve_fcst.dtype == F
    want = R.metric_optimizer_curve(ref, fcst, pool, R.Ets)
    got = amd.metric_optimizer_curve(ref, fcst, pool, amd.Ets)
    R.same_bits(got[0], want[0])
    R.same_bits(got[1], want[1])
    with tile(amd, 8):
        got = amd.metric_optimizer_curve(ref, fcst, pool, amd.Ets)
        R.same_bits(got[0], want[0])
        R.same_bits(got[1], want[1])


def test_curve_quadratic_case_of_the_reference(amd):
    """tests/test_metric_optimizer.py of the reference: curve_ref within 1.5 of curve_fcst squared"""
    obs = np.linspace(0, 10, 101)
    for metric in (amd.Pc, amd.Bias):
        curve_ref, curve_fcst = amd.metric_optimizer_curve(obs, obs ** 2, [1, 2, 3, 4], metric)
        assert list(curve_fcst) == [1, 2, 3, 4] and np.all(np.abs(curve_ref - curve_fcst ** 2) < 1.5)
        want = R.metric_optimizer_curve(obs, obs ** 2, [1, 2, 3, 4], metric)
        R.same_bits(curve_ref, want[0])
    x = amd.get_optimal_threshold([0, 1, 1.4, 1.6, 2], [1, 2, 2.4, 2.6, 3], 1.5, amd.Bias)
    assert 2.4 < x < 2.6 and x == 2.5


# ---- input forms ----------------------------------------------------------------------------------------------------------------------------------
def test_tensors_views_and_float64(amd, torch):
    from gridpp_amd import _capi
    n = 257
    ref, fcst = data(n, False)
    thresholds = np.array(R.THRESHOLDS, F)
    for metric in (amd.Ets, amd.Kss):
        want = np.array([expected(n, False, t, metric) for t in R.THRESHOLDS], F)
        want_curve = R.metric_optimizer_curve(ref, fcst, thresholds, metric)
        d_ref, d_fcst = torch.from_numpy(ref.copy()).cuda(), torch.from_numpy(fcst.copy()).cuda()
        pad = torch.full((n + 3,), 77.0, device="cuda")
        v_ref, v_fcst = pad.clone(), pad.clone()
        v_ref[3:] = d_ref
        v_fcst[3:] = d_fcst
        strided = torch.stack([d_fcst, pad[:n]], dim=1)[:, 0]   # not contiguous
        forms = [(ref.astype(np.float64), fcst.astype(np.float64)), (list(ref), list(fcst)), (d_ref, d_fcst), (v_ref[3:], v_fcst[3:]),
                 (d_ref, strided), (d_ref.double(), d_fcst.double())]
        for r, f in forms:
            R.same_bits([amd.get_optimal_threshold(r, f, t, metric) for t in R.THRESHOLDS], want)
            curve = amd.metric_optimizer_curve(r, f, thresholds, metric)
            assert isinstance(curve[0], np.ndarray) and isinstance(curve[1], np.ndarray)
            R.same_bits(curve[0], want_curve[0])
            R.same_bits(curve[1], want_curve[1])
        # a longer ref: only the first len(fcst) values count
        R.same_bits(amd.get_optimal_threshold(np.concatenate([ref, [9, 9, 9]]), fcst, 2.0, metric), want[1])
        R.same_bits(amd.get_optimal_threshold(torch.cat([d_ref, pad[:5]]), d_fcst, 2.0, metric), want[1])
        # GPP_HOST_F64 through the C-ABI: doubles that are no float32 values, rounded on the device
        lib = _capi.lib()
        wide_ref, wide_fcst = ref.astype(np.float64) * (1 + 2.0 ** -30), fcst.astype(np.float64) * (1 + 2.0 ** -30)
        assert np.array_equal(wide_ref.astype(F), ref) and np.array_equal(wide_fcst.astype(F), fcst)
        out = C.c_float(7)
        assert lib.gpp_get_optimal_threshold(C.c_void_p(wide_ref.ctypes.data), C.c_void_p(wide_fcst.ctypes.data), n, 2.0, metric, C.byref(out),
                                             _capi.MEM_HOST | _capi.HOST_F64) == _capi.GPP_OK
        R.same_bits(out.value, want[1])
    with pytest.raises(ValueError, match="either all field arguments are torch CUDA tensors or none is"):
        amd.get_optimal_threshold(d_ref, fcst, 2.0, amd.Ets)


# ---- repeated calls ----------------------------------------------------------------------------------------------------------------------------------
def test_repeat_calls_around_release_workspaces(amd):
    sizes = (1025, 255, 1025, 64)
    first = [amd.get_optimal_threshold(*data(n, False), 2.0, amd.Ets) for n in sizes]
    amd.release_workspaces()
    again = [amd.get_optimal_threshold(*data(n, False), 2.0, amd.Ets) for n in sizes]
    R.same_bits(first, [expected(n, False, 2.0, R.Ets) for n in sizes])
    R.same_bits(again, first)
    amd.release_workspaces()
    R.same_bits(amd.get_optimal_threshold(*data(257, True), 0.5, amd.Hss), expected(257, True, 0.5, R.Hss))
