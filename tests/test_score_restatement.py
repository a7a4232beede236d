"""CPU: the numpy restatement of calc_score / neighbourhood_score (tests/score_ref.py) against the reference's own known answers
(tests/golden/score_known_answers.json: the 24 rows of its tests/test_metric_optimizer.py), hand-worked tables for every guard branch
of metric_optimizer.cpp:207-244, the counting rules of the vector form, and one neighbourhood_score small enough to check by hand."""
import numpy as np
import pytest

from tests import score_ref as R

NAMES = sorted(R.METRIC)


def nan_or(v):
    return np.nan if v is None else v


def test_enum_values():
    assert R.METRIC == {"Ets": 0, "Ts": 1, "Kss": 20, "Pc": 30, "Bias": 40, "Hss": 50}   # include/gridpp.h:103-110
    assert (R.Ets, R.Ts, R.Kss, R.Pc, R.Bias, R.Hss) == tuple(R.METRIC[n] for n in ("Ets", "Ts", "Kss", "Pc", "Bias", "Hss"))


@pytest.mark.parametrize("name", NAMES)
def test_known_answers(name):
    k = R.KNOWN
    assert len(k["thresholds"]) * len(k["expected"]) == 24
    for t, threshold in enumerate(k["thresholds"]):
        got = R.calc_score(k["obs"], k["fcst"], threshold, R.METRIC[name])
        assert isinstance(got, np.float32)
        np.testing.assert_almost_equal(got, nan_or(k["expected"][name][t]), R.GOLDEN["decimals"])      # the reference's comparison
        R.same_bits(R.calc_score(k["obs"], k["fcst"], threshold, threshold, R.METRIC[name]), got)   # the four-argument form passes it twice


@pytest.mark.parametrize("row", R.GUARDS, ids=["%s-%d-%d-%d-%d" % (r[4], r[0], r[1], r[2], r[3]) for r in R.GUARDS])
def test_guard_branches(row):
    a, b, c, d, name, want = row
    got = R.calc_score(a, b, c, d, R.METRIC[name])
    if want is None:
        assert np.isnan(got)
    else:
        assert got == np.float32(want)


def test_hand_worked_table():
    """a = 3, b = 1, c = 2, d = 4 by hand, with the reference's roundings"""
    F, D = np.float32, np.float64
    a, b, c, d = F(3), F(1), F(2), F(4)
    ar = F(D(4) / D(10) * D(5))                                   # 2
    assert R.calc_score(a, b, c, d, R.Ets) == F(D(a - ar) / D(a + b + c - ar))   # 1 / 4
    assert R.calc_score(a, b, c, d, R.Ets) == F(0.25)
    assert R.calc_score(a, b, c, d, R.Ts) == F(0.5)
    assert R.calc_score(a, b, c, d, R.Pc) == F(7) / F(10)
    assert R.calc_score(a, b, c, d, R.Kss) == F(D(10) / D(25))
    assert R.calc_score(a, b, c, d, R.Bias) == F(1) - F(1) / F(3)
    assert R.calc_score(a, b, c, d, R.Hss) == F(D(2) * D(10) / D(F(5 * 6 + 4 * 5)))
    # the promotions matter: Ts divides in double and rounds once, Pc divides in float
    a, b, c, d = F(1) / F(3), F(1) / F(7), F(1) / F(11), F(1) / F(13)
    assert R.calc_score(a, b, c, d, R.Ts) == F(D(a) / D(a + b + c))
    assert R.calc_score(a, b, c, d, R.Pc) == (a + d) / (a + b + c + d)
    assert R.calc_score(a, b, c, d, R.Hss) == F(D(2.0) * D(a * d - b * c) / D((a + c) * (c + d) + (a + b) * (b + d)))


def test_arrays_and_scalars_agree():
    rng = np.random.default_rng(3)
    t = (rng.integers(0, 6, (4, 50)) / np.float32(7)).astype(np.float32)
    for metric in R.METRICS:
        whole = R.calc_score_table(t[0], t[1], t[2], t[3], metric)
        assert whole.dtype == np.float32
        each = np.array([R.calc_score_table(t[0, i], t[1, i], t[2, i], t[3, i], metric) for i in range(50)], np.float32)
        R.same_bits(whole, each)


def test_unknown_metric():
    for metric in (2, -1, 10, 60):
        with pytest.raises(ValueError, match="Unknown metric"):
            R.calc_score(1, 1, 1, 1, metric)


def test_counting_rules():
    nan = np.nan
    #            a    b    c    d    none  c(NaN fcst)  d(NaN fcst)  none
    ref = [2.0, 0.0, 2.0, 0.0, nan, 2.0, 0.0, nan]
    fcst = [2.0, 2.0, 0.0, 0.0, 2.0, nan, nan, nan]
    assert R.counts(ref, fcst, 1.0, 1.0) == (1, 1, 2, 2)
    assert R.counts(ref, fcst, 1.0, 3.0) == (0, 0, 3, 3)           # fthreshold moves only the forecast's side
    assert R.counts([1.0], [1.0], 1.0, 1.0) == (0, 0, 0, 1)        # equal to the threshold: not above
    assert R.counts([], [], 0.0, 0.0) == (0, 0, 0, 0)
    assert R.counts([5, 5, 5], [5, 5], 1.0, 1.0) == (2, 0, 0, 0)   # a longer ref: the first len(fcst) elements
    with pytest.raises(ValueError, match="ref and fcst not the same size"):
        R.counts([5], [5, 5], 1.0, 1.0)
    assert R.calc_score([], [], 0.0, R.Bias) == 1
    for metric in (R.Ets, R.Ts, R.Kss, R.Pc, R.Hss):
        assert np.isnan(R.calc_score([], [], 0.0, metric))


def test_neighbourhood_score_by_hand():
    """3 x 3 Cartesian grid (1 km), 2 observations, half width 1, threshold 0.5.
    ref_grid: 1.0 at (0, 0), 0.0 at (2, 2), NaN elsewhere.  fcst is 1 everywhere, so (0, 0) is an `a` cell and (2, 2) a `b` cell.
    Windows: corner (0, 0) holds 4 cells, one of them a -> a = 1/4, b = 0; the centre holds 9 cells: a = b = 1/9; ..."""
    from oracle import oracle as O
    F, D = np.float32, np.float64
    lats, lons = R.geometry(3, 3, False)
    og = O.Pts(lats.ravel(), lons.ravel(), ctype=O.Cartesian)
    op = O.Pts([100.0, 1900.0], [-200.0, 2100.0], ctype=O.Cartesian)
    fcst, ref = np.ones((3, 3), np.float32), [1.0, 0.0]
    a, b, c, d = R.hoods(og, op, fcst, ref, 1, 0.5)
    q, n, s = F(D(1) / D(4)), F(D(1) / D(9)), F(D(1) / D(6))
    np.testing.assert_array_equal(a, [[q, s, 0], [s, n, 0], [0, 0, 0]])
    np.testing.assert_array_equal(b, [[0, 0, 0], [0, n, s], [0, s, q]])
    assert not c.any() and not d.any()
    ts = R.neighbourhood_score(og, op, fcst, ref, 1, R.Ts, 0.5)
    nan = np.nan
    np.testing.assert_array_equal(ts, [[1, 1, nan], [1, 0.5, 0], [nan, 0, 0]])
    bias = R.neighbourhood_score(og, op, fcst, ref, 1, R.Bias, 0.5)
    np.testing.assert_array_equal(bias, [[1, 1, 1], [1, 0, 0], [1, 0, 0]])                 # b == c = 0 -> 1; a window with the b cell: 1 - b / b = 0
    pc = R.neighbourhood_score(og, op, fcst, ref, 1, R.Pc, 0.5)
    np.testing.assert_array_equal(pc, [[1, 1, nan], [1, 0.5, 0], [nan, 0, 0]])             # (a + d) / N, 0 / 0 where no observation falls
    for metric in (R.Ets, R.Kss, R.Hss):                                                    # c = d = 0 everywhere: their guards
        out = R.neighbourhood_score(og, op, fcst, ref, 1, metric, 0.5)
        assert np.isnan(out[0, 2]) and np.isnan(out[2, 0])
    # the checks, in order
    with pytest.raises(ValueError, match="Grid size"):
        R.neighbourhood_score(og, op, np.ones((3, 4)), [1.0], 0, 99, 0.5)
    with pytest.raises(ValueError, match="half_width"):
        R.neighbourhood_score(og, op, fcst, [1.0], 0, 99, 0.5)
    with pytest.raises(ValueError, match="Unknown metric"):
        R.neighbourhood_score(og, op, fcst, [1.0], 1, 99, 0.5)
    with pytest.raises(ValueError, match="Points size"):
        R.neighbourhood_score(og, op, fcst, [1.0], 1, R.Ets, 0.5)
