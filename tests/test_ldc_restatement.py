"""CPU: the restatement of local_distribution_correction (tests/ldc_ref.py) against answers derived by hand, and the measurement
that justifies its tie rule.

The reference has no numeric test of this function, so the GPU tests (tests/test_gpu_ldc_parity.py) hold the kernels to the
restatement and these pins hold the restatement to src/api/local_distribution_correction.cpp:33-203.

The tie rule.  The reference sorts the (value, rho) pairs by value alone with an unstable sort.  Where no two values tie that is
a total order and a sort by (value, rho) gives the same curve, bit for bit.  Where values tie (precipitation rounded to 0.5 mm:
many zeros) the order of the rho within a run of equal values -- and with it the cumulative curve -- is whatever the sort and
the R-tree's enumeration order make it: a stable sort by value (one of the orders the reference may produce) and the sort by
(value, rho) differ in more than a tenth of the cells, and the stable sort's result changes when the neighbours are enumerated in
another order.  Sorting ties by rho ascending is a total order on what the algorithm can see."""
import numpy as np
import pytest

from tests import ldc_ref as R

F = np.float32


@pytest.fixture(scope="module")
def O():
    import __graft_entry__ as g
    g.build()
    from oracle import oracle
    return oracle


def test_hand_derived_answers(O):
    """A 1 x 3 Cartesian grid with every cell at the origin, 4 stations at the origin (rho = 1), pobs 1..4, pbackground 2..8,
    quantiles 0 / 1, min_points 1, Barnes 2 500: the curves are ref (0, 1, 2, 3, 4) and fcst (0, 2, 4, 6, 8) at the quantiles
    (0, 1/4, 1/2, 3/4, 1), sum_rho = 4.
      background 3      branch 4: q = 1/4 + 1/4 (3 - 2) / (4 - 2) = 0.375, new_ref = 1.5, w0 = 1 - exp(-0.04):
                        w0 1.5 + (1 - w0) 3 = 2.941184
      background 10     branch 3: 10 + (4 - 8) = 6
      background 0.005  branch 1: 0"""
    zero = np.zeros((1, 3))
    g, p = O.Pts(zero, zero, ctype=1), O.Pts(np.zeros(4), np.zeros(4), ctype=1)
    cands = R.candidates(O, g, p, O.Struct("Barnes", 2500))
    assert all(list(idx) == [0, 1, 2, 3] and (rho == 1).all() for idx, rho in cands)
    out, tags, count = R.ldc(O, cands, [[3, 10, 0.005]], [1, 2, 3, 4], [2, 4, 6, 8], 0, 1, 1)
    assert list(tags) == [R.B4, R.B3, R.B1] and list(count) == [4, 4, 4]
    w0 = 1 - np.exp(-0.04)
    np.testing.assert_allclose(out[0, 0], w0 * 1.5 + (1 - w0) * 3, rtol=3e-7)
    assert abs(float(out[0, 0]) - 2.941184) < 5e-7
    assert out[0, 1] == 6.0 and out[0, 2] == 0.0
    # the (T, S) form pools the times: the same four pairs as two times of two stations
    p2 = O.Pts(np.zeros(2), np.zeros(2), ctype=1)
    out2, _, count2 = R.ldc(O, R.candidates(O, g, p2, O.Struct("Barnes", 2500)), [[3, 10, 0.005]], [[1, 2], [3, 4]], [[2, 4], [6, 8]], 0, 1, 1)
    np.testing.assert_array_equal(out2, out)
    assert list(count2) == [4, 4, 4]


def test_hand_derived_edges(O):
    """the same stations: too few pairs, invalid background, dropped pairs, no rain observed (2a / 2b / 2c), an empty trimmed range"""
    zero = np.zeros((1, 4))
    g, p = O.Pts(zero, zero, ctype=1), O.Pts(np.zeros(4), np.zeros(4), ctype=1)
    cands = R.candidates(O, g, p, O.Struct("Barnes", 2500))
    bg = np.array([[3, np.nan, np.inf, 0.005]], F)
    out, tags, _ = R.ldc(O, cands, bg, [1, 2, 3, 4], [2, 4, 6, 8], 0, 1, 5)   # 4 pairs < 5
    assert list(tags) == [R.FEW, R.INVALID, R.INVALID, R.FEW]
    np.testing.assert_array_equal(out, bg)
    # NaN and negative entries drop their pair: (2, 4) and (3, 6) stay -> ref (0, 2, 3), fcst (0, 4, 6); 7 >= 6: 7 + (3 - 6)
    out, tags, count = R.ldc(O, cands, [[7, 7, 7, 7]], [np.nan, 2, 3, 4], [2, 4, 6, -8], 0, 1, 0)
    assert list(count) == [2] * 4 and list(tags) == [R.B3] * 4 and (out == 4.0).all()
    # no rain observed, fcst_last = 0.02: 0.05 < 0.06 (2a); 0.08 < 0.1 (2b); 0.5 stays (2c); 0.0099999998 < 0.01 in double (1)
    out, tags, _ = R.ldc(O, cands, np.array([[0.05, 0.08, 0.5, 0.01]], F), [0, 0, 0, 0], [0.0, 0.01, 0.02, 0.02], 0, 1, 0)
    assert list(tags) == [R.B2A, R.B2B, R.B2C, R.B1]
    np.testing.assert_array_equal(out, np.array([[0, 0, 0.5, 0]], F))
    # quantiles 0.5 / 0.5: d0 == d1, the curve is the lone (0, 0) point and branch 2 applies
    out, tags, _ = R.ldc(O, cands, np.array([[0.05, 0.5, 3, 0.001]], F), [1, 2, 3, 4], [2, 4, 6, 8], 0.5, 0.5, 0)
    assert list(tags) == [R.B2B, R.B2C, R.B2C, R.B1]
    np.testing.assert_array_equal(out, np.array([[0, 0.5, 3, 0]], F))


def test_hand_derived_zero_rho(O):
    """One cell at the origin, ten stations, T = 1, CrossValidation(Barnes 2 500, 1 000), quantiles 0.2 / 0.8, background 5.5: ten pairs,
    d0 = (int)(10 x 0.2f) = 2, d1 = (int)(10 x 0.8f) = 8.  Stations 2 ... 7 lie within the cross-validation distance (rho = 0), the other
    four 2 000 m away (rho = exp(-0.32) = 0.726149).

    The trimmed ref curve all rho = 0, the fcst curve not: pobs = 1 ... 10 by station, so the six middle values 3 ... 8 are the inner
    stations'; pbackground gives the outer stations 4 ... 7.  ref: values (0, 3, ..., 8), cumulative rho all 0, total 0, quantiles
    (0, NaN x 6) -- the leading 0 is never normalised (:151).  fcst: values (0, 3, 4, 5, 6, 7, 8), cumulative rho (0, 0, r, 2r, 3r, 4r, 4r),
    quantiles (0, 0.2, 0.35, 0.5, 0.65, 0.8, 0.8).  ref_last = 8 > 0 and 5.5 < fcst_last = 8: branch 4.  q = 0.5 + 0.15 / 2 = 0.575.  In the
    second interpolate 0.575 is neither > NaN nor < 0; the scan from the front stops at index 0; the scan from the back skips the NaN,
    meets 0 < 0.575 and leaves with no index: the reference indexes with (int) NaN there (util.cpp:391-396), the project's rule is NaN
    (gridpp_amd/csrc/curve.h).  w0 = 1 - exp(-0.01 x 4r) is finite and not 0, so the result is NaN.

    The mirror (pobs and pbackground exchanged): the fcst quantiles are (0, NaN x 6), 5.5 lies between its entries 5 and 6, q is NaN
    and interpolate of an invalid x is NaN.

    All ten stations within the distance: both totals and sum_rho are 0, w0 = 1 - exp(0) = 0, and 0 x NaN + 1 x 5.5 is NaN."""
    g = O.Pts([[0.0]], [[0.0]], ctype=1)
    x = np.array([2000.0, 0.0, 100, 200, 300, 400, 500, 600, -2000.0, 0.0])
    y = np.array([0.0, 2000.0, 0, 0, 0, 0, 0, 0, 0.0, -2000.0])
    st = O.Struct("Barnes", 2500).cross_validation(1000)
    cands = R.candidates(O, g, O.Pts(y, x, ctype=1), st)
    rho = F(np.exp(-0.5 * (2000.0 / 2500.0) ** 2))
    np.testing.assert_array_equal(cands[0][0], np.arange(10))
    np.testing.assert_allclose(cands[0][1], [rho, rho, 0, 0, 0, 0, 0, 0, rho, rho], rtol=2e-7)
    middle = np.arange(1.0, 11.0)
    spread = [4, 5, 9, 10, 1, 2, 3, 8, 6, 7]
    for pobs, pbg, zero in ((middle, spread, "sum_r"), (spread, middle, "sum_f")):
        sums = {}
        out, tags, count = R.ldc(O, cands, [[5.5]], pobs, pbg, 0.2, 0.8, 0, sums=sums)
        other = "sum_f" if zero == "sum_r" else "sum_r"
        assert list(tags) == [R.B4] and list(count) == [10]
        assert sums[zero][0] == 0 and abs(sums[other][0] - 4 * rho) < 1e-6 and abs(sums["sum_rho"][0] - 4 * rho) < 1e-6
        assert abs(sums["w0"][0] - (1 - np.exp(-0.04 * rho))) < 1e-7
        assert np.isnan(out[0, 0]), (zero, out)
    # the fcst quantiles of the first case, as derived: the background maps to q = 0.575
    xs, qs, total = R._curve(np.array(spread, F), cands[0][1], 2, 8, False, F(0.2), F(0.8))
    np.testing.assert_array_equal(xs, [0, 3, 4, 5, 6, 7, 8])
    np.testing.assert_allclose(qs, [0, 0.2, 0.35, 0.5, 0.65, 0.8, 0.8], atol=1e-6)
    assert abs(O.interpolate(5.5, xs, qs) - 0.575) < 1e-6
    # every station inside
    inside = O.Pts(np.zeros(10), 100.0 * np.arange(10), ctype=1)
    cands = R.candidates(O, g, inside, st)
    assert (cands[0][1] == 0).all() and cands[0][0].size == 10
    sums = {}
    out, tags, _ = R.ldc(O, cands, [[5.5]], middle, spread, 0.2, 0.8, 0, sums=sums)
    assert list(tags) == [R.B4] and sums["sum_r"][0] == 0 and sums["sum_f"][0] == 0 and sums["sum_rho"][0] == 0 and sums["w0"][0] == 0
    assert np.isnan(out[0, 0])


def test_interpolate_with_an_undefined_index_is_nan(O):
    """the oracle's interpolate where one scan finds no valid entry on its side, and that nothing else moved: the defined cases of
    util.cpp:377-414 as before"""
    nan = np.nan
    assert np.isnan(O.interpolate(0.5, [0, nan, nan], [0, 3, 4]))        # no valid entry >= x from the back
    assert np.isnan(O.interpolate(0.5, [nan, nan, 1], [2, 3, 4]))        # no valid entry <= x from the front
    assert O.interpolate(0.5, [0, nan, 1], [2, 3, 4]) == 3.0             # both found: NaN entries are skipped
    assert O.interpolate(0.0, [0, nan, nan], [7, 3, 4]) == 7.0           # x on the one valid entry: both scans stop there
    assert O.interpolate(2.0, [0, 1], [5, 6]) == 6.0 and O.interpolate(-1.0, [0, 1], [5, 6]) == 5.0
    assert O.interpolate(0.25, [0, 1], [4, 8]) == 5.0


@pytest.fixture(scope="module")
def sensitivity(O):
    res = {}
    for rounded in (False, True):
        fx = R.FixtureA(rounded)
        g, p = fx.oracle_points(O)
        cands = R.candidates(O, g, p, O.Struct("Barnes", fx.H))
        args = (O, cands, fx.bg, fx.pobs, fx.pbg, fx.MINQ, fx.MAXQ, fx.MIN_POINTS)
        rng = np.random.default_rng(1)
        res[rounded] = dict(rule=R.ldc(*args), stable=R.ldc(*args, stable=True),
                            rule_shuffled=R.ldc(*args, order=rng.permutation),
                            stable_shuffled=R.ldc(*args, stable=True, order=rng.permutation))
    return res


# Another enumeration order changes sum_rho = a float32 sum of n <= 127 terms in [0, 1] by at most (n - 1) 2^-24 sum_rho < 1e-3, the
# weight w0 = 1 - exp(-0.01 sum_rho) by at most 1e-5, and the result by that times |new_ref - background|: the project's parity bound
# of 1e-5 max(|ref|, 1e-3) (the one tests/test_gpu_ldc_parity.py uses) covers it.
def close(a, b, four):
    a, b = a[0].ravel().astype(np.float64)[four], b[0].ravel().astype(np.float64)[four]
    return np.all(np.abs(a - b) <= 1e-5 * np.maximum(np.abs(a), 1e-3))


def differing(a, b):
    a, b = a[0].ravel(), b[0].ravel()
    return (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))


def test_on_tie_free_data_the_rule_is_the_sort_by_value(sensitivity):
    s = sensitivity[False]
    assert not differing(s["rule"], s["stable"]).any()
    # another enumeration order moves only the float32 sum_rho, and only branch 4 sees it
    moved = differing(s["rule"], s["rule_shuffled"])
    assert not moved[s["rule"][1] != R.B4].any()
    assert close(s["rule"], s["rule_shuffled"], s["rule"][1] == R.B4)


def test_on_rounded_data_a_sort_by_value_alone_is_not_a_function_of_its_input(sensitivity):
    s = sensitivity[True]
    n = s["rule"][0].size
    assert differing(s["rule"], s["stable"]).sum() > n / 10            # the two rules differ in more than a tenth of the cells
    assert differing(s["stable"], s["stable_shuffled"]).sum() > n / 10   # and the stable rule follows the enumeration order
    # the (value, rho) rule does not: only sum_rho's rounding is left
    four = s["rule"][1] == R.B4
    assert not differing(s["rule"], s["rule_shuffled"])[~four].any()
    assert close(s["rule"], s["rule_shuffled"], four)
    np.testing.assert_array_equal(s["rule"][1], s["rule_shuffled"][1])
