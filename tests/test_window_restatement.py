"""CPU: tests/window_ref.py, the float32 restatement the window kernels are compared with, reproduces every known answer of the
reference's tests/test_window.py (tests/golden/window_known_answers.json) exactly -- and the property that decides the kernel's
shape: the reference's Sum is a difference of two sequential float32 prefix sums, which is not the exact sum of the window."""
import numpy as np
import pytest

from tests import window_ref as R


@pytest.mark.parametrize("case", R.CASES, ids=[c["id"] for c in R.CASES])
def test_restatement_reproduces_the_reference_known_answers(case):
    R.check_case(case, R)


def test_the_golden_file_lists_every_test_of_the_reference():
    ids = [c["id"] for c in R.CASES]
    assert len(ids) == len(set(ids)) == 39
    # test_count_nan: two flags x two values x three calls; test_before / test_centered: four calls each; test_invalid_length: two lengths
    assert sum(i.startswith("count_nan_") for i in ids) == 12
    assert sum(i.startswith("before_") for i in ids) == 4 and sum(i.startswith("centered_") for i in ids) == 4
    for name in ("sum", "count", "mean", "min", "max", "sum_before", "count_before", "sum_missing_edge", "count_missing", "sum_keep_missing", "edge_case",
                 "edge_case2", "no_times", "no_cases", "no_anything", "invalid_length_0", "invalid_length_1", "long_length", "time_length_1"):
        assert name in ids


def test_checks_run_in_the_reference_order():
    """window.cpp:10-28: length <= 0 first, then the two empty shapes, only then the odd-length rule"""
    for shape in ((0, 0), (0, 5), (5, 0), (5, 5)):
        with pytest.raises(ValueError, match="must be > 0"):
            R.window(np.zeros(shape), 0, R.Sum)
    assert R.window(np.zeros((0, 5)), 4, R.Sum).shape == (0, 0)
    assert R.window(np.zeros((5, 0)), 4, R.Sum).shape == (5, 0)
    with pytest.raises(ValueError, match="odd number"):
        R.window(np.zeros((5, 5)), 4, R.Sum)
    assert R.window(np.zeros((5, 5)), 4, R.Sum, True).shape == (5, 5)
    for statistic in (R.Quantile, R.Unknown, 7):
        with pytest.raises(RuntimeError, match="Cannot compute statistic"):
            R.window(np.zeros((5, 5)), 3, statistic)


def test_mean_with_an_empty_window_after_valid_values_is_nan():
    """window.cpp:86-90 divides whenever counts[end] != 0, also where the window itself holds nothing: NaN / 0"""
    out = R.window([[1, np.nan, np.nan, np.nan, 2]], 2, R.Mean, True, False, False)
    np.testing.assert_array_equal(out, [[1, 1, np.nan, np.nan, 2]])
    out = R.window([[np.nan, np.nan, 2]], 1, R.Sum, True, False, False)
    np.testing.assert_array_equal(out, [[np.nan, np.nan, 2]])


def test_statistics_over_the_window_follow_calc_statistic():
    row = [[4, np.nan, 1, np.inf, 7, 2]]
    np.testing.assert_array_equal(R.window(row, 3, R.Median, False, False, False), [[4, 2.5, 1, 4, 4.5, 4.5]])
    np.testing.assert_array_equal(R.window(row, 3, R.Max, True, False, True), [[np.nan, np.nan, 4, 1, 7, 7]])
    np.testing.assert_array_equal(R.window(row, 3, R.Min, True, True, False), [[4, np.nan, np.nan, np.nan, np.nan, np.nan]])
    np.testing.assert_array_equal(R.window(row, 3, R.Variance, False, False, False), [[0, 2.25, 0, 9, 6.25, 6.25]])
    np.testing.assert_array_equal(R.window(row, 3, R.Std, False, False, False), [[0, 1.5, 0, 3, 2.5, 2.5]])
    R.check_random_choice(R.window(row, 3, R.Max, False, False, False), row, 3, False, False, False)   # (the maximum is a member)
    with pytest.raises(AssertionError):
        R.check_random_choice(np.zeros((1, 6), np.float32), row, 3, False, False, False)


def test_the_scan_form_sum_is_not_the_exact_window_sum():
    """Why the kernel adds sequentially per row and is no parallel scan: on gamma-distributed float32 values (precipitation-like) the
    reference's P[end] - P[start - 1] at T = 600 strays from the exact sum of the window's values by far more than the project's
    1e-5 parity bound.  Any other order of the additions gives other roundings of P, so only the reference's order reproduces the
    reference."""
    rng = np.random.default_rng(600)
    T, length = 600, 3
    a = rng.gamma(0.5, 4.0, (64, T)).astype(np.float32)
    got = R.window(a, length, R.Sum, True, False, False).astype(np.float64)
    c = np.concatenate([np.zeros((64, 1)), np.cumsum(a.astype(np.float64), axis=1)], axis=1)   # exact to ~1e-16 relative
    x = np.arange(T)
    start = np.maximum(x - length + 1, 0)
    exact = c[:, x + 1] - c[:, start]
    worst = float(np.max(np.abs(got - exact) / np.maximum(exact, 1e-3)))
    print("scan-form Sum against the exact window sum, T = %d, length %d: worst relative difference %.3g" % (T, length, worst))
    assert worst > 1e-5
    # where the window starts at column 0 the result is P[end] itself, a plain sum of at most `length` positive values: two roundings
    # of 2^-24 each at the most.  The stray comes from the difference of two LONG prefixes, not from float32 as such.
    head = float(np.max(np.abs(got[:, :length] - exact[:, :length]) / exact[:, :length]))
    assert head <= 2.0 ** -23 < 1e-5 < worst
