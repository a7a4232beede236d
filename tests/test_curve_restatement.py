"""CPU: the numpy float32 restatement of tests/curve_ref.py reproduces every known answer of the reference's
tests/test_apply_curve.py, tests/test_interpolate.py, tests/test_quantile_mapping.py and tests/test_monotonize.py
(tests/golden/curve_known_answers.json).  This pins the checker that the GPU tests hold the curve kernels to: the reference
itself cannot be built where this suite runs, so the chain is known answers -> restatement -> kernels."""
import numpy as np
import pytest

from tests import curve_ref as R

CASES = R.CASES


class Restatement:
    """tests/curve_ref.py behind the reference's call forms (a scalar x, the reference's own argument checks)"""
    @staticmethod
    def apply_curve(fcst, curve_ref, curve_fcst, policy_below, policy_above):
        cr, cf = np.asarray(curve_ref, np.float32), np.asarray(curve_fcst, np.float32)
        if cr.ndim == 2 or cf.ndim == 2:   # [[]]: no overload takes it
            raise ValueError("curve_ref and curve_fcst must be 1-D or 3-D")
        if cr.ndim == 3 and (cr.shape != cf.shape or np.shape(fcst) != cr.shape[:2]):   # curve.cpp:111-116
            raise ValueError("dimension sizes mismatch")
        return R.apply_curve(fcst, cr, cf, policy_below, policy_above)

    @staticmethod
    def interpolate(x, iX, iY):
        if np.ndim(x) == 0 and not np.isfinite(x):   # util.cpp:378-379 comes before the size check
            return np.float32(np.nan)
        if len(iX) != len(iY):
            raise ValueError("Dimension mismatch. Cannot interpolate.")
        return R.interpolate(x, iX, iY)

    quantile_mapping_curve = staticmethod(R.quantile_mapping_curve)
    monotonize_curve = staticmethod(R.monotonize_curve)


def test_known_answers_cover_the_four_reference_files():
    srcs = [c["source"].split(":")[0] for c in CASES]
    assert set(srcs) == {"tests/test_apply_curve.py", "tests/test_interpolate.py", "tests/test_quantile_mapping.py", "tests/test_monotonize.py"}
    assert srcs.count("tests/test_apply_curve.py") >= 30
    assert srcs.count("tests/test_interpolate.py") >= 25
    assert srcs.count("tests/test_quantile_mapping.py") >= 10
    assert sum(c["id"].startswith("mono_with_missing_") for c in CASES) == 14   # test_monotonize.py:99-144
    assert len({c["id"] for c in CASES}) == len(CASES)
    assert sum("raises" in c for c in CASES) >= 25
    for c in CASES:
        assert c["source"].split(":")[1].isdigit()


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_restatement_reproduces_known_answer(case):
    R.check_case(case, Restatement)


def test_restatement_agrees_with_the_oracles_interpolate():
    """oracle/gridpp_oracle.c carries its own transcription of util.cpp:339-414 (the quantile_fast checker uses it): two independent
    readings of the same lines agree bit for bit on random curves with duplicates"""
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    for _ in range(300):
        C = int(rng.integers(1, 9))
        iX = np.sort(np.round(rng.normal(0, 1, C) * 3) / 3).astype(np.float32)
        iY = rng.normal(0, 1, C).astype(np.float32)
        xs = np.concatenate([rng.normal(0, 1.2, 6).astype(np.float32), iX[:3]])
        ours = R.interpolate(xs, iX, iY)
        theirs = np.array([O.interpolate(float(x), iX, iY) for x in xs], np.float32)
        np.testing.assert_array_equal(ours, theirs)


def test_restatement_is_not_vacuous():
    """dropping the duplicate rule changes known answers; a bisection on an unsorted curve changes a crafted case"""
    by_id = {c["id"]: c for c in CASES}
    for cid in ("interp_duplicates_all", "interp_duplicates_edge_1", "interp_duplicates_edge_0"):
        c = by_id[cid]
        with np.errstate(all="ignore"):
            got = R.interpolate([c["x"]], c["iX"], c["iY"], duplicate_rule=False)
        assert not np.allclose(got, c["expected"], atol=1e-5, equal_nan=False)
    # the scans on an unsorted curve do not find what a bisection finds: x = 2.5 on iX = [0, 3, 1, 2, 4]
    iX, iY = [0, 3, 1, 2, 4], [0, 30, 10, 21, 40]
    scan = R.interpolate([2.5], iX, iY)
    bis = R.interpolate([2.5], iX, iY, bisect=True)
    # forward scan: 0 < 2.5 -> 0, then 3 > 2.5 stops: lower = 0; backward scan: 4 > 2.5 -> 4, then 2 < 2.5 stops: upper = 4
    np.testing.assert_array_equal(scan, np.float32(0) + np.float32(40) * np.float32(2.5) / np.float32(4))
    assert not np.array_equal(scan, bis)
    # on a sorted curve without invalid entries the two agree bit for bit (what licenses the kernels' bisection)
    rng = np.random.default_rng(11)
    for _ in range(200):
        C = int(rng.integers(1, 12))
        sX = np.sort(np.round(rng.normal(0, 1, C) * 2) / 2).astype(np.float32)
        sY = rng.normal(0, 1, C).astype(np.float32)
        xs = np.concatenate([rng.uniform(sX[0], sX[-1], 5).astype(np.float32), sX])
        np.testing.assert_array_equal(R.interpolate(xs, sX, sY), R.interpolate(xs, sX, sY, bisect=True))


def test_apply_curve_is_defined_for_every_curve_with_valid_ends():
    """the claim the kernels rely on: first and last curve_fcst valid and the input between them -> both scan indices exist, for
    unsorted curves with NaNs as well"""
    rng = np.random.default_rng(3)
    for _ in range(4000):
        C = int(rng.integers(1, 8))
        f = rng.normal(0, 1, C).astype(np.float32)
        f[rng.random(C) < 0.3] = np.nan
        f[0], f[-1] = sorted(rng.normal(0, 1, 2).astype(np.float32))
        x = rng.uniform(f[0], f[-1], 4).astype(np.float32)
        x = x[(x >= f[0]) & (x <= f[-1])]
        lo, hi = R.scan_indices(x, f)
        assert (lo >= 0).all() and (hi >= 0).all()
