"""float32 numpy restatement of the reference's curve functions, the yardstick of the curve kernels:

    interpolate              src/api/util.cpp:339-426 (get_lower_index / get_upper_index as linear scans)
    apply_curve              src/api/curve.cpp:6-133
    monotonize_curve         src/api/curve.cpp:134-250
    quantile_mapping_curve   src/api/quantile_mapping.cpp:5-46

Vectorised over the values (or cells) with a python loop over the C curve entries, so that a 2000 x 2000 x 10 case is
affordable.  A curve is (C,) (one for all values) or (N, C) (one per value).  Every operation is float32, in the reference's
order.  tests/test_curve_restatement.py pins it to the reference's own known answers.

Where the reference's index is undefined ((int) NaN: no valid entry on the side a scan walks) the result is NaN.  That is
outside the pinned behaviour; the library does the same."""
import json
import os

import numpy as np

OneToOne, MeanSlope, NearestSlope, Zero, Unchanged = 0, 10, 20, 30, 40
POLICIES = (OneToOne, MeanSlope, NearestSlope, Zero, Unchanged)
F = np.float32


def _f32(a):
    return np.asarray(a, dtype=np.float32)   # (not ascontiguousarray: it turns a scalar into a 1-D array)


def valid(v):   # util.cpp:16-18
    return np.isfinite(v)


def _col(X, i):
    return X[..., i]


def scan_indices(x, X):
    """get_lower_index / get_upper_index (util.cpp:339-376) for every x; -1 where the reference's index stays undefined."""
    n, C = x.shape[0], X.shape[-1]
    lower, upper = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    done = np.zeros(n, bool)
    for i in range(C):
        c = np.broadcast_to(_col(X, i), (n,))
        ok = valid(c) & ~done
        lower[ok & (c <= x)] = i
        done |= ok & (c >= x)
    done = np.zeros(n, bool)
    for i in range(C - 1, -1, -1):
        c = np.broadcast_to(_col(X, i), (n,))
        ok = valid(c) & ~done
        upper[ok & (c >= x)] = i
        done |= ok & (c <= x)
    return lower, upper


def bisect_indices(x, X):
    """What a bisection finds (only right for a sorted curve without invalid entries): for the non-vacuity test."""
    assert X.ndim == 1
    lb, ub = np.searchsorted(X, x, side="left"), np.searchsorted(X, x, side="right")
    eq = lb < ub
    lower = np.where(eq, lb, lb - 1)
    upper = np.where(eq, ub - 1, np.where(lb < X.shape[0], lb, -1))
    return lower.astype(np.int64), upper.astype(np.int64)


def _take(X, idx, n):
    idx = np.maximum(idx, 0)
    if X.ndim == 1:
        return X[idx]
    return np.take_along_axis(X, idx[:, None], axis=1)[:, 0]


def interpolate(x, iX, iY, duplicate_rule=True, bisect=False):
    """util.cpp:377-426 for an array x (any shape); iX / iY are (C,) or x.shape + (C,)."""
    x = _f32(x)
    shape = x.shape
    x = x.reshape(-1)
    n = x.shape[0]
    iX, iY = _f32(iX), _f32(iY)
    if iX.ndim > 1:
        iX, iY = iX.reshape(n, -1), iY.reshape(n, -1)
    C = iX.shape[-1]
    out = np.full(n, np.nan, F)
    if C == 0 or n == 0:
        return out.reshape(shape)
    ok = valid(x)
    last_x, first_x = np.broadcast_to(_col(iX, C - 1), (n,)), np.broadcast_to(_col(iX, 0), (n,))
    with np.errstate(all="ignore"):
        hi = ok & (x > last_x)
        lo = ok & ~hi & (x < first_x)
        mid = ok & ~hi & ~lo
        out[hi] = np.broadcast_to(_col(iY, C - 1), (n,))[hi]
        out[lo] = np.broadcast_to(_col(iY, 0), (n,))[lo]
        i0, i1 = bisect_indices(x, iX) if bisect else scan_indices(x, iX)
        x0, x1, y0, y1 = _take(iX, i0, n), _take(iX, i1, n), _take(iY, i0, n), _take(iY, i1, n)
        half = (y0 + y1) / F(2)
        first, last = i0 == 0, i1 == C - 1
        dup = np.where(first & last, half, np.where(first, y1, np.where(last, y0, half)))   # util.cpp:398-407
        lin = y0 + (y1 - y0) * (x - x0) / (x1 - x0)
        y = np.where(x0 == x1, dup, lin) if duplicate_rule else lin
        y = np.where((i0 < 0) | (i1 < 0), F(np.nan), y).astype(F)
    out[mid] = y[mid]
    return out.reshape(shape)


def _slope(policy, below, C, sO, sF, lO, lF, ref, fcst, n):
    """curve.cpp:45-72 for one policy on one side -> (slope, unchanged)"""
    one = np.ones(n, F)
    if policy == Unchanged:
        return one, True
    if policy == Zero:
        return np.zeros(n, F), False
    if policy == OneToOne or C <= 1:
        return one, False
    with np.errstate(all="ignore"):
        if policy == MeanSlope:
            return ((lO - sO) / (lF - sF)).astype(F), False
        if policy == NearestSlope:
            a, b = (1, 0) if below else (C - 1, C - 2)
            d_obs = np.broadcast_to(_col(ref, a) - _col(ref, b), (n,))
            d_fcst = np.broadcast_to(_col(fcst, a) - _col(fcst, b), (n,))
            return (d_obs / d_fcst).astype(F), False
    raise ValueError("Unknown extrapolation policy")


def apply_curve(fcst, curve_ref, curve_fcst, policy_below, policy_above, **interp_options):
    """curve.cpp:6-133 for an array of inputs (any shape); curves (C,) or fcst.shape + (C,).  An unknown policy raises only where
    some input extrapolates with it, as the scalar reference does."""
    x = _f32(fcst)
    shape = x.shape
    x = x.reshape(-1)
    n = x.shape[0]
    ref, cf = _f32(curve_ref), _f32(curve_fcst)
    if ref.shape != cf.shape:
        raise ValueError("curve_ref and curve_fcst must be the same size")
    if ref.shape[-1] == 0:
        raise ValueError("curve_ref and curve_fcst cannot have size 0")
    if ref.ndim > 1:
        ref, cf = ref.reshape(n, -1), cf.reshape(n, -1)
    C = ref.shape[-1]
    sO, sF = np.broadcast_to(_col(ref, 0), (n,)), np.broadcast_to(_col(cf, 0), (n,))
    lO, lF = np.broadcast_to(_col(ref, C - 1), (n,)), np.broadcast_to(_col(cf, C - 1), (n,))
    with np.errstate(all="ignore"):
        inside = (x >= sF) & (x <= lF)
        out = interpolate(x, cf, ref, **interp_options)
        below = ~inside & (x <= sF)
        above = ~inside & ~below
        for side, is_below, policy, nO, nF in ((below, True, policy_below, sO, sF), (above, False, policy_above, lO, lF)):
            if not side.any():
                continue
            slope, unchanged = _slope(policy, is_below, C, sO, sF, lO, lF, ref, cf, n)
            y = x if unchanged else (nO + slope * (x - nF)).astype(F)
            out[side] = y[side]
    return out.reshape(shape)


def monotonize_curve(curve_ref, curve_fcst):
    """curve.cpp:134-250 -> (curve_ref, curve_fcst); two empty arrays where no pair is valid"""
    ref, fcst = _f32(curve_ref), _f32(curve_fcst)
    if ref.size != fcst.size:
        raise ValueError("curve_ref and curve_fcst must be the same size")
    if ref.size == 0:
        raise ValueError("curve_ref and curve_fcst cannot have size 0")
    keep = valid(ref) & valid(fcst)
    ref, fcst = ref[keep], fcst[keep]
    N = ref.size
    if N == 0:
        return np.zeros(0, F), np.zeros(0, F)
    tol = F(0.1)
    idx = [0]
    prev = x_min = x_max = fcst[0]
    deviation = False
    for i in range(1, N):
        x = fcst[i]
        if deviation:
            if x < x_min:
                x_min = x
            if x > F(x_max + tol):
                while idx and not fcst[idx[-1]] < F(x_min - tol):
                    idx.pop()
                idx.append(i)
                deviation = False
                prev = x_max = x
        elif x <= F(prev + tol):
            deviation = True
            x_min = x
        else:
            idx.append(i)
            prev = x_max = x
    if deviation:   # :227-238: one pop of the LAST entry for every kept point >= x_min met walking down
        for j in range(len(idx) - 1, -1, -1):
            if fcst[idx[j]] >= x_min:
                idx.pop()
    idx = np.asarray(idx, np.int64)
    return ref[idx], fcst[idx]


def quantile_mapping_curve(ref, fcst, quantiles=()):
    """quantile_mapping.cpp:5-46 -> (curve_ref, curve_fcst); with quantiles the index selects from the inputs as given (:41-42)"""
    ref, fcst, q = _f32(ref).ravel(), _f32(fcst).ravel(), _f32(quantiles).ravel()
    if ref.size != fcst.size:
        raise ValueError("ref and fcst must be of the same size")
    if q.size and not np.all(valid(q) & (q <= 1) & (q >= 0)):
        raise ValueError("Quantiles must be >= 0 and <= 1")
    S = ref.size
    if S <= 1:
        return ref.copy(), fcst.copy()
    if q.size == 0:
        return np.sort(ref), np.sort(fcst)
    index = (q * F(S - 1)).astype(np.int64)
    return ref[index], fcst[index]


# ---- the reference's known answers (tests/golden/curve_known_answers.json) and how a case is run and compared ------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "curve_known_answers.json")) as f:
        return json.load(f)


GOLDEN = golden()
CASES = GOLDEN["cases"]
POLICY = GOLDEN["policies"]
EXC = {"ValueError": ValueError, "Exception": Exception}


def policy(p):
    return POLICY[p] if isinstance(p, str) else p


def field(case, key):
    if key + "_arange_shape" in case:
        shape = case[key + "_arange_shape"]
        return np.arange(int(np.prod(shape))).reshape(shape)
    return case[key]


def compare(got, expected, how):
    """the comparison the reference's own test makes"""
    got, expected = np.asarray(got), np.asarray(expected, np.float64)
    if how == "equal":
        np.testing.assert_array_equal(got, expected)
    else:
        decimals = int(how[len("almost"):])
        assert got.shape == expected.shape or got.size == expected.size == 0
        if got.size:
            np.testing.assert_array_almost_equal(got, expected, decimals)


def run_case(case, M):
    """one known-answer case through module M (the restatement, or the library) -> what it returned"""
    fn = case["function"]
    if fn == "apply_curve":
        return M.apply_curve(field(case, "input"), field(case, "curve_ref"), field(case, "curve_fcst"), policy(case["policy_below"]), policy(case["policy_above"]))
    if fn == "interpolate":
        return M.interpolate(case["x"], case["iX"], case["iY"])
    if fn == "quantile_mapping_curve":
        return M.quantile_mapping_curve(case["ref"], case["fcst"], case["quantiles"])
    assert fn == "monotonize_curve"
    return M.monotonize_curve(case["curve_ref"], case["curve_fcst"])


def check_case(case, M):
    import pytest
    if "raises" in case:
        with pytest.raises(EXC[case["raises"]]):
            run_case(case, M)
        return
    got = run_case(case, M)
    if case["compare"] == "runs":
        assert len(got) == 2 and len(got[0]) == len(got[1])
        return
    if "expected" in case:
        compare(got, case["expected"], case["compare"])
    else:
        compare(got[0], case["expected_ref"], case["compare"])
        compare(got[1], case["expected_fcst"], case["compare"])


def needs_device(case):
    """the case runs an array form on real values (a GPU call in the library)"""
    if "raises" in case or case["function"] not in ("apply_curve", "interpolate"):
        return False
    values = case["input"] if case["function"] == "apply_curve" else case["x"]
    return np.ndim(values) > 0 and np.size(values) > 0


# ---- seeded random curves and inputs for the parity tests -------------------------------------------------------------------------
KINDS = ("sorted", "duplicates", "nans", "unsorted", "constant")


def random_curves(rng, shape, nc, kind):
    """(curve_ref, curve_fcst) of shape + (nc,): sorted / sorted with duplicates / with NaNs (ends and inside; now and then an
    infinity) / unsorted / constant curve_fcst"""
    full = tuple(shape) + (nc,)
    f = rng.normal(0, 1, full).astype(np.float32)
    r = rng.normal(0, 1, full).astype(np.float32)
    if kind == "sorted":
        f = np.sort(f, axis=-1)
    elif kind == "duplicates":
        f = np.sort(np.round(f * 2) / 2, axis=-1).astype(np.float32)
    elif kind == "nans":
        f = np.sort(f, axis=-1)
        f[rng.random(full) < 0.2] = np.nan
        r[rng.random(full) < 0.1] = np.nan
        f[rng.random(full) < 0.01] = np.inf
        f[rng.random(full) < 0.01] = -np.inf
    elif kind == "constant":
        f[...] = f[..., :1]
    else:
        assert kind == "unsorted"
    return r, f


def random_inputs(rng, shape, curve_fcst):
    """values around, on and outside the curves, with NaN and both infinities sprinkled in"""
    x = rng.normal(0, 1.3, shape).astype(np.float32)
    nc = curve_fcst.shape[-1]
    pick = rng.integers(0, nc, shape)
    if curve_fcst.ndim == 1:
        on = curve_fcst[pick]
    else:
        on = np.take_along_axis(curve_fcst, pick[..., None], axis=-1)[..., 0]
    hit = rng.random(shape) < 0.15
    x[hit] = on[hit]
    u = rng.random(shape)
    x[u < 0.01] = np.nan
    x[(u >= 0.01) & (u < 0.015)] = np.inf
    x[(u >= 0.015) & (u < 0.02)] = -np.inf
    return x
