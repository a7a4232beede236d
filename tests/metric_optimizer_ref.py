"""Brute-force numpy restatement of get_optimal_threshold and metric_optimizer_curve as DESIGN.md 4.13 defines them: the yardstick of
gridpp_amd/csrc/metric_optimizer.hip.  It is NOT the reference's algorithm (Boost's brent_find_minima on a piecewise-constant function)
but the exact optimum over the plateaus of the score function, which the reference's own known answers satisfy
(tests/test_metric_optimizer_api.py).

No sort, no scan: at every distinct finite value u_k of fcst the table is counted with boolean masks (tests/score_ref.py: counts, the
2**24 cap and the float32 / float64 steps of score.h), then the plateaus are walked in order."""
import numpy as np

from tests import score_ref as S

F, D = np.float32, np.float64
Ets, Ts, Kss, Pc, Bias, Hss = S.METRICS
METRICS = S.METRICS
NEAR_ZERO, AT_BOUNDARY = F(0.0001), F(0.001)   # metric_optimizer.cpp:167,180 as floats


def plateaus(fcst):
    """-> u_0 < ... < u_{m-1}: the distinct finite values of fcst, -0 as +0"""
    f = np.asarray(fcst, dtype=F).ravel()
    return np.unique(f[np.isfinite(f)] + F(0))


def plateau_scores(ref, fcst, threshold, metric):
    """-> (u, s): s[k] = calc_score(ref, fcst, threshold, u[k], metric)"""
    u = plateaus(fcst)
    s = np.array([S.calc_score_vec(ref, fcst, threshold, x, metric) for x in u], dtype=F)
    return u, s


def get_optimal_threshold(ref, fcst, threshold, metric):
    if metric not in METRICS:
        raise ValueError("Unknown metric")
    fcst = np.asarray(fcst, dtype=F).ravel()
    ref = np.asarray(ref, dtype=F).ravel()
    if ref.size < fcst.size:
        raise ValueError("ref and fcst not the same size")
    u, s = plateau_scores(ref, fcst, threshold, metric)
    valid = np.isfinite(s)
    if not valid.any():
        return F(np.nan)
    best = s[valid].max()
    k = int(np.flatnonzero(valid & (s == best))[0])          # the lowest plateau that attains it
    j = k + 1
    while j < len(u) and s[j] == best:                       # (a NaN or an infinite score differs)
        j += 1
    lo, hi = u[k], u[j] if j < len(u) else u[-1]
    x = F((D(lo) + D(hi)) / D(2))
    if hi > lo and not x < hi:
        x = lo
    with np.errstate(invalid="ignore", over="ignore"):
        if best <= NEAR_ZERO:
            return F(np.nan)
        if np.abs(F(best - s[0])) < AT_BOUNDARY or np.abs(F(best - s[-1])) < AT_BOUNDARY:
            return F(np.nan)
    return F(x)


def metric_optimizer_curve(ref, fcst, thresholds, metric):
    """-> (curve_ref, curve_fcst), the reference's naming (metric_optimizer.cpp:119-126)"""
    if metric not in METRICS:
        raise ValueError("Unknown metric")
    if np.size(ref) != np.size(fcst):
        raise ValueError("ref and fcst not the same size")
    curve_ref, curve_fcst = [], []
    for t in np.asarray(thresholds, dtype=F).ravel():
        x = get_optimal_threshold(ref, fcst, t, metric)
        if np.isfinite(x):
            curve_ref.append(x)
            curve_fcst.append(t)
    return np.array(curve_ref, dtype=F), np.array(curve_fcst, dtype=F)


def same_bits(got, want):
    S.same_bits(np.atleast_1d(np.asarray(got, dtype=F)), np.atleast_1d(np.asarray(want, dtype=F)))


# ---- the data of the GPU parity cases (tests/test_gpu_metric_optimizer_parity.py) ---------------------------------------------------
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1025)
THRESHOLDS = (0.5, 2.0, 4.0)


def case(n, halves, seed):
    """ref = gamma(1, 2), fcst = ref * U(0.5, 1.5) + N(0, 0.5); halves: fcst rounded to halves (heavy ties)"""
    rng = np.random.default_rng(seed)
    ref = rng.gamma(1.0, 2.0, n).astype(F)
    fcst = (ref * rng.uniform(0.5, 1.5, n) + rng.normal(0, 0.5, n)).astype(F)
    if halves:
        fcst = (np.round(fcst * 2) / 2).astype(F)
    return ref, fcst
