"""numpy restatement of the reference's gridpp::calc_score (src/api/metric_optimizer.cpp:185-244) and gridpp::neighbourhood_score
(src/api/neighbourhood_score.cpp:6-60), the yardstick of the score kernels.

calc_score_table follows the reference operation for operation with np.float32 / np.float64 values: every `/ 1.0`, `* 1.0` and `2.0 *`
lifts that operation to double, sums such as a + b + c stay float, the result is rounded to float once.  It takes scalars or arrays.
calc_score_vec counts as the reference does (a NaN ref nowhere, a NaN fcst as c or d) and stops every count at 2**24, where the
reference's `float x++` stops growing.  neighbourhood_score is composed from pieces that other tests already pin to the reference:
oracle.gridding_nearest, oracle.neighbourhood(..., Mean) on the four planes of zeros and ones, then calc_score_table per cell.

tests/test_score_restatement.py pins calc_score to the reference's own known answers (tests/golden/score_known_answers.json); the
reference has no test of neighbourhood_score, so that parity rests on this composition."""
import json
import os

import numpy as np

Ets, Ts, Kss, Pc, Bias, Hss = 0, 1, 20, 30, 40, 50
METRICS = (Ets, Ts, Kss, Pc, Bias, Hss)
Mean = 0
F, D = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def calc_score_table(a, b, c, d, metric):
    """metric_optimizer.cpp:207-244; scalars -> np.float32, arrays -> float32 array"""
    a, b, c, d = (np.asarray(v, dtype=F) for v in (a, b, c, d))
    nan, one = F(np.nan), F(1)
    with np.errstate(all="ignore"):
        if metric == Ets:                                                   # :208-214
            N = a + b + c + d
            ar = ((a + b).astype(D) / D(1.0) / N.astype(D) * (a + c).astype(D)).astype(F)
            den = a + b + c - ar
            value = ((a - ar).astype(D) / D(1.0) / den.astype(D)).astype(F)
            out = np.where(den == 0, nan, value)
        elif metric == Ts:                                                  # :215-218
            out = (a.astype(D) / D(1.0) / (a + b + c).astype(D)).astype(F)
        elif metric == Pc:                                                  # :219-222
            N = a + b + c + d
            out = (a + d) / N
        elif metric == Kss:                                                 # :223-227
            den = (a + c) * (b + d)
            value = ((a * d - b * c).astype(D) * D(1.0) / den.astype(D)).astype(F)
            out = np.where(den == 0, nan, value)
        elif metric == Bias:                                                # :228-234
            out = np.where(b == c, one, one - np.abs(b - c) / (b + c))
        elif metric == Hss:                                                 # :235-240
            den = (a + c) * (c + d) + (a + b) * (b + d)
            value = (D(2.0) * (a * d - b * c).astype(D) / den.astype(D)).astype(F)
            out = np.where(den == 0, nan, value)
        else:
            raise ValueError("Unknown metric")                              # :241-243
    out = np.asarray(out, dtype=F)
    return out[()] if out.ndim == 0 else out


def counts(ref, fcst, threshold, fthreshold):
    """metric_optimizer.cpp:189-204 over the first len(fcst) elements -> the four integer counts"""
    fcst = np.asarray(fcst, dtype=F).ravel()
    ref = np.asarray(ref, dtype=F).ravel()
    if ref.size < fcst.size:
        raise ValueError("ref and fcst not the same size")   # (the reference reads out of bounds)
    ref = ref[:fcst.size]
    with np.errstate(invalid="ignore"):
        hit, above, below = fcst > F(fthreshold), ref > F(threshold), ref <= F(threshold)
    return (int(np.sum(hit & above)), int(np.sum(hit & below)), int(np.sum(~hit & above)), int(np.sum(~hit & below)))


def score_of_counts(n, metric):
    t = [F(min(int(v), 1 << 24)) for v in n]   # `float x++` stops at 2^24
    return calc_score_table(t[0], t[1], t[2], t[3], metric)


def calc_score_vec(ref, fcst, threshold, fthreshold, metric):
    return score_of_counts(counts(ref, fcst, threshold, fthreshold), metric)


def calc_score(*args):
    """the three overloads, told apart as the library's python mirror does"""
    if len(args) == 5 and np.ndim(args[0]) == 0:
        return calc_score_table(*args)
    if len(args) == 4:
        return calc_score_vec(args[0], args[1], args[2], args[2], args[3])
    return calc_score_vec(*args)


def planes(ref_grid, fcst, threshold):
    """neighbourhood_score.cpp:19-42 -> the planes a, b, c, d (float32 zeros and ones)"""
    ref_grid, fcst, t = np.asarray(ref_grid, dtype=F), np.asarray(fcst, dtype=F), F(threshold)
    ok = np.isfinite(ref_grid) & np.isfinite(fcst)
    with np.errstate(invalid="ignore"):
        hit, above, below = fcst > t, ref_grid > t, ref_grid <= t
    return [(ok & m).astype(F) for m in (hit & above, hit & below, ~hit & above, ~hit & below)]


def gridded(og, op, ref, shape):
    """:25 -> ref_grid; og / op are oracle point sets (oracle.Pts)"""
    from oracle import oracle as O
    return O.gridding_nearest(og, op, ref, 1, Mean).reshape(shape)


def hoods(og, op, fcst, ref, half_width, threshold, ref_grid=None):
    """:25-48 -> the four neighbourhood means of fcst (Y, X); ref_grid: gridded(...) of an earlier call with the same observations"""
    from oracle import oracle as O
    fcst = np.asarray(fcst, dtype=F)
    if ref_grid is None:
        ref_grid = gridded(og, op, ref, fcst.shape)
    return [O.neighbourhood(p, half_width, Mean) for p in planes(ref_grid, fcst, threshold)]


def neighbourhood_score(og, op, fcst, ref, half_width, metric, threshold):
    """neighbourhood_score.cpp:6-60 with its checks in order"""
    fcst = np.asarray(fcst, dtype=F)
    if fcst.ndim != 2 or fcst.size != og.n:
        raise ValueError("Grid size is not the same as forecast values")
    if half_width <= 0:
        raise ValueError("half_width must be greater than 0")
    if metric not in METRICS:
        raise ValueError("Unknown metric")
    if np.size(ref) != op.n:
        raise ValueError("Points size is not the same as values")
    a, b, c, d = hoods(og, op, fcst, ref, half_width, threshold)
    return calc_score_table(a, b, c, d, metric)


def same_bits(got, want):
    """bit for bit, NaN positions included (any NaN payload)"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    np.testing.assert_array_equal(got.view(np.uint32)[keep], want.view(np.uint32)[keep])


# ---- the reference's known answers (tests/golden/score_known_answers.json) --------------------------------------------------------
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "score_known_answers.json")) as f:
        return json.load(f)


GOLDEN = golden()
METRIC = GOLDEN["metrics"]          # name -> value
KNOWN = GOLDEN["calc_score"]        # obs, fcst, thresholds, expected[metric name] = one value per threshold (None = NaN)

# guard branches worked by hand: (a, b, c, d, metric name, expected or None for NaN)
GUARDS = [
    (5, 0, 0, 7, "Ets", 1.0),       # b = c = 0: ar = 5 / 12 * 5 rounded to float, a + b + c - ar = a - ar != 0 -> (a - ar) / (a - ar) = 1
    (5, 0, 0, 0, "Ets", None),      # b = c = d = 0: ar = 5 / 5 * 5 = a, the guard holds
    (0, 0, 0, 7, "Ets", None),      # a = b = c = 0: ar = 0, the guard holds
    (0, 3, 0, 4, "Kss", None),      # a + c = 0: an empty column
    (3, 0, 4, 0, "Kss", None),      # b + d = 0
    (0, 0, 0, 0, "Hss", None),      # denom = 0
    (0, 0, 0, 0, "Bias", 1.0),      # b == c, even when everything is 0
    (4, 2, 2, 9, "Bias", 1.0),
    (0, 0, 0, 0, "Ts", None),       # 0 / 0
    (0, 0, 0, 0, "Pc", None),
    (0, 0, 0, 0, "Ets", None),
    (0, 0, 0, 0, "Kss", None),
]


# ---- the geometry and contents of the GPU parity cases (tests/test_gpu_score_parity.py) ----------------------------------------------
OBS_SETS = ("none", "one", "tenth", "several", "one_cell", "sprinkled", "at_threshold", "above", "below")
THRESHOLD = 0.5


def geometry(Y, X, geodetic):
    """-> lats, lons (Y, X) float32: a regular grid, degrees or metres"""
    if geodetic:
        lats, lons = np.meshgrid(60 + 0.01 * np.arange(Y), 10 + 0.02 * np.arange(X), indexing="ij")
    else:
        lats, lons = np.meshgrid(1000.0 * np.arange(Y), 1000.0 * np.arange(X), indexing="ij")
    return lats.astype(F), lons.astype(F)


def case_inputs(Y, X, geodetic, obs, seed):
    """-> lats, lons, plat, plon, ref (S,), fcst (Y, X): one parity case"""
    rng = np.random.default_rng(seed)
    lats, lons = geometry(Y, X, geodetic)
    C = Y * X
    S = {"none": 0, "one": 1, "tenth": max(1, C // 10), "several": 3 * C, "one_cell": 40}.get(obs, max(1, C // 3))
    dy, dx = (0.01, 0.02) if geodetic else (1000.0, 1000.0)
    y0, x0 = (60.0, 10.0) if geodetic else (0.0, 0.0)
    if obs == "one_cell":
        cy, cx = rng.integers(0, Y), rng.integers(0, X)
        py, px = cy + rng.uniform(-0.3, 0.3, S), cx + rng.uniform(-0.3, 0.3, S)
    else:
        py, px = rng.uniform(-0.7, Y - 0.3, S), rng.uniform(-0.7, X - 0.3, S)   # a little beyond the edges too
    plat, plon = (y0 + dy * py).astype(F), (x0 + dx * px).astype(F)
    ref = rng.random(S).astype(F)
    fcst = rng.random((Y, X)).astype(F)
    if obs == "several":      # the means of a cell's observations straddle the threshold closely
        ref = (THRESHOLD + rng.uniform(-0.01, 0.01, S)).astype(F)
    elif obs == "sprinkled":
        for arr in (ref, fcst.reshape(-1)):
            u = rng.random(arr.size)
            arr[u < 0.10] = np.nan
            arr[(u >= 0.10) & (u < 0.14)] = np.inf
            arr[(u >= 0.14) & (u < 0.18)] = -np.inf
    elif obs == "at_threshold":
        ref[rng.random(S) < 0.4] = THRESHOLD
        fcst[rng.random((Y, X)) < 0.4] = THRESHOLD
    elif obs == "above":      # only a: b + d = 0, the guards of Kss and Hss
        ref, fcst = ref + F(1), fcst + F(1)
    elif obs == "below":      # only d
        ref, fcst = ref - F(1), fcst - F(1)
    return lats, lons, plat, plon, ref, fcst
