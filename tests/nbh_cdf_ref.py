"""numpy restatement of the curve neighbourhood_quantile_fast interpolates in -- the reference's `yarray`
(src/api/neighbourhood.cpp:340-394 for a 2-D field, :453-509 for a cube) -- the yardstick of gridpp_amd.neighbourhood_cdf:

    per threshold t:  temp = float(#valid members <= thresholds[t]) / #valid members     (:455-471; NaN where no member is valid)
                      stats = neighbourhood(temp, halfwidth, Mean)                        (:473, the oracle's)
    per cell:         sum += stats  E times in float32, / E                               (:493-502; 2-D: the value itself, :376-384)
                      clamped to [0, 1]                                                   (:503-508)

and, with tests/curve_ref.interpolate and the two special cases of :514-517, of the quantile itself.  tests/test_nbh_quantiles_api.py
pins the chain to the oracle's neighbourhood_quantile_fast before any GPU run."""
import numpy as np

from tests import curve_ref

F = np.float32


def fractions(field, threshold):
    """:455-471 (2-D: :344-355): the per-cell fraction of valid members at or below the threshold, NaN where no member is valid"""
    f = np.asarray(field, F)
    if f.ndim == 2:
        f = f[:, :, None]
    ok = np.isfinite(f)
    with np.errstate(invalid="ignore"):
        below = (ok & (f <= F(threshold))).sum(axis=2)
    count = ok.sum(axis=2)
    out = np.full(count.shape, np.nan, F)
    m = count > 0
    out[m] = below[m].astype(F) / count[m].astype(F)      # float(sum) / count: the int is promoted to float
    return out


def fold(stats, E):
    """:493-508: the E-fold float32 sum of a plane of means, / E, clamped; NaN stays NaN"""
    stats = np.asarray(stats, F)
    acc = np.zeros(stats.shape, F)
    with np.errstate(invalid="ignore"):
        for _ in range(E):
            acc = (acc + stats).astype(F)
        y = (acc / F(E)).astype(F)
        y = np.where(y > 1, F(1), np.where(y < 0, F(0), y)).astype(F)
    return np.where(np.isfinite(stats), y, F(np.nan)).astype(F)


def cdf(O, field, thresholds, halfwidth):
    """(Y, X, T): the yarray of every cell, for the thresholds as given"""
    field = np.asarray(field, F)
    E = field.shape[2] if field.ndim == 3 else 1
    thresholds = np.asarray(thresholds, F).ravel()
    out = np.empty(field.shape[:2] + (thresholds.size,), F)
    for t, thr in enumerate(thresholds):
        out[:, :, t] = fold(O.neighbourhood(fractions(field, thr), halfwidth, O.Mean), E)
    return out


def quantile_from_cdf(ya, thresholds, q):
    """:513-520 on the columns of `ya` (Y, X, T): NaN where the column holds one, the two special cases, else interpolate()"""
    ya, thresholds, q = np.asarray(ya, F), np.asarray(thresholds, F).ravel(), F(q)
    Y, X, T = ya.shape
    if T == 0:
        return np.full((Y, X), np.nan, F)
    out = curve_ref.interpolate(np.full((Y, X), q, F), ya, np.broadcast_to(thresholds, ya.shape))
    out = np.where((q == 1) & (ya[:, :, 0] == 1), thresholds[0], out)
    out = np.where((q == 0) & (ya[:, :, T - 1] == 0), thresholds[T - 1], out)
    return np.where(np.isnan(ya).any(axis=2), F(np.nan), out).astype(F)
