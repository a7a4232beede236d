"""numpy restatement of gridpp_amd.fractions_skill_score as DESIGN.md 4.22 defines it, the yardstick of the FSS kernels: the per-cell
integers k, m, o and the counting bit, their exact window sums from an int64 summed-area table, the per-cell terms in float64 with the
operations of the definition and no others, and the two totals by math.fsum (the correctly rounded sum, so the only freedom the
library has against it is the order of its own float64 additions)."""
import collections
import math

import numpy as np

Lt, Leq, Gt, Geq = 0, 10, 20, 30
F = np.float32
FssRef = collections.namedtuple("FssRef", ["fss", "fbs", "fbs_worst", "cells"])


def compare(values, threshold, op):
    """`values op threshold` in float32, False where it cannot hold (NaN)"""
    t = F(threshold)
    with np.errstate(invalid="ignore"):
        return {Lt: values < t, Leq: values <= t, Gt: values > t, Geq: values >= t}[op]


def cell_integers(fcst, ref, threshold, op=Gt):
    """step 1 -> k, m, o, c as int64 (Y, X); all four are 0 where the cell does not count"""
    fcst, ref = np.asarray(fcst, F), np.asarray(ref, F)
    cube = fcst if fcst.ndim == 3 else fcst[:, :, None]
    valid = np.isfinite(cube)
    m = valid.sum(axis=2).astype(np.int64)
    k = (valid & compare(cube, threshold, op)).sum(axis=2).astype(np.int64)
    c = np.isfinite(ref) & (m > 0)
    o = (c & compare(ref, threshold, op)).astype(np.int64)
    return np.where(c, k, 0), np.where(c, m, 0), o, c.astype(np.int64)


def box_sum(a, h):
    """step 2: the sum of the int64 plane over [y - h, y + h] x [x - h, x + h] clipped to the grid, exactly"""
    Y, X = a.shape
    sat = np.zeros((Y + 1, X + 1), np.int64)
    sat[1:, 1:] = np.cumsum(np.cumsum(a, axis=0, dtype=np.int64), axis=1, dtype=np.int64)
    y0, y1 = np.maximum(np.arange(Y) - h, 0), np.minimum(np.arange(Y) + h, Y - 1) + 1
    x0, x1 = np.maximum(np.arange(X) - h, 0), np.minimum(np.arange(X) + h, X - 1) + 1
    return sat[y1][:, x1] - sat[y0][:, x1] - sat[y1][:, x0] + sat[y0][:, x0]


def terms(fcst, ref, threshold, h, op=Gt):
    """step 3 -> the float64 terms (Ff - Fo)^2 and Ff^2 + Fo^2 of the contributing cells, in row-major order"""
    k, m, o, c = cell_integers(fcst, ref, threshold, op)
    K, M, O, n = (box_sum(a, h) for a in (k, m, o, c))
    on = n > 0
    Ff = K[on].astype(np.float64) / M[on].astype(np.float64)
    Fo = O[on].astype(np.float64) / n[on].astype(np.float64)
    d = Ff - Fo
    return d * d, Ff * Ff + Fo * Fo


def value(fbs, fbs_worst):
    """step 5"""
    return math.nan if fbs_worst == 0 else 1.0 - fbs / fbs_worst


def fss(fcst, ref, thresholds, halfwidths, op=Gt):
    T, H = len(thresholds), len(halfwidths)
    out = FssRef(np.full((T, H), np.nan), np.zeros((T, H)), np.zeros((T, H)), np.zeros(H, np.int64))
    if np.asarray(fcst).size == 0:
        return out
    for t, th in enumerate(thresholds):
        for j, h in enumerate(halfwidths):
            a, b = terms(fcst, ref, th, int(h), op)
            out.fbs[t, j], out.fbs_worst[t, j] = math.fsum(a), math.fsum(b)
            out.fss[t, j] = value(out.fbs[t, j], out.fbs_worst[t, j])
            out.cells[j] = a.size
    return out
