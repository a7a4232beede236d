"""The yardstick of neighbourhood_members / calc_gradient_members: a numpy restatement in float64 of the window statistics of
every plane of a (Y, X, E) cube -- window sum, count, min and max over the valid values -- and of the two gradients built on them, plus the
data the bit tests use.

exact_cube(): multiples of 1/8 with |v| <= 64.  Every float32 square and every base * value product (multiples of 1/64 up to 4096) is exact,
every partial sum is exact in double (so every summation order gives the same sum), and the quotient s / n of such sums is at least
1 / (8 n 2^25) (relative) away from every float32 rounding boundary, far more than a few ulp(double): any quotient within a few ulp(double)
rounds to the same float32 (checked on the CPU by tests/test_members_api.py::test_exact_means_are_far_from_rounding_boundaries)."""
import numpy as np

F = np.float32
SHAPES = [(37, 29, 5), (9, 70, 3), (130, 3, 1), (5, 4, 65), (33, 65, 50)]
HALFWIDTHS = [0, 1, 7, 15, 16, 17, 40]


def holes(f, rng, inf=True):
    """a NaN block, 3 % sprinkled NaN, a block missing in every member, one +-Inf, one member that is entirely NaN (where there are several)"""
    Y, X, E = f.shape
    f[Y // 4:Y // 4 + max(1, Y // 5), X // 5:X // 5 + max(1, X // 2), : max(1, E // 2)] = np.nan
    f[rng.random(f.shape) < 0.03] = np.nan
    f[Y // 2:Y // 2 + max(1, Y // 6), X // 2:X // 2 + max(1, X // 6), :] = np.nan
    if inf:
        f[Y - 1, X - 1, E - 1] = np.inf
        f[0, X // 2, 0] = -np.inf
    if E > 1:
        f[:, :, E // 2] = np.nan
    return f


def exact_cube(seed, shape, missing=True):
    rng = np.random.default_rng(seed)
    f = (rng.integers(-512, 513, shape) / 8).astype(F)
    return holes(f, rng) if missing else f


def general_cube(seed, shape):
    """field()'s recipe of tests/test_gpu_neighbourhood_parity.py, uniform(0, 10), with the holes above"""
    rng = np.random.default_rng(seed)
    return holes(rng.uniform(0, 10, shape).astype(F), rng)


def valid(a):
    return np.isfinite(a)


def _box(a, hw, axis):
    """sum over the window [i - hw, i + hw] clipped to the axis"""
    n = a.shape[axis]
    c = np.concatenate([np.zeros_like(np.take(a, [0], axis)), np.cumsum(a, axis)], axis)
    i = np.arange(n)
    return np.take(c, np.minimum(n, i + hw + 1), axis) - np.take(c, np.maximum(0, i - hw), axis)


def _select(a, hw, axis, pick):
    """pick (np.fmin / np.fmax: NaN only where both are) over the window clipped to the axis, by direct shifts"""
    n = a.shape[axis]
    out = np.full(a.shape, np.nan)
    a = np.moveaxis(a, axis, 0)
    o = np.moveaxis(out, axis, 0)
    for d in range(-min(hw, n - 1), min(hw, n - 1) + 1):
        lo, hi = max(0, -d), min(n, n - d)
        o[lo:hi] = pick(o[lo:hi], a[lo + d:hi + d])
    return out


def window_stats(a, hw):
    """a: a plane (Y, X) or a cube (Y, X, E), windows along the first two axes of every member.
    -> (sum float64, count int64, min float64, max float64) over the valid values; min / max are NaN where count == 0"""
    a = np.asarray(a, np.float64)
    ok = valid(a)
    z = np.where(ok, a, 0.0)
    s = _box(_box(z, hw, 0), hw, 1)
    n = np.rint(_box(_box(ok.astype(np.float64), hw, 0), hw, 1)).astype(np.int64)
    m = np.where(ok, a, np.nan)
    with np.errstate(invalid="ignore"):
        lo = _select(_select(m, hw, 0, np.fmin), hw, 1, np.fmin)
        hi = _select(_select(m, hw, 0, np.fmax), hw, 1, np.fmax)
    return s, n, lo, hi


def expected(a, hw, statistic_name):
    """float32 result of Mean / Sum / Count / Min / Max: Mean = float32(float64 sum / count)"""
    s, n, lo, hi = window_stats(a, hw)
    with np.errstate(invalid="ignore", divide="ignore"):
        if statistic_name == "Mean":
            return np.where(n > 0, s / np.maximum(n, 1), np.nan).astype(F)
        if statistic_name == "Sum":
            return np.where(n > 0, s, np.nan).astype(F)
        if statistic_name == "Count":
            return n.astype(F)
        return {"Min": lo, "Max": hi}[statistic_name].astype(F)


def mean_of_squares(a, hw):
    """E[x^2] over the window in float64 (the scale of the variance bounds)"""
    a = np.asarray(a, np.float64)
    s, n, _, _ = window_stats(np.where(valid(a), a * a, np.nan), hw)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, s / np.maximum(n, 1), np.nan)


def variance(a, hw):
    """E[x^2] - E[x]^2 in float64"""
    s, n, _, _ = window_stats(a, hw)
    with np.errstate(invalid="ignore", divide="ignore"):
        return mean_of_squares(a, hw) - np.where(n > 0, s / np.maximum(n, 1), np.nan) ** 2


def gradient_linear(base, values, hw, num_min, min_range, default_gradient):
    """calc_gradient.cpp:79-124 in float64 for one plane (or a cube with a base of the same shape): the slope of values against base over the
    cells where both are valid"""
    base, values = np.asarray(base, np.float64), np.asarray(values, np.float64)
    good = valid(base) & valid(values)

    def mean(a):
        s, n, _, _ = window_stats(np.where(good, a, np.nan), hw)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, s / np.maximum(n, 1), np.nan), n
    mx, n = mean(base)
    my, mxx, mxy = mean(values)[0], mean(base * base)[0], mean(base * values)[0]
    var = mxx - mx * mx
    with np.errstate(invalid="ignore", divide="ignore"):
        use = (n >= num_min) & (n > 0) & (var != 0)
        if np.isfinite(min_range):
            use &= np.sqrt(np.maximum(var, 0)) >= min_range
        return np.where(use, (mxy - mx * my) / np.where(use, var, 1.0), default_gradient)


def gradient_minmax(base, values, hw, num_min, min_range, default_gradient):
    """calc_gradient.cpp:26-74 for one plane in float32: the walk in row-major order, strict > / <"""
    base, values = np.asarray(base, F), np.asarray(values, F)
    Y, X = base.shape
    out = np.full((Y, X), default_gradient, F)
    good = valid(base) & valid(values)
    for y in range(Y):
        for x in range(X):
            ya, yb, xa, xb = max(0, y - hw), min(Y, y + hw + 1), max(0, x - hw), min(X, x + hw + 1)
            g = good[ya:yb, xa:xb].ravel()
            if not g.any():
                continue
            b, v = base[ya:yb, xa:xb].ravel()[g], values[ya:yb, xa:xb].ravel()[g]
            imax, imin = int(np.argmax(b)), int(np.argmin(b))      # the first of equal ones, as strict comparisons keep it
            if b.size < num_min or abs(b[imax] - b[imin]) <= min_range:    # (a NaN min_range compares false, as in the reference)
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                out[y, x] = (v[imax] - v[imin]) / (b[imax] - b[imin])
    return out


def per_plane(fn, cube, *args):
    """fn(plane e, *args) of every member, stacked into a cube"""
    return np.stack([np.asarray(fn(np.ascontiguousarray(cube[:, :, e]), *args)) for e in range(cube.shape[2])], -1)
