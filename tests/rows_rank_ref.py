"""numpy restatement of calc_ranks, sort_rows, reorder_by_ranks and calc_crps, one row at a time.

Valid means finite.  Ranks are numpy.argsort(kind="stable") on the valid values of a row (numeric comparison, so -0.0 == +0.0, and equal
values in the order of their positions); the sorted row and the reorder follow from them.  The CRPS comes from the PAIRWISE definition in
float64, (1/N) sum |x_i - y| - (1/(2 N^2)) sum sum |x_i - x_j|, not from the rank form the kernels use: the two share no formula.
tests/test_ranks_api.py holds the argsort ranks to the counting definition and the two CRPS forms to each other."""
import numpy as np

F = np.float32


def ranks(row):
    """int32 ranks of one row; -1 for an invalid value"""
    row = np.asarray(row, F)
    valid = np.isfinite(row)
    out = np.full(row.shape, -1, np.int32)
    order = np.argsort(row[valid], kind="stable")
    r = np.empty(order.size, np.int32)
    r[order] = np.arange(order.size, dtype=np.int32)
    out[valid] = r
    return out


def ranks_by_counting(row):
    """the definition: #{valid j : a[j] < a[i]} + #{valid j < i : a[j] == a[i]}"""
    row = np.asarray(row, F)
    out = np.full(row.shape, -1, np.int32)
    idx = np.flatnonzero(np.isfinite(row))
    v = row[idx]
    for n, i in enumerate(idx):
        out[i] = np.count_nonzero(v < v[n]) + np.count_nonzero(v[:n] == v[n])
    return out


def sorted_row(row):
    """out[rank[i]] = row[i] (its bits), NaN from the number of valid values on"""
    row = np.asarray(row, F)
    r = ranks(row)
    out = np.full(row.shape, np.nan, F)
    out[r[r >= 0]] = row[r >= 0]
    return out


def reorder(values, template):
    """out[i] = sorted_row(values)[ranks(template)[i]]; NaN for a rank of -1 or one that is not below the number of valid values"""
    s, r = sorted_row(values), ranks(template)
    nv = np.count_nonzero(np.isfinite(np.asarray(values, F)))
    out = np.full(s.shape, np.nan, F)
    ok = (r >= 0) & (r < nv)
    out[ok] = s[r[ok]]
    return out


def crps_pairwise(row, y):
    """float64, from the pairwise definition; NaN without a valid member or a finite y"""
    row = np.asarray(row, F)
    x = row[np.isfinite(row)].astype(np.float64)
    if x.size == 0 or not np.isfinite(y):
        return np.nan
    y = np.float64(y)
    pairs = sum(np.abs(x[i:i + 512, None] - x[None, :]).sum() for i in range(0, x.size, 512))   # (512 rows of the N x N table at a time)
    return np.abs(x - y).sum() / x.size - pairs / (2.0 * x.size * x.size)


def crps_rank_form(row, y):
    """float64, (1/N) sum |x_(k) - y| - (1/N^2) sum (2k - N + 1) x_(k) over the sorted valid members"""
    row = np.asarray(row, F)
    x = np.sort(row[np.isfinite(row)].astype(np.float64))
    if x.size == 0 or not np.isfinite(y):
        return np.nan
    n = x.size
    return np.abs(x - np.float64(y)).sum() / n - ((2.0 * np.arange(n) - n + 1) * x).sum() / (float(n) * n)


def crps_slack(row, y):
    """the absolute term of the CRPS tolerance: 8 N 2^-53 (max |x| + |y|), from the row itself"""
    row = np.asarray(row, F)
    x = row[np.isfinite(row)].astype(np.float64)
    if x.size == 0 or not np.isfinite(y):
        return 0.0
    return 8.0 * x.size * 2.0 ** -53 * (np.abs(x).max() + abs(float(y)))


def rows_of(fn, a, *more):
    """fn row by row over the last axis of `a` (and of every array in `more`)"""
    a = np.asarray(a, F)
    flat = a.reshape(-1, a.shape[-1])
    others = [np.asarray(m, F).reshape(-1, a.shape[-1]) for m in more]
    out = [fn(flat[n], *[o[n] for o in others]) for n in range(flat.shape[0])]
    return np.array(out).reshape(a.shape) if out else np.zeros(a.shape, F)


def crps(ens, ref):
    """float64 pairwise CRPS per row, of ref's shape"""
    ens, ref = np.asarray(ens, F), np.asarray(ref, F)
    flat = ens.reshape(-1, ens.shape[-1])
    return np.array([crps_pairwise(flat[n], ref.reshape(-1)[n]) for n in range(flat.shape[0])], np.float64).reshape(ref.shape)


def random_rows(rng, count, maxlen=64):
    """(row, y) pairs: normal, gamma with many tied zeros, small integers with -0.0, scales 1e-3 ... 1e5, 10 % NaN, +-inf"""
    for n in range(count):
        L = int(rng.integers(1, maxlen + 1))
        kind = n % 3
        scale = F(10.0 ** rng.uniform(-3, 5))
        if kind == 0:
            row = (rng.normal(0, 1, L) * scale).astype(F)
        elif kind == 1:
            row = (np.maximum(rng.gamma(0.5, 2, L) - 1, 0) * scale).astype(F)
        else:
            row = rng.integers(-2, 3, L).astype(F)
            row[(row == 0) & (rng.random(L) < 0.5)] = F(-0.0)
        row[rng.random(L) < 0.1] = np.nan
        if n % 7 == 0:
            row[rng.integers(0, L)] = np.inf if n % 2 else -np.inf
        y = F(rng.normal(0, 1) * scale) if kind != 2 else F(rng.integers(-3, 4))
        yield row, y
