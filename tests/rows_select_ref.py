"""The result contract of calc_quantile on rows, restated in numpy float32 (no test here: tests/test_rows_select_restatement.py checks
this file against the CPU oracle, tests/test_gpu_rows_select.py checks the GPU paths against it).

Valid means finite.  The order is the order of the f2ord keys (gridpp_amd/csrc/row_stats.h), so -0.0 ranks below +0.0.  The two order
statistics and the weight are those of quantile_from_order, every step rounded to float32.  q == 0 and q == 1 are the positional
Min / Max of row_statistic: the first valid value, replaced on a strict compare only (the lowest index wins among equals, the sign of a
zero included).  NaN q, or no valid value -> NaN."""
import numpy as np

F = np.float32


def f2ord(x):
    """monotone map float32 -> uint32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def quantile(row, q):
    row = np.ascontiguousarray(row, np.float32).ravel()
    q = F(q)
    v = row[np.isfinite(row)]
    N = v.size
    if np.isnan(q) or N == 0:
        return F(np.nan)
    if q == 0 or q == 1:
        m = v[0]
        for x in v[1:]:
            if (x < m) if q == 0 else (x > m):
                m = x
        return F(m)
    s = v[np.argsort(f2ord(v), kind="stable")]
    pos = q * F(N - 1)
    lo, up = int(np.floor(pos)), int(np.ceil(pos))
    if lo == up:
        return F(s[lo])
    with np.errstate(over="ignore", invalid="ignore"):
        lq, uq = F(lo) / F(N - 1), F(up) / F(N - 1)
        f = (q - lq) / (uq - lq)
        return F(s[lo] + (s[up] - s[lo]) * f)


def rows_quantile(a, q):
    """a: (R, L); q: a scalar or R levels -> R float32 values"""
    a = np.asarray(a, np.float32)
    qs = np.broadcast_to(np.asarray(q, np.float32).ravel(), (a.shape[0],)) if np.ndim(q) else [q] * a.shape[0]
    return np.array([quantile(r, x) for r, x in zip(a, qs)], np.float32)


def adversarial(L):
    """rows of length L that stress a selection by keys: see the names"""
    i = np.arange(L)
    out = {
        "constant": np.full(L, 3.5, np.float32),
        "zeros": np.where(i * 7 % 3 == 0, F(-0.0), F(0.0)).astype(np.float32),
        "one_valid": np.where(i == L // 2, F(2.5), F(np.nan)).astype(np.float32),
        "low_byte": (np.uint32(0x40400000) + (i * 37 % 256).astype(np.uint32)).view(np.float32),
        "high_byte": (((i * 53 % 256).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00123456)).view(np.float32),
        "denormals": ((((i * 97 + 1) & 0x7FFFFF).astype(np.uint32)) | ((i % 2).astype(np.uint32) << np.uint32(31))).view(np.float32),
        "flt_max": np.where(i % 2 == 0, np.finfo(np.float32).max, -np.finfo(np.float32).max).astype(np.float32),
        "negative": (-(1 + i * 0.37)).astype(np.float32),
        "descending": (1000 - i * 0.5).astype(np.float32),
    }
    return np.stack(list(out.values()))
