"""float32 numpy restatement of the reference's gridpp::window (src/api/window.cpp:6-156) with calc_statistic / calc_quantile
(src/api/util.cpp:16-178), the yardstick of the window kernels.

Sequential along the time axis like the reference -- a python loop over the T columns, vectorised over the rows -- and every
operation in float32 in the reference's order.  That order is the point: Mean / Sum / Count are differences of a sequential
float32 prefix sum (window.cpp:33-111), which is NOT the exact window sum (tests/test_window_restatement.py measures how far it
strays), so an implementation has to add in this order to agree with the reference.  tests/test_window_restatement.py pins the
restatement to the reference's own known answers.

counts[start - 1] with start == 0 is one element before the reference's vector (window.cpp:83,88,92); its tests pin the value 0
there, and 0 is what this restatement and the library use (N[-1] = 0, P[-1] = 0)."""
import json
import os

import numpy as np

Mean, Min, Median, Max, Quantile, Std, Variance, Sum, Count, RandomChoice, Unknown = 0, 10, 20, 30, 40, 50, 60, 70, 80, 90, -1
SCAN = (Mean, Sum, Count)
GATHER = (Min, Max, Median, Std, Variance, RandomChoice)
F = np.float32


def valid(v):   # util.cpp:16-18
    return np.isfinite(v)


def bounds(x, T, length, before):
    """-> (start, end, outside): the clipped window of column x (window.cpp:61-69,118-133)"""
    if before:
        start, end = x - length + 1, x
    else:
        start, end = x - length // 2, x + length // 2
    outside = start < 0 or end > T - 1
    return max(start, 0), min(end, T - 1), outside


def prefix(a):
    """window.cpp:34-54 -> (P, N): the sequential float32 prefix sum over the valid values of every row and their count; an invalid
    value repeats its predecessor, an invalid value at x = 0 leaves 0"""
    Y, T = a.shape
    ok = valid(a)
    clean = np.where(ok, a, F(0))
    P, N = np.zeros((Y, T), np.float32), np.zeros((Y, T), np.int64)
    p, n = np.zeros(Y, np.float32), np.zeros(Y, np.int64)
    for x in range(T):
        p = np.where(ok[:, x], p + clean[:, x], p)   # :46 / :50 (at x = 0: :40 -- 0 + v is v)
        n = n + ok[:, x]                             # :47 / :51
        P[:, x], N[:, x] = p, n
    return P, N


def _scan(a, length, statistic, before, keep_missing, missing_edges):
    Y, T = a.shape
    P, N = prefix(a)
    out = np.full((Y, T), np.nan, np.float32)
    for x in range(T):
        start, end, _ = bounds(x, T, length, before)
        n_end = N[:, end]
        n = n_end - (N[:, start - 1] if start >= 1 else 0)   # counts[-1] = 0 (see the module's docstring)
        if start >= 1:
            v = np.where(n != 0, P[:, end] - P[:, start - 1], F(np.nan))   # :71-75
        else:
            v = np.where(n_end != 0, P[:, end], F(np.nan))                 # :76-80
        v = v.astype(np.float32)
        if statistic == Count:                                             # :82-84: whatever keep_missing / missing_edges say
            out[:, x] = n.astype(np.float32)
            continue
        if statistic == Mean:                                              # :86-90
            with np.errstate(divide="ignore", invalid="ignore"):
                v = np.where(n_end != 0, v / n.astype(np.float32), v).astype(np.float32)
        if keep_missing:                                                   # :91-95
            v = np.where(n < end - start + 1, F(np.nan), v)
        if missing_edges:                                                  # :97-108
            if before:
                if x < length - 1:
                    v = np.full(Y, np.nan, np.float32)
            elif x < length // 2 or x + length // 2 + 1 > T:
                v = np.full(Y, np.nan, np.float32)
        out[:, x] = v
    return out


def calc_statistic(W, statistic):
    """util.cpp:19-178 on every row of W (rows x n), sequential in column order"""
    Y, n = W.shape
    ok = valid(W)
    nan = np.full(Y, np.nan, np.float32)
    if statistic in (Min, Max):   # calc_quantile with 0 / 1 (:121-146)
        m = nan.copy()
        for i in range(n):
            v = W[:, i]
            first = ok[:, i] & ~valid(m)
            better = ok[:, i] & valid(m) & ((v < m) if statistic == Min else (v > m))
            m = np.where(first | better, v, m)
        return m
    if statistic in (Std, Variance):   # :40-74
        total, total2, K = np.zeros(Y, np.float32), np.zeros(Y, np.float32), nan.copy()
        count = np.zeros(Y, np.int64)
        for i in range(n):
            v = np.where(ok[:, i], W[:, i], F(0))
            K = np.where(ok[:, i] & ~valid(K), v, K)
            with np.errstate(invalid="ignore"):
                d = (v - K).astype(np.float32)
                total = np.where(ok[:, i], total + d, total)
                total2 = np.where(ok[:, i], total2 + d * d, total2)
            count = count + ok[:, i]
        with np.errstate(divide="ignore", invalid="ignore"):
            c = count.astype(np.float32)
            mean, mean2 = total / c, total2 / c
            var = mean2 - mean * mean
            var = np.where(var < 0, F(0), var)
            value = np.sqrt(var) if statistic == Std else var
        return np.where(count > 0, value, F(np.nan)).astype(np.float32)
    if statistic == Median:   # calc_quantile with 0.5 (:147-177)
        S = np.sort(np.where(ok, W, F(np.inf)), axis=1)   # the valid values first, in order
        N = ok.sum(axis=1)
        q = F(0.5)
        Nm1 = np.maximum(N - 1, 0).astype(np.float32)
        pos = q * Nm1
        li, ui = np.floor(pos).astype(np.int64), np.ceil(pos).astype(np.int64)
        rows = np.arange(Y)
        lv, uv = S[rows, li], S[rows, ui]
        with np.errstate(divide="ignore", invalid="ignore"):
            lq, uq = li.astype(np.float32) / Nm1, ui.astype(np.float32) / Nm1
            f = (q - lq) / (uq - lq)
            between = lv + (uv - lv) * f
        value = np.where(li == ui, lv, between)
        return np.where(N > 0, value, F(np.nan)).astype(np.float32)
    raise RuntimeError("Internal error. Cannot compute statistic")   # :106 (Quantile, Unknown); RandomChoice has no one answer


def gather_missing(a, length, before, keep_missing, missing_edges):
    """where window.cpp:144-147 put NaN whatever the statistic -> bool (Y, T)"""
    Y, T = a.shape
    bad = ~valid(a)
    out = np.zeros((Y, T), bool)
    for x in range(T):
        start, end, outside = bounds(x, T, length, before)
        if keep_missing:
            out[:, x] = bad[:, start:end + 1].any(axis=1)
        if missing_edges and outside:
            out[:, x] = True
    return out


def _gather(a, length, statistic, before, keep_missing, missing_edges):
    """window.cpp:112-152.  The windows of all columns go through calc_statistic together: window x is padded behind its last
    value with NaN up to the longest window, which calc_statistic skips like any invalid value, so every row still sees its values
    one after the other in column order."""
    Y, T = a.shape
    spans = [bounds(x, T, length, before) for x in range(T)]
    start = np.array([s for s, _, _ in spans])
    n = np.array([e - s + 1 for s, e, _ in spans])
    i = np.arange(n.max())
    inside = i[None, :] < n[:, None]                                  # (T, longest window)
    col = np.minimum(start[:, None] + i[None, :], T - 1)
    W = np.where(inside[None, :, :], a[:, col], F(np.nan))            # :136-142 for every x
    value = calc_statistic(W.reshape(Y * T, -1), statistic).reshape(Y, T)
    forced = gather_missing(a, length, before, keep_missing, missing_edges)
    return np.where(forced, F(np.nan), value).astype(np.float32)      # :144-151


def window(array, length, statistic, before=False, keep_missing=False, missing_edges=True):
    """window.cpp:6-156, the checks in its order"""
    if length <= 0:                                    # :10-12
        raise ValueError("Length variable must be > 0")
    a = np.asarray(array, dtype=np.float32)
    if a.ndim != 2:
        a = a.reshape((0, 0))
    Y, T = a.shape
    if Y == 0:                                         # :14-17
        return np.zeros((0, 0), np.float32)
    if T == 0:                                         # :19-22
        return np.zeros((Y, 0), np.float32)
    if length % 2 == 0 and not before:                 # :26-28
        raise ValueError("Length variable must be an odd number")
    if statistic in SCAN:
        return _scan(a, length, statistic, before, keep_missing, missing_edges)
    return _gather(a, length, statistic, before, keep_missing, missing_edges)


def check_random_choice(got, array, length, before, keep_missing, missing_edges):
    """RandomChoice has no one answer (util.cpp:75-96 draws with rand()): every output is a valid member of its clipped window, and
    NaN exactly where the rules put NaN (keep_missing / missing_edges) or the window holds no valid value"""
    a = np.asarray(array, dtype=np.float32)
    got = np.asarray(got)
    Y, T = a.shape
    assert got.shape == (Y, T) and got.dtype == np.float32
    forced = gather_missing(a, length, before, keep_missing, missing_edges)
    for x in range(T):
        start, end, _ = bounds(x, T, length, before)
        W = a[:, start:end + 1]
        want_nan = forced[:, x] | ~valid(W).any(axis=1)
        np.testing.assert_array_equal(np.isnan(got[:, x]), want_nan, err_msg="column %d" % x)
        member = ((W == got[:, x:x + 1]) & valid(W)).any(axis=1)
        assert np.all(member | want_nan), "column %d: a value that is no valid member of its window" % x


def same_bits(got, want):
    """bit for bit, NaN positions included (any NaN payload)"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    np.testing.assert_array_equal(got.view(np.uint32)[keep], want.view(np.uint32)[keep])


# ---- the reference's known answers (tests/golden/window_known_answers.json) and how a case is run and compared ---------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nan(o):
    if o is None:
        return np.nan
    if isinstance(o, list):
        return [_nan(v) for v in o]
    return o


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "window_known_answers.json")) as f:
        return json.load(f)


GOLDEN = golden()
CASES = GOLDEN["cases"]
STATISTIC = GOLDEN["statistics"]
EXC = {"ValueError": ValueError}


def case_array(case):
    if "array_zeros_shape" in case:
        return np.zeros(case["array_zeros_shape"])
    return np.array(_nan(case["array"]), dtype=np.float64)   # (float64, as the reference's test passes it)


def run_case(case, M):
    """one known-answer case through module M (this restatement, or the library) -> what it returned"""
    return M.window(case_array(case), case["length"], STATISTIC[case["statistic"]], case["before"], case["keep_missing"], case["missing_edges"])


def check_case(case, M):
    import pytest
    if "raises" in case:
        with pytest.raises(EXC[case["raises"]]):
            run_case(case, M)
        return
    got = np.asarray(run_case(case, M))
    if "expected_shape" in case:
        assert got.shape == tuple(case["expected_shape"])
        return
    np.testing.assert_array_equal(got, np.array(_nan(case["expected"]), dtype=np.float64))   # the reference's comparison


def needs_device(case):
    """the case reaches a kernel in the library: a non-empty array and no exception before it"""
    return "raises" not in case and "expected_shape" not in case
