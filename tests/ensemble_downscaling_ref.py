"""downscale_probability, mask_threshold_downscale_consensus / _quantile and smart restated in numpy float32 over the oracle
(the reference's structure: src/api/downscale_probability.cpp:20-63, mask_threshold_downscale_consensus.cpp:19-82,
smart.cpp:12-66):

    nearest input cell per output cell   oracle.nearest_indices (exact metric, ties -> lowest index)
    valid                                not NaN, not +-inf
    probability                          (valid members with member OP threshold) / (valid members), NaN if none
    masked[k]                            NaN where threshold_values[k] is not valid, ivalues_true[k] where
                                         threshold_values[k] OP threshold, else ivalues_false[k]
    mask_*                               oracle.calc_statistic(masked) / oracle.calc_quantile(masked, q)
    smart                                candidates oracle.get_neighbours(R), rho = Struct.corr; the min(num, n) of largest
                                         rho (ties -> lower flat index); float32 sum / count

The known answers (tests/golden/ensemble_downscaling_known_answers.json) pin the first three; the GPU tests compare the
kernels with all four."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
Lt, Leq, Gt, Geq = 0, 10, 20, 30
Mean, Min, Median, Max, Quantile, Std, Variance, Sum, Count, RandomChoice = 0, 10, 20, 30, 40, 50, 60, 70, 80, 90
OPS = {Lt: np.less, Leq: np.less_equal, Gt: np.greater, Geq: np.greater_equal}
OP_NAMES = dict(Lt=Lt, Leq=Leq, Gt=Gt, Geq=Geq)
STAT_NAMES = dict(Mean=Mean, Min=Min, Median=Median, Max=Max, Quantile=Quantile, Std=Std, Variance=Variance, Sum=Sum, Count=Count)


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "ensemble_downscaling_known_answers.json")) as f:
        return json.load(f)


def known_answers():
    return golden()["cases"]


def valid(a):
    return np.isfinite(a)


def masked_rows(idx, vt, vf, tv, thr, op, check_valid=True):
    """(nq, E) float32: the masked members of every output cell (idx = nearest flat input cell per output cell)"""
    E = np.shape(vt)[-1]
    vt, vf, tv = (np.asarray(a, F).reshape(-1, E)[idx] for a in (vt, vf, tv))
    t = np.asarray(thr, F).ravel()[:, None]
    with np.errstate(invalid="ignore"):
        m = np.where(OPS[op](tv, t), vt, vf)
    if check_valid:
        m = np.where(valid(tv), m, F(np.nan))
    return m.astype(F)


def probability(idx, values, thr, op):
    E = np.shape(values)[-1]
    v = np.asarray(values, F).reshape(-1, E)[idx]
    t = np.asarray(thr, F).ravel()[:, None]
    ok = valid(v)
    count = ok.sum(axis=1)
    with np.errstate(invalid="ignore"):
        total = (OPS[op](v, t) & ok).sum(axis=1)
    out = np.full(count.shape, np.nan, F)
    some = count > 0
    out[some] = total[some].astype(F) / count[some].astype(F)
    return out.reshape(np.shape(thr))


def mask(O, idx, vt, vf, tv, thr, op, stat, quantile=None, check_valid=True):
    rows = masked_rows(idx, vt, vf, tv, thr, op, check_valid)
    out = np.empty(rows.shape[0], F)
    for k, m in enumerate(rows):
        out[k] = O.calc_quantile(m, quantile) if stat == Quantile else O.calc_statistic(m, stat)
    return out.reshape(np.shape(thr))


def compose_case(O, c, idx, op=None, check_valid=True):
    """a known-answer case through the restatement (op / check_valid: the deliberately wrong variants of the non-vacuity test)"""
    op = OP_NAMES[c["comparison_operator"]] if op is None else op
    thr = np.asarray(c["threshold"], F)
    if c["function"] == "downscale_probability":
        return probability(idx, np.asarray(c["values"], F), thr, op)
    cubes = [np.asarray(c[k], F) for k in ("ivalues_true", "ivalues_false", "threshold_values")]
    if c["function"] == "mask_threshold_downscale_quantile":
        return mask(O, idx, *cubes, thr, op, Quantile, c["quantile"], check_valid)
    return mask(O, idx, *cubes, thr, op, STAT_NAMES[c["statistic"]], None, check_valid)


def smart_candidates(O, g, q, st):
    """per output cell: (flat input indices within the localization distance, their float32 rho = st.corr(output cell, input cell))"""
    R = st.localization_distance()
    out = []
    for k in range(q.n):
        idx = O.get_neighbours(g, q.lats[k], q.lons[k], R)
        p1 = (q.x[k], q.y[k], q.z[k], q.elevs[k], q.lafs[k])
        out.append((idx, np.array([st.corr(p1, (g.x[i], g.y[i], g.z[i], g.elevs[i], g.lafs[i])) for i in idx], F)))
    return out


def smart(cands, values, num):
    """-> per output cell: out, kept count, mean |value| of the kept cells, relative rho gap across the cut (inf where nothing is cut)"""
    v = np.asarray(values, F).ravel()
    nq = len(cands)
    out = np.full(nq, np.nan, F)
    kept = np.zeros(nq, int)
    mabs = np.zeros(nq)
    gap = np.full(nq, np.inf)
    for k, (idx, rho) in enumerate(cands):
        if idx.size == 0 or num <= 0:
            continue
        order = np.lexsort((idx, -rho.astype(np.float64)))   # rho descending, ties -> lower index
        n = min(num, idx.size)
        sel = idx[order[:n]]
        s = F(0)
        for i in sel:
            s = F(s + v[i])
        out[k] = s / F(n)
        kept[k] = n
        mabs[k] = np.mean(np.abs(v[sel].astype(np.float64)))
        if idx.size > n:
            a, b = float(rho[order[n - 1]]), float(rho[order[n]])
            gap[k] = (a - b) / max(a, 1e-30)
    return out, kept, mabs, gap
