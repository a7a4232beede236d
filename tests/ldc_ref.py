"""local_distribution_correction restated in numpy float32 over the oracle (src/api/local_distribution_correction.cpp:33-203).

The reference has one test of this function, a comparison between thread counts, and no numeric pin: parity is pinned by this
restatement alone (and the restatement by the hand-derived answers of tests/test_ldc_restatement.py).

    neighbours      oracle.get_neighbours(points, cell, structure.localization_distance()), match included
    rho             Struct.corr(cell, station, background=True); stations with rho = 0 take part
    kept pairs      per (time, station): both values valid and >= 0
    count, sum_rho  number of kept pairs; float32 sum of their rho in the order of enumeration
    the two sorts   (pobs, rho) and (pbackground, rho), each ascending by value, ties in value by rho ascending (-0 sorts as +0).
                    THE TIE RULE is this project's: the reference sorts by value alone with an unstable sort, so on tied
                    values its result depends on its R-tree's enumeration order.  stable=True sorts by value alone with a
                    stable sort instead (one of the orders the reference may produce); only the sensitivity test uses it.
    trimming        d0 = (int)((float)count * min_quantile), d1 likewise; entries [d0, d1)
    the curves      (0, 0) prepended, sequential float32 cumulative rho, normalised as :151-154 (the leading 0 stays 0)
    branches        :156-198 in their order; 0.01 and 0.1 are double literals there, so those two comparisons are made in double
    interpolate     the oracle's (src/api/util.cpp:377-414); exp rounded to float32.  Where a rho total of 0 has made a curve's quantiles
                    NaN a scan can end without an index; the reference indexes with (int) NaN there, the project's rule is NaN
                    (gridpp_amd/csrc/curve.h, tests/curve_ref.py) and the oracle follows it

Per cell it also returns the branch taken and the count."""
import math

import numpy as np

F = np.float32
INVALID, FEW, B1, B2A, B2B, B2C, B3, B4 = "invalid", "too few", "1", "2a", "2b", "2c", "3", "4"
TAGS = (INVALID, FEW, B1, B2A, B2B, B2C, B3, B4)


def candidates(O, g, p, st):
    """per cell: (station indices in the oracle's enumeration order, their float32 corr_background)"""
    R = st.localization_distance()
    out = []
    for k in range(g.n):
        idx = O.get_neighbours(p, g.lats[k], g.lons[k], R)
        p1 = (g.x[k], g.y[k], g.z[k], g.elevs[k], g.lafs[k])
        out.append((idx, np.array([st.corr(p1, (p.x[i], p.y[i], p.z[i], p.elevs[i], p.lafs[i]), background=True) for i in idx], F)))
    return out


def _curve(values, rho, d0, d1, stable, min_quantile, max_quantile):
    v = values + F(0)   # -0 -> +0
    order = np.argsort(v, kind="stable") if stable else np.lexsort((rho, v))
    sel = order[d0:d1]
    x = np.concatenate([[F(0)], v[sel]]).astype(F)
    q = np.zeros(x.size, F)
    for s in range(1, x.size):   # :135-141
        q[s] = F(q[s - 1] + rho[sel[s - 1]])
    total = q[-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        q[1:] = min_quantile + q[1:] / total * F(max_quantile - min_quantile)   # :151-154
    return x, q, total


def ldc(O, cands, background, pobs, pbackground, min_quantile, max_quantile, min_points, stable=False, order=None, sums=None):
    """-> (out float32 of background's shape, tag per cell, count per cell).  pobs / pbackground are (S) or (T, S).
    order: a function permuting each cell's enumeration (the sensitivity test shuffles it).
    sums: a dict that receives, per cell that built its curves (NaN elsewhere), "sum_r" and "sum_f" -- the rho totals of the
    trimmed ref and fcst curves, the divisors of :151-154 -- "sum_rho" and, on branch 4, the weight "w0"."""
    bg = np.asarray(background, F)
    b_flat = bg.ravel()
    po, pb = np.atleast_2d(np.asarray(pobs, F)), np.atleast_2d(np.asarray(pbackground, F))
    min_quantile, max_quantile = F(min_quantile), F(max_quantile)
    nT = po.shape[0]
    out = b_flat.copy()
    tags, counts = [], np.zeros(b_flat.size, int)
    if sums is not None:
        sums.update({name: np.full(b_flat.size, np.nan, F) for name in ("sum_r", "sum_f", "sum_rho", "w0")})
    for k, (idx, rho) in enumerate(cands):
        b = b_flat[k]
        if not np.isfinite(b):   # :72
            tags.append(INVALID)
            continue
        if order is not None:
            perm = order(idx.size)
            idx, rho = idx[perm], rho[perm]
        ref, fcst, w = [], [], []
        sum_rho = F(0)
        for i, r in zip(idx, rho):   # :93-112
            for t in range(nT):
                o, f = po[t, i], pb[t, i]
                if not np.isfinite(o) or not np.isfinite(f) or o < 0 or f < 0:
                    continue
                ref.append(o); fcst.append(f); w.append(r)
                sum_rho = F(sum_rho + r)
        count = counts[k] = len(w)
        if count < min_points:   # :114
            tags.append(FEW)
            continue
        ref, fcst, w = np.array(ref, F), np.array(fcst, F), np.array(w, F) + F(0)
        d0, d1 = int(F(count) * min_quantile), int(F(count) * max_quantile)   # :121-122
        x_ref, q_ref, sum_r = _curve(ref, w, d0, d1, stable, min_quantile, max_quantile)
        x_fcst, q_fcst, sum_f = _curve(fcst, w, d0, d1, stable, min_quantile, max_quantile)
        if sums is not None:
            sums["sum_r"][k], sums["sum_f"][k], sums["sum_rho"][k] = sum_r, sum_f, sum_rho
        if float(b) < 0.01:   # :156
            out[k] = 0
            tags.append(B1)
        elif x_ref[-1] <= 0:   # :160
            if b < F(3) * x_fcst[-1]:
                out[k] = 0
                tags.append(B2A)
            elif float(b) < 0.1:
                out[k] = 0
                tags.append(B2B)
            else:
                tags.append(B2C)
        elif b >= x_fcst[-1]:   # :178
            out[k] = F(b + F(x_ref[-1] - x_fcst[-1]))
            tags.append(B3)
        else:   # :186
            q = F(O.interpolate(b, x_fcst, q_fcst))
            new_ref = F(O.interpolate(q, q_ref, x_ref))
            w0 = F(F(1) - F(math.exp(float(F(F(-0.01) * sum_rho)))))
            w1 = F(F(1) - w0)
            if sums is not None:
                sums["w0"][k] = w0
            out[k] = F(F(w0 * new_ref) + F(w1 * b))
            tags.append(B4)
    return out.reshape(bg.shape), np.array(tags), counts


class FixtureA:
    """A 12 x 12 Cartesian grid over 20 km plus two rows 60 km and more away (14 x 12); 60 stations uniform over the box and 12
    "dry" stations beside the far rows (pobs = 0, pbackground in [0, 0.02]: 3 * fcst_last < 0.1, so 2b is reachable); T = 3;
    values ~ gamma(0.6, 3); one NaN pobs entry, one negative pbackground entry; background ~ gamma(0.6, 3) with one NaN cell,
    one cell at 0.001 and the first far row at linspace(0.02, 0.5, 12).  rounded: values and background to 0.5 mm (many tied zeros)."""
    H, MINQ, MAXQ, MIN_POINTS = 2500.0, 0.1, 0.9, 5

    def __init__(self, rounded=False, seed=7):
        rng = np.random.default_rng(seed)
        xs = np.linspace(0, 20000, 12)
        ys = np.concatenate([xs, [80000.0, 88000.0]])
        self.lons, self.lats = np.meshgrid(xs, ys)
        S, D, T = 60, 12, 3
        self.px = np.concatenate([rng.uniform(0, 20000, S), rng.uniform(0, 20000, D)])
        self.py = np.concatenate([rng.uniform(0, 20000, S), rng.uniform(79000, 81000, D)])
        pobs = rng.gamma(0.6, 3, (T, S + D)).astype(F)
        pbg = rng.gamma(0.6, 3, (T, S + D)).astype(F)
        bg = rng.gamma(0.6, 3, self.lats.shape).astype(F)
        if rounded:
            pobs, pbg, bg = (np.round(a * 2) / 2 for a in (pobs, pbg, bg))
        pobs[:, S:] = 0
        pbg[:, S:] = rng.uniform(0, 0.02, (T, D))
        pobs[1, 7] = np.nan
        pbg[2, 11] = -1.0
        bg[3, 4] = np.nan
        bg[5, 6] = 0.001
        bg[12] = np.linspace(0.02, 0.5, 12)
        self.pobs, self.pbg, self.bg = pobs.astype(F), pbg.astype(F), bg.astype(F)

    def oracle_points(self, O):
        return O.Pts(self.lats, self.lons, ctype=1), O.Pts(self.py, self.px, ctype=1)

    def device_points(self, gridpp):
        return (gridpp.Grid(self.lats, self.lons, ((),), ((),), gridpp.Cartesian),
                gridpp.Points(self.py, self.px, (), (), gridpp.Cartesian))
