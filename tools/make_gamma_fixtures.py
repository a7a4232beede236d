"""Writes tests/golden/gamma_cases.npz: the value contract of gamma_inv and the Gamma transform evaluated with mpmath at
60 digits on seeded float32 inputs -- independent of the library and of scipy (scipy only supplies the starting point of the mpmath
root refinement where it has one; the refinement runs until its own step is below 1e-45 relative).

    python tools/make_gamma_fixtures.py          # about a minute

The domains are tests/gamma_ref.py's (the wide one and the reference benchmark's), plus the edges: the float32 neighbours of level 0,
0.5 and 1, the exact 0 and 1.  Every array is float32 (int32 for the parameter-set index)."""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import gamma_ref as R   # noqa: E402

F = np.float32
mp.mp.dps = 60
STOP = mp.mpf(10) ** -45
N_GAMMA_INV, N_SETS, N_FORWARD, N_BACKWARD = 1600, 8, 140, 110


def to_f32(x):
    """the float32 nearest to the mpmath number x (through double, then the neighbours: no double rounding)"""
    if mp.isnan(x):
        return F(np.nan)
    if mp.isinf(x):
        return F(np.inf) if x > 0 else F(-np.inf)
    with np.errstate(all="ignore"):
        c = F(float(x))
        cands = [c, np.nextafter(c, F(np.inf)), np.nextafter(c, F(-np.inf))]
    best = min((v for v in cands if np.isfinite(v)), key=lambda v: abs(mp.mpf(float(v)) - x), default=c)
    return F(best)


def p_inverse(a, p):
    """x with P(a, x) = p, 0 < p < 1: Newton on the logarithm of the smaller tail against ln x, from the leading term of the series"""
    a, p = mp.mpf(a), mp.mpf(p)
    upper = p > mp.mpf("0.5")
    target = mp.log(1 - p) if upper else mp.log(p)
    try:
        import scipy.special as sp
        x0 = sp.gammainccinv(float(a), float(1 - p)) if upper else sp.gammaincinv(float(a), float(p))
    except ImportError:
        x0 = 0.0
    if np.isfinite(x0) and x0 > 1e-250:
        u = mp.log(mp.mpf(x0))
    else:
        u = (mp.log(p) + mp.loggamma(a + 1)) / a
    for _ in range(200):
        x = mp.exp(u)
        tail = mp.gammainc(a, x, mp.inf, regularized=True) if upper else mp.gammainc(a, 0, x, regularized=True)
        if tail == 0:   # far below every float32: the leading term is the answer
            return x
        g = mp.log(tail) - target
        slope = mp.exp(a * u - x - mp.loggamma(a)) / tail * (-1 if upper else 1)
        du = -g / slope
        du = max(min(du, 2), -2)
        u += du
        if abs(du) < STOP:
            return mp.exp(u)
    raise RuntimeError("no convergence for a=%s p=%s" % (a, p))


def ndtri(c):
    c = mp.mpf(c)
    z = mp.mpf(0)
    try:
        import scipy.special as sp
        z = mp.mpf(float(sp.ndtri(float(c))))
    except ImportError:
        pass
    for _ in range(200):
        dz = -(mp.ncdf(z) - c) / mp.npdf(z)
        dz = max(min(dz, 1), -1)
        z += dz
        if abs(dz) < STOP * max(1, abs(z)):
            return z
    raise RuntimeError("no convergence for c=%s" % c)


def gamma_inv(level, shape, scale):
    if level == 0:
        return F(0)
    if level == 1:
        return F(np.inf)
    return to_f32(mp.mpf(float(scale)) * p_inverse(float(shape), float(level)))


def cdf_to_normal(c):
    if c == 0:
        return F(-np.inf)
    if c == 1:
        return F(np.inf)
    return to_f32(ndtri(float(c)))


def forward(v, shape, scale, tol):
    if not np.isfinite(v):
        return (F(np.nan),) * 3
    x = F(v) + F(tol)   # the float32 addition
    if x < 0:
        return (F(np.nan),) * 3
    r = mp.mpf(float(x)) / mp.mpf(float(scale))
    a = mp.mpf(float(shape))
    cdf = 1 - mp.gammainc(a, r, mp.inf, regularized=True) if r > a else mp.gammainc(a, 0, r, regularized=True)
    c = to_f32(cdf)
    lo, hi = max(np.nextafter(c, F(-1)), F(0)), min(np.nextafter(c, F(2)), F(1))
    return cdf_to_normal(c), cdf_to_normal(lo), cdf_to_normal(hi)


def backward(v, shape, scale, tol):
    if not np.isfinite(v):
        return F(np.nan)
    c = to_f32(mp.ncdf(mp.mpf(float(v))))
    if c == 1:
        return F(np.inf)
    x = mp.mpf(0) if c == 0 else p_inverse(float(shape), float(c))
    return to_f32(mp.mpf(float(scale)) * x - mp.mpf(float(tol)))


def main():
    level, shape, scale = R.seeded_gamma_inv(N_GAMMA_INV, seed=1)
    one = F(1)
    edges = [F(0), np.nextafter(F(0), one), F(R.TINY), np.nextafter(F(0.5), F(0)), F(0.5), np.nextafter(F(0.5), one), np.nextafter(one, F(0)), one]
    e_level, e_shape, e_scale = [], [], []
    for lv in edges:
        for a in (0.01, 0.5, 1.0, 2.5, 100.0, 1000.0):
            for s in (1e-3, 1.0, 1e3):
                e_level.append(lv), e_shape.append(a), e_scale.append(s)
    level = np.concatenate([level, np.array(e_level, F)])
    shape = np.concatenate([shape, np.array(e_shape, F)])
    scale = np.concatenate([scale, np.array(e_scale, F)])
    gi_want = np.array([gamma_inv(*c) for c in zip(level, shape, scale)], F)
    print("gamma_inv: %d cases, %d below the smallest normal, %d infinite" % (len(level), int(np.sum(np.abs(gi_want) < R.TINY)), int(np.isinf(gi_want).sum())), flush=True)

    params = R.seeded_params(N_SETS)
    rng = np.random.default_rng(2)
    fw_set, fw_in, fw_want, fw_lo, fw_hi, bw_set, bw_in, bw_want = [], [], [], [], [], [], [], []
    for k, p in enumerate(params):
        v = R.seeded_forward_inputs(p, N_FORWARD, rng)
        if k < 2:   # Gamma(1, 2): the reference's test inputs, and 35, where the float32 cdf has saturated
            v[-4:] = (0.0, 1.99, 35.0, 40.0)
        for x in v:
            w = forward(x, *p)
            fw_set.append(k), fw_in.append(x), fw_want.append(w[0]), fw_lo.append(w[1]), fw_hi.append(w[2])
        v = R.seeded_backward_inputs(N_BACKWARD, rng)
        if k < 2:
            v[-1] = 0.3374749
        for x in v:
            bw_set.append(k), bw_in.append(x), bw_want.append(backward(x, *p))
        print("set %d %s done" % (k, p), flush=True)
    out = os.path.join(ROOT, "tests", "golden", "gamma_cases.npz")
    np.savez_compressed(out, gi_level=level, gi_shape=shape, gi_scale=scale, gi_want=gi_want, params=params,
                        fw_set=np.array(fw_set, np.int32), fw_in=np.array(fw_in, F), fw_want=np.array(fw_want, F), fw_want_lo=np.array(fw_lo, F),
                        fw_want_hi=np.array(fw_hi, F), bw_set=np.array(bw_set, np.int32), bw_in=np.array(bw_in, F), bw_want=np.array(bw_want, F))
    print("wrote %s: %d bytes" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
