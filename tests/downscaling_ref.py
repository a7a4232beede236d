"""The downscalers restated as a numpy float32 composition over a per-field downscaler d(f) (the reference's structure:
src/api/simple_gradient.cpp, src/api/gradient.cpp:5-274 downscale every field on its own, then combine them):

    simple_gradient: out = d(values) + (oelev - d(ielevs)) * elev_gradient                      (no validity test)
    full_gradient:   out = d(values) + (laf_corr + elev_corr),
                     elev_corr = d(elev_gradient) * (oelev - d(ielevs)) where oelev and d(ielevs) are valid, else 0; laf_corr alike

d is built on the oracle (oracle.nearest / oracle.bilinear) or on the library's own nearest / bilinear; the known answers
(tests/golden/downscaling_known_answers.json) pin the composition, the GPU tests compare the fused kernel with it."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def known_answers():
    with open(os.path.join(ROOT, "tests", "golden", "downscaling_known_answers.json")) as f:
        return json.load(f)["cases"]


def _arr(a):
    if a is None:
        return None
    return np.asarray(a, dtype=np.float64)


def set_arrays(d):
    """a grid / points description of the known answers -> (lats, lons, elevs, lafs) as float64 arrays (None where not given)"""
    return _arr(d["lats"]), _arr(d["lons"]), _arr(d.get("elevs")), _arr(d.get("lafs"))


def oracle_downscaler(O, glats, glons, qlats, qlons, downscaler, ctype=0):
    """d(f) on the oracle: f (Y, X) -> (nq,), f (T, Y, X) -> (T, nq)"""
    Y, X = np.shape(glats)
    g = O.Pts(np.ravel(glats), np.ravel(glons), ctype=ctype)
    q = O.Pts(np.ravel(qlats), np.ravel(qlons), ctype=ctype)

    def d(f):
        f = np.asarray(f, F32)
        if g.n == 0:
            return np.full(f.shape[:-2] + (q.n,), np.nan, F32)
        if downscaler == 1:
            return O.bilinear(g, (Y, X), q, f)
        if f.ndim == 3:
            return np.stack([O.nearest(g, q, f[t]) for t in range(f.shape[0])]) if f.shape[0] else np.zeros((0, q.n), F32)
        return O.nearest(g, q, f)
    return d


def device_downscaler(gridpp, igrid, output, downscaler):
    """d(f) with the library's own nearest / bilinear (the composed device path)"""
    nq = output.size() if not isinstance(output, gridpp.Grid) else int(np.prod(output.size()))

    def d(f):
        f = np.asarray(f, F32)
        r = gridpp.bilinear(igrid, output, f) if downscaler == 1 else gridpp.nearest(igrid, output, f)
        return np.asarray(r).reshape(f.shape[:-2] + (nq,))
    return d


def _valid(a):
    return np.isfinite(a)


def compose_simple(d, values, ielevs, oelevs, elev_gradient):
    """-> (T, nq) or (nq,) float32"""
    values = np.asarray(values, F32)
    ie = np.full(values.shape[-2:], np.nan, F32) if ielevs is None else np.asarray(ielevs, F32)
    oe = np.asarray(oelevs, F32).ravel()
    with np.errstate(invalid="ignore", over="ignore"):
        corr = (oe - d(ie)) * F32(elev_gradient)
        return (d(values) + corr).astype(F32)


def compose_full(d, values, elev_gradient, laf_gradient, ielevs, ilafs, oelevs, olafs):
    """gradients: arrays of the values' shape, or None (absent)"""
    values = np.asarray(values, F32)
    out = d(values)
    zero = np.zeros_like(out)
    corr = {}
    with np.errstate(invalid="ignore", over="ignore"):
        for name, grad, ifield, ofield in (("laf", laf_gradient, ilafs, olafs), ("elev", elev_gradient, ielevs, oelevs)):
            if grad is None:
                corr[name] = zero
                continue
            dg = d(np.asarray(grad, F32))
            di = d(np.full(values.shape[-2:], np.nan, F32) if ifield is None else np.asarray(ifield, F32))
            o = np.asarray(ofield, F32).ravel()
            ok = _valid(o) & _valid(di)
            corr[name] = np.where(ok, dg * (o - di), F32(0)).astype(F32)
        return (out + (corr["laf"] + corr["elev"])).astype(F32)


def present(g):
    """a gradient argument with no elements means: this term is absent"""
    return None if g is None or np.size(g) == 0 else g
