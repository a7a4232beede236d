"""What the gamma tests share: the loader of tests/golden/gamma_cases.npz (written by tools/make_gamma_fixtures.py with mpmath), the
comparison rule, the seeded inputs, and a scipy.special restatement of the value contract for the soaks on machines
that have scipy (`restatement()` is behind pytest.importorskip).

The comparison rule
  * 1e-5 relative (pointwise_ref.RTOL, the project's parity measure); NaN matches NaN, infinities match by sign;
  * where |expected| is below float32's smallest normal, the difference is at most that number (a result there is a subnormal or 0:
    a relative measure has nothing to hold on to) -- such cases are compared, not dropped;
  * Gamma.forward only: a result may instead match the expected value for one of the two float32 neighbours of the cdf.  The cdf is
    rounded to float32 before the normal quantile (transform.cpp:169), and near 1 one float32 step of it moves the result by more than
    0.1, so a cdf that is 1e-13 off and falls on the other side of a rounding boundary must not count as an error (the precedent is
    pointwise_ref.transform_mismatches for BoxCox near 1)."""
import os

import numpy as np

from tests.pointwise_ref import RTOL

F = np.float32
TINY = float(np.finfo(F).tiny)   # 1.1754944e-38
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gamma_cases.npz")

# the reference's own known answers: tests/test_distribution.py:11-16 of the reference, (level, shape, scale) -> value, to 3 decimals there
# (the digits are those of the function itself, which scipy.special reproduces)
PINS_GAMMA_INV = [((0.5, 1.0, 2.0), 1.38629), ((0.5, 2.0, 2.0), 3.35669), ((0.5, 7.5, 1.0), 7.16943)]
# tests/test_transform.py:67-75 of the reference: Gamma(1, 2, 0.01)
PINS_TRANSFORM = [("forward", 0.0, -2.5766933), ("forward", 1.99, 0.33747494), ("backward", 0.3374749, 1.99)]
PIN_DECIMALS = 5   # np.testing.assert_almost_equal(..., 5) of the vector forms there


def _match(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(all="ignore"):
        both_nan = np.isnan(got) & np.isnan(want)
        inf = np.isinf(want)
        same_inf = inf & (got == want)
        small = ~inf & (np.abs(want) < TINY)
        ok_small = small & (np.abs(got - want) <= TINY)
        ok_rel = ~inf & ~small & (np.abs(got - want) <= RTOL * np.abs(want))
    return both_nan | same_inf | ok_small | ok_rel


def mismatches(got, want, alternatives=()):
    """indices where `got` matches neither `want` nor any of `alternatives` under the rule above"""
    ok = _match(got, want)
    for alt in alternatives:
        ok |= _match(got, alt)
    return np.flatnonzero(~ok.ravel())


def report(idx, got, want, *inputs):
    i = idx[:5]
    return "%d mismatches, first at %s: got %s want %s inputs %s" % (len(idx), i, np.asarray(got).ravel()[i], np.asarray(want).ravel()[i],
                                                                   [np.asarray(a).ravel()[i] for a in inputs])


class Golden:
    """gamma_inv: level / shape / scale / want.  forward: per case the index of its parameter set (params[k] = shape, scale, tolerance),
    the input, want and the wants of the cdf's two float32 neighbours.  backward: set, input, want."""

    def __init__(self):
        z = np.load(GOLDEN)
        self.gi_level, self.gi_shape, self.gi_scale, self.gi_want = z["gi_level"], z["gi_shape"], z["gi_scale"], z["gi_want"]
        self.params = z["params"]
        self.fw_set, self.fw_in, self.fw_want, self.fw_want_lo, self.fw_want_hi = z["fw_set"], z["fw_in"], z["fw_want"], z["fw_want_lo"], z["fw_want_hi"]
        self.bw_set, self.bw_in, self.bw_want = z["bw_set"], z["bw_in"], z["bw_want"]
        for a in vars(self).values():
            assert a.dtype in (F, np.int32)
            a.setflags(write=False)

    def forward_sets(self):
        for k, p in enumerate(self.params):
            m = self.fw_set == k
            yield tuple(float(v) for v in p), self.fw_in[m], self.fw_want[m], (self.fw_want_lo[m], self.fw_want_hi[m])

    def backward_sets(self):
        for k, p in enumerate(self.params):
            m = self.bw_set == k
            yield tuple(float(v) for v in p), self.bw_in[m], self.bw_want[m]


_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = Golden()
    return _golden


def tile(a, n):
    """the first n values of `a` repeated"""
    return np.resize(a, n)


# ---- the seeded domains (the issue's: wide, and the reference benchmark's tests/benchmark.py:78) -------------------------------------------
def log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(F)


def seeded_gamma_inv(n, seed=20240611):
    rng = np.random.default_rng(seed)
    h = n // 2
    level = np.concatenate([rng.random(h), 0.05 + 0.9 * rng.random(n - h)]).astype(F)
    shape = np.concatenate([log_uniform(rng, 1e-2, 1e3, h), np.maximum(rng.random(n - h), 1e-7).astype(F)])
    scale = np.concatenate([log_uniform(rng, 1e-3, 1e3, h), np.maximum(rng.random(n - h), 1e-7).astype(F)])
    return level, shape, scale


def seeded_params(n, seed=20240612):
    """(shape, scale, tolerance) sets: Gamma(1, 2, 0.01) and Gamma(1, 2, 0) first, then the wide domain with either tolerance"""
    rng = np.random.default_rng(seed)
    out = [(1.0, 2.0, 0.01), (1.0, 2.0, 0.0)]
    shape, scale = log_uniform(rng, 1e-2, 1e3, n), log_uniform(rng, 1e-3, 1e3, n)
    for k in range(n - 2):
        out.append((float(shape[k]), float(scale[k]), 0.01 if k % 2 == 0 else 0.0))
    return np.array(out[:n], F)


def saturation(shape, scale):
    """about where the float32 cdf of Gamma(shape, scale) reaches 1 (35 for Gamma(1, 2)): mean + 6 standard deviations + 18 scales"""
    return float(scale) * (float(shape) + 6 * np.sqrt(float(shape)) + 18)


def seeded_forward_inputs(params, n, rng):
    """from 0 to past the saturation of the cdf: a third log-uniform towards 0, the rest uniform, and the specials"""
    top = 1.15 * saturation(params[0], params[1])
    v = np.concatenate([log_uniform(rng, top * 1e-8, top, n // 3), rng.uniform(0, top, n - n // 3).astype(F)])
    specials = np.array([0.0, -0.0, top, -0.005, -0.02, -1.0, np.nan, np.inf, -np.inf], F)
    v[:len(specials)] = specials
    return v.astype(F)


def seeded_backward_inputs(n, rng):
    v = rng.uniform(-15, 6, n).astype(F)
    specials = np.array([-15, -14.5, -14.0, -5.0, 0.0, 5.4, 5.5, 6.0, np.nan, np.inf, -np.inf], F)
    v[:len(specials)] = specials
    return v


# ---- the contract, restated with scipy.special ------------------------------------------------------------------------------------------
class Restatement:
    def __init__(self, special):
        self.sp = special

    def p_inverse(self, a, p):
        a, p = np.asarray(a, np.float64), np.asarray(p, np.float64)
        with np.errstate(all="ignore"):
            low = self.sp.gammaincinv(a, np.minimum(p, 0.5))
            high = self.sp.gammainccinv(a, np.where(p > 0.5, 1 - p, 0.5))   # 1 - p is exact for a float32 p
        return np.where(p > 0.5, high, low)

    def gamma_inv(self, level, shape, scale):
        level, shape, scale = (np.asarray(a, F) for a in (level, shape, scale))
        with np.errstate(all="ignore"):
            return (scale.astype(np.float64) * self.p_inverse(shape, level)).astype(F)

    def cdf_to_normal(self, c):
        c = np.asarray(c, F)
        with np.errstate(all="ignore"):
            return np.where(c == 0, -np.inf, np.where(c == 1, np.inf, self.sp.ndtri(c.astype(np.float64)))).astype(F)

    def forward(self, value, shape, scale, tolerance, neighbours=False):
        v = np.asarray(value, F)
        x = v + F(tolerance)   # a float32 addition
        with np.errstate(all="ignore"):
            c = self.sp.gammainc(float(F(shape)), np.maximum(x, 0).astype(np.float64) / float(F(scale))).astype(F)
        bad = ~np.isfinite(v) | (x < 0)

        def finish(c_):
            return np.where(bad, np.nan, self.cdf_to_normal(c_)).astype(F)
        if not neighbours:
            return finish(c)
        return finish(c), finish(np.maximum(np.nextafter(c, F(-1)), F(0))), finish(np.minimum(np.nextafter(c, F(2)), F(1)))

    def backward(self, value, shape, scale, tolerance):
        v = np.asarray(value, F)
        with np.errstate(all="ignore"):
            c = self.sp.ndtr(np.where(np.isfinite(v), v, 0).astype(np.float64)).astype(F)
            x = float(F(scale)) * self.p_inverse(float(F(shape)), np.where(c < 1, c, 0.5)) - float(F(tolerance))
            out = np.where(c == 1, np.inf, x)
        return np.where(np.isfinite(v), out, np.nan).astype(F)


def restatement():
    import pytest
    return Restatement(pytest.importorskip("scipy.special"))
