"""A numpy restatement of the reference's weather diagnostics (src/api/humidity.cpp, pressure.cpp, qnh.cpp, wind.cpp) and value
transforms (src/api/transform.cpp), written from the reference's text and sharing nothing with gridpp_amd/csrc/pointwise.h.

Every function takes arrays (or scalars), works element-wise and returns float32.  The float / double steps are explicit: `_d(x)` is the
promotion of a float to double, `_f(x)` the rounding at a store into a `float`; numpy keeps float32 op float32 in float32.  Transcendentals
(exp, log, pow, atan2) are evaluated in float64 from the already-rounded arguments and rounded where the reference stores a float; the
qualified std::atan2(float, float) of wind.cpp:21 is rounded to float32 at once.

mismatches() is the parity measure of the pointwise tests; the rest of the second half is what those tests share."""
import numpy as np

F, D = np.float32, np.float64
_ERR = dict(all="ignore")


def _a(x):
    """an argument as the reference receives it: a float (the typemap's rounding of whatever was given)"""
    with np.errstate(**_ERR):
        return np.asarray(x, dtype=D).astype(F)


def _d(x):
    return np.asarray(x).astype(D)


def _f(x):
    with np.errstate(**_ERR):
        return np.asarray(x).astype(F)


def _valid(x):   # util.cpp:16-18
    return np.isfinite(x)


def _nan_where(cond, x):
    return np.where(cond, F(np.nan), x).astype(F)


# ---- humidity.cpp ---------------------------------------------------------------------------------------------------------------------
def dewpoint(temperature, relative_humidity):
    t, rh = np.broadcast_arrays(_a(temperature), _a(relative_humidity))
    with np.errstate(**_ERR):
        tempC = _f(_d(t) - 273.15)                                                              # :8
        e = _f(_d(rh) * 0.611 * np.exp((17.63 * _d(tempC)) / (_d(tempC) + 243.04)))             # :9
        le = np.log(_d(e))
        tdC = _f((116.9 + 243.04 * le) / (16.78 - le))                                          # :10
        td = _f(_d(tdC) + 273.15)                                                               # :11
        out = np.where(td <= t, td, t)                                                          # :12 (a NaN td gives the temperature)
    return _nan_where(~(_valid(t) & _valid(rh)), out)


_EWT = np.array([.000034, .000089, .000220, .000517, .001155, .002472, .005080, .01005, .01921, .03553, .06356, .1111, .1891, .3139, .5088,
                 .8070, 1.2540, 1.9118, 2.8627, 4.2148, 6.1078, 8.7192, 12.272, 17.044, 23.373, 31.671, 42.430, 56.236, 73.777, 95.855,
                 123.40, 157.46, 199.26, 250.16, 311.69, 385.56, 473.67, 578.09, 701.13, 845.28, 1013.25], dtype=D).astype(F)   # :34-40


def _ewt(kelvin):   # :49-57
    x = _f((_d(kelvin) - 173.16) * 0.2)
    x = np.where(x < 0, F(0), np.where(x > 39, F(39), x)).astype(F)
    x = np.where(np.isfinite(x), x, F(0)).astype(F)   # (invalid inputs are masked by the caller)
    idx = x.astype(np.int32)
    return _EWT[idx] + (_EWT[idx + 1] - _EWT[idx]) * (x - idx.astype(F))


def relative_humidity(temperature, dewpoint):
    t, td = np.broadcast_arrays(_a(temperature), _a(dewpoint))
    with np.errstate(**_ERR):
        rh = _ewt(td) / _ewt(t)                                                                 # :68
        rh = np.where(rh < 0, F(0), rh)
        rh = np.where(rh > 1, F(1), rh)
        out = np.where(t <= td, F(1), rh)                                                       # :43-44
    return _nan_where(~(_valid(t) & _valid(td)), out)


def wetbulb(temperature, pressure, relative_humidity):
    t, p, rh = np.broadcast_arrays(_a(temperature), _a(pressure), _a(relative_humidity))
    with np.errstate(**_ERR):
        tC = _f(_d(t) - 273.15)                                                                 # :92
        early = (_d(tC) <= -243.04) | (rh <= 0)                                                 # :93
        bad = ~(_valid(tC) & _valid(p) & _valid(rh))                                            # :95
        e = _f(_d(rh) * 0.611 * np.exp((17.63 * _d(tC)) / (_d(tC) + 243.04)))                   # :96
        le = np.log(_d(e))
        Td = _f((116.9 + 243.04 * le) / (16.78 - le))                                           # :97
        gamma = _f(0.00066 * _d(p) / 1000)                                                      # :98
        delta = _f(_d(F(4098) * e) / np.power(_d(Td) + 243.04, 2.0))                            # :99
        zero = (gamma + delta) == 0                                                             # :100
        wb = (gamma * tC + delta * Td) / (gamma + delta)                                        # :102
        out = _f(_d(wb) + 273.15)                                                               # :103
    return _nan_where(early | bad | zero, out)


# ---- pressure.cpp ---------------------------------------------------------------------------------------------------------------------
def pressure(ielev, oelev, ipressure, itemperature=288.15):
    ie, oe, ip, it = np.broadcast_arrays(_a(ielev), _a(oelev), _a(ipressure), _a(itemperature))
    g0, M, R = F(9.80665), F(0.0289644), F(8.3144598)
    with np.errstate(**_ERR):
        arg = (-g0) * M * (oe - ie) / (R * it)
        out = _f(_d(ip) * np.exp(_d(arg)))                                                      # :11
    return _nan_where(~(_valid(ie) & _valid(oe) & _valid(ip) & _valid(it)), out)


SLP_MESSAGES = {1: "sea_level_pressure: altitude is NAN", 2: "sea_level_pressure: temperature is NAN",
                3: "sea_level_pressure: unphysical values in input"}


def sea_level_pressure(ps, altitude, temperature, rh=np.nan, dewpoint=np.nan):
    """-> (values, codes): codes 0, or 1 / 2 / 3 where the reference throws the message SLP_MESSAGES[code] (the value is NaN there)"""
    ps, alt, t, rh, dew = np.broadcast_arrays(_a(ps), _a(altitude), _a(temperature), _a(rh), _a(dewpoint))
    with np.errstate(**_ERR):
        code = np.where(~_valid(alt), 1, np.where(~_valid(t), 2, np.where((ps < 0) | (t < 0) | (rh < 0) | (rh > 1) | (dew < 0), 3, 0)))   # :32-38
        T = _f(_d(t) - 273.15)                                                                  # :42
        Ts = _f(273.15 + _d(T))                                                                 # :43
        g, R, a, Ch = F(9.80665), F(287.05), F(0.0065), F(0.12)
        ps = _f(_d(ps) * 0.01)                                                                  # :50
        # the relative humidity branch (:52-59)
        es = _f(6.11 * np.power(10., (7.5 * _d(T)) / (237.3 + _d(T))))
        e_rh = rh * es
        A, B, C = F(17.625), F(243.04), F(6.1094)
        lg = np.log(_d(e_rh / C))
        dew_rh = _f((_d(B) * lg) / (_d(A) - lg))
        # the dewpoint branch (:60-62)
        dew_dp = _f(_d(dew) - 273.15)
        e_dp = _f(6.11 * np.power(10., (7.5 * _d(dew_dp)) / (237.3 + _d(dew_dp))))
        # neither (:65-66)
        dew_no = _f(_d(T) - 3.)
        has_rh, has_dp = _valid(rh), _valid(dew)
        e = np.where(has_rh, e_rh, np.where(has_dp, e_dp, F(0))).astype(F)
        dp = np.where(has_rh, dew_rh, np.where(has_dp, dew_dp, dew_no)).astype(F)
        high = _f(_d(ps) * np.exp(_d(g * alt / R) / (_d(Ts) + 0.5 * _d(a) * _d(alt) + _d(e * Ch))))              # :70
        Tv = _f((273.15 + _d(T)) / (1 - 0.379 * (6.11 * np.power(10., (7.5 * _d(dp)) / (237.7 + _d(dp))) / _d(ps))))   # :72
        Ck = _f(_d(ps * alt) / (29.27 * _d(Tv)))                                                # :73
        low = ps + Ck
        slp = np.where(alt >= 50, high, np.where(alt < 50, low, F(0))).astype(F)
        out = _f(_d(slp) * 100.)                                                                # :77
    return _nan_where(code != 0, out), code.astype(np.int32)


# ---- qnh.cpp --------------------------------------------------------------------------------------------------------------------------
def qnh(pressure, altitude):
    p, alt = np.broadcast_arrays(_a(pressure), _a(altitude))
    g, T0, L, CRGas, p0 = F(9.80665), F(288.15), F(0.0065), F(287.053), F(101325)
    with np.errstate(**_ERR):
        inner = np.power(_d(p / p0), D((CRGas * L) / g))
        out = _f(D(p0) * np.power(inner + _d((alt * L) / T0), D(g / (CRGas * L))))              # :24
    out = _nan_where(~(_valid(alt) & _valid(p)), out)
    return np.where(p == 0, F(0), out).astype(F)                                                # :7-8


# ---- wind.cpp -------------------------------------------------------------------------------------------------------------------------
def wind_speed(xwind, ywind):
    x, y = np.broadcast_arrays(_a(xwind), _a(ywind))
    with np.errstate(**_ERR):
        return _f(np.sqrt(_d(x * x + y * y)))                                                   # :7


def wind_direction(xwind, ywind):
    x, y = np.broadcast_arrays(_a(xwind), _a(ywind))
    with np.errstate(**_ERR):
        d = _f(np.arctan2(_d(-x), _d(-y))) * F(180) / F(3.14159265)                             # :21
        return np.where(d < 0, d + F(360), d).astype(F)                                         # :22-23


# ---- transform.cpp --------------------------------------------------------------------------------------------------------------------
class Transform:
    def forward(self, value):
        return np.full(np.shape(value), -1, F)                                                  # :7-9

    def backward(self, value):
        return np.full(np.shape(value), -1, F)                                                  # :10-12


class Identity(Transform):
    def forward(self, value):
        return _a(value)

    backward = forward


class Log(Transform):
    def forward(self, value):
        v = _a(value)
        with np.errstate(**_ERR):
            return _nan_where(~_valid(v), _f(np.log(_d(v))))                                    # :85-90

    def backward(self, value):
        v = _a(value)
        with np.errstate(**_ERR):
            return _nan_where(~_valid(v), _f(np.exp(_d(v))))                                    # :91-96


class BoxCox(Transform):
    def __init__(self, threshold):
        self.threshold = F(threshold)

    def forward(self, value):
        v, thr = _a(value), self.threshold
        with np.errstate(**_ERR):
            w = np.where(v <= 0, F(0), v).astype(F)                                             # :103-104
            if thr == 0:
                out = _f(np.log(_d(w)))
            else:
                out = _f((np.power(_d(w), D(thr)) - 1) / D(thr))                                # :108
        return _nan_where(~_valid(v), out)

    def backward(self, value):
        v, thr = _a(value), self.threshold
        with np.errstate(**_ERR):
            if thr == 0:
                r = _f(np.exp(_d(v)))
            else:
                bound = -1.0 / D(thr)
                w = np.where(_d(v) < bound, F(bound), v).astype(F)                              # :117-119
                r = _f(np.power(_d(F(1) + thr * w), D(F(1) / thr)))                             # :120
            r = np.where(r <= 0, F(0), r)                                                       # :122-123
        return _nan_where(~_valid(v), r)


class StartedBoxCox(Transform):
    def __init__(self, threshold, scaling_factor):
        if not np.isfinite(F(threshold)) or F(threshold) <= 0:
            raise ValueError("threshold parameter must be > 0 in the started Box-Cox distribution")
        if not np.isfinite(F(scaling_factor)) or F(scaling_factor) <= 0:
            raise ValueError("Scaling factor parameter must be > 0 in the started Box-Cox distribution")
        self.threshold, self.scaling = F(threshold), F(scaling_factor)

    def forward(self, value):
        v, thr, s = _a(value), self.threshold, self.scaling
        with np.errstate(**_ERR):
            w = np.where(v < 0, F(0), v).astype(F)                                              # :136-137
            big = _f(D(s) * (1 + ((np.power(_d(w / s), D(thr)) - 1) / D(thr))))                 # :141
            out = np.where(w <= s, w, big)
        return _nan_where(~_valid(v), out)

    def backward(self, value):
        v, thr, s = _a(value), self.threshold, self.scaling
        with np.errstate(**_ERR):
            big = _f(D(s) * np.power(_d(F(1) + thr / s * (v - s)), D(F(1) / thr)))              # :150
            r = np.where(v <= s, v, big)
            r = np.where(r < 0, F(0), r)                                                        # :151-152
        return _nan_where(~_valid(v), r)


# ---- the parity measure -----------------------------------------------------------------------------------------------------------------
def mismatches(got, want, rtol):
    """indices where got differs from want: NaN matches NaN, infinities match by sign, -0.0 equals 0, finite values within rtol relative
    (rtol = 0: equal)"""
    got, want = np.asarray(got, F).ravel(), np.asarray(want, F).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(**_ERR):
        same = got == want   # equal values, infinities of one sign, +-0
        g, w = got.astype(D), want.astype(D)
        close = np.isfinite(g) & np.isfinite(w) & (np.abs(g - w) <= rtol * np.maximum(np.abs(g), np.abs(w)))
    return np.nonzero(~(both_nan | same | close))[0]


def bit_differences(got, want):
    """how many values are not bit-identical (NaN payloads and the sign of zero set aside)"""
    return int(mismatches(got, want, 0).size)


# ---- what the tests share: the pins, the seeded inputs and the tolerance of every function ------------------------------------------------
RTOL = 1e-5   # the project's parity measure for floats (BASELINE.json)
# bit for bit where no transcendental is involved: the same IEEE operations in the same order
EXACT = ("relative_humidity", "wind_speed", "Identity")
DIAGNOSTICS = {"dewpoint": 2, "relative_humidity": 2, "wetbulb": 3, "pressure": 4, "sea_level_pressure": 5, "qnh": 2, "wind_speed": 2,
               "wind_direction": 2}   # name -> number of arguments


def pins():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointwise_known_answers.json")) as f:
        return json.load(f)


def nan_of(x):
    """null of the JSON -> NaN, in nested lists too"""
    if isinstance(x, list):
        return [nan_of(v) for v in x]
    return np.nan if x is None else x


def within_decimals(got, want, decimals):
    """the reference's assertAlmostEqual(got, want, decimals) (and stricter than numpy's assert_almost_equal, which allows 1.5 units);
    decimals None: NaN expected; "exact": equal"""
    got, want = np.asarray(got, D), np.asarray(want, D)
    if decimals is None:
        return bool(np.all(np.isnan(got)))
    if decimals == "exact":
        return bool(np.all(got == want))
    return bool(np.all(np.abs(got - want) < 0.5 * 10.0 ** -decimals))


_SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 1.0, -273.15, 1e30, -1e30], F)


def sprinkle(rng, a, specials=_SPECIALS, share=0.03):
    """a with `share` of its values replaced by special ones"""
    a = np.array(a, F)
    hit = rng.random(a.size) < share
    a[hit] = rng.choice(np.asarray(specials, F), int(hit.sum()))
    return a


def seeded_inputs(name, n, seed=20240607, offenders=True):
    """n seeded cases of the arguments of a diagnostic: physical ranges (temperatures beyond both ends of the humidity table, altitudes on
    both sides of sea_level_pressure's 50 m) with NaN, +-inf, 0, -0.0 and negatives sprinkled in.  offenders = False: nothing that makes
    sea_level_pressure throw (NaN and inf stay where the reference lets them pass)."""
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    u = lambda lo, hi: rng.uniform(lo, hi, n).astype(F)
    t = u(150, 400)
    if name == "dewpoint":
        args = [t, u(-0.1, 1.1)]
    elif name == "relative_humidity":
        args = [t, (t - u(-5, 60)).astype(F)]
    elif name == "wetbulb":
        args = [t, u(30000, 110000), u(-0.1, 1.1)]
    elif name == "pressure":
        args = [u(-500, 5000), u(-500, 5000), u(30000, 110000), u(200, 330)]
    elif name == "qnh":
        args = [u(30000, 110000), u(-1000, 9000)]
    elif name in ("wind_speed", "wind_direction"):
        args = [rng.normal(0, 10, n).astype(F), rng.normal(0, 10, n).astype(F)]
        args[0][rng.random(n) < 0.05] = 0   # the axes, where atan2 changes its branch
        args[1][rng.random(n) < 0.05] = 0
    elif name == "sea_level_pressure":
        alt = np.where(rng.random(n) < 0.3, u(0, 100), u(-400, 4000)).astype(F)   # a third around the 50 m switch
        which = rng.integers(0, 3, n)   # relative humidity given / dewpoint given / neither
        rh = np.where(which == 0, u(0, 1), F(np.nan)).astype(F)
        dew = np.where(which == 1, u(220, 300), F(np.nan)).astype(F)
        dew = np.where(rng.random(n) < 0.1, u(220, 300), dew).astype(F)   # (both given: the relative humidity wins)
        args = [u(50000, 110000), alt, u(230, 320), rh, dew]
        if not offenders:
            args[0] = sprinkle(rng, args[0], [np.nan, np.inf, 0.0, -0.0, 1.0, 1e30])
            args[3] = sprinkle(rng, args[3], [np.nan, 0.0, -0.0, 1.0])   # (an infinite relative humidity is > 1: it offends)
            args[4] = sprinkle(rng, args[4], [np.nan, 0.0, -0.0, 1.0, 1e30])
            return args
    else:
        raise KeyError(name)
    return [sprinkle(rng, a) for a in args]


def transforms():
    """the transforms the tests run: (id, constructor name, parameters)"""
    return [("Identity", "Identity", ()), ("Log", "Log", ()), ("BoxCox(0.1)", "BoxCox", (0.1,)), ("BoxCox(0)", "BoxCox", (0,)),
            ("BoxCox(-0.5)", "BoxCox", (-0.5,)), ("StartedBoxCox(0.3, 2.5)", "StartedBoxCox", (0.3, 2.5))]


def seeded_values(direction, n, seed=20240608):
    """n seeded inputs of a transform: precipitation-like values (many zeros, a tenth of them within 1e-5 of 1, where BoxCox.forward
    cancels) for forward, transformed-space values (beyond BoxCox's -1 / threshold bound too) for backward, specials sprinkled in"""
    rng = np.random.default_rng([seed, len(direction)])
    if direction == "forward":
        v = rng.gamma(0.7, 4.0, n)
        v[rng.random(n) < 0.2] = 0
        near = rng.random(n) < 0.1
        v[near] = 1 + rng.uniform(-1e-5, 1e-5, int(near.sum()))
        v[rng.random(n) < 0.05] *= -1
    else:
        v = rng.uniform(-15, 8, n)
        wide = rng.random(n) < 0.1
        v[wide] = rng.uniform(-100, 100, int(wide.sum()))
    return sprinkle(rng, v.astype(F))


def transform_mismatches(tid, direction, values, got, want):
    """mismatches() with the tolerance of the transform.  BoxCox.forward with a threshold != 0 subtracts 1 from a power that is near 1
    for an input near 1: one float32 ulp of the power is then any relative amount of the result, so for inputs within 0.5 of 1 the
    POWER the reference computed, 1 + threshold * out, is compared at RTOL instead of out."""
    if tid.startswith("Identity"):
        return mismatches(got, want, 0)
    if tid.startswith("BoxCox") and direction == "forward" and not tid.startswith("BoxCox(0)"):
        thr = D(F(float(tid[len("BoxCox("):-1])))
        near = np.abs(np.asarray(values, D).ravel() - 1) < 0.5
        power = lambda o: np.where(near, 1 + thr * np.asarray(o, D).ravel(), np.asarray(o, D).ravel())
        return mismatches(power(got), power(want), RTOL)
    return mismatches(got, want, RTOL)
