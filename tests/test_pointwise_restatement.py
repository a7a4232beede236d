"""CPU: the numpy restatement of the weather diagnostics and the value transforms (tests/pointwise_ref.py) against every known answer of
the reference's own tests (tests/golden/pointwise_known_answers.json), to the decimals the reference asserts, and against a hand-worked
case for every quirk of the reference's text that the implementation has to keep.  The restatement is what the API and the GPU tests
compare with, so this file is what makes it trustworthy."""
import math

import numpy as np
import pytest

from tests import pointwise_ref as R

PINS = R.pins()
F = np.float32


def _id(c):
    return "%s%s@%s" % (c.get("fn") or c["transform"] + "." + c["direction"], c.get("args", c.get("input")), c["source"].split("/")[-1])


@pytest.mark.parametrize("case", PINS["diagnostics"], ids=_id)
def test_diagnostic_pins(case):
    args = R.nan_of(case["args"])
    if case["fn"] == "sea_level_pressure":
        value, code = R.sea_level_pressure(*args)
        if "raises" in case:
            assert case["raises"] == "RuntimeError" and int(code) in R.SLP_MESSAGES and np.isnan(value)
            return
        assert int(code) == 0
    else:
        value = getattr(R, case["fn"])(*args)
    assert value.dtype == F
    assert R.within_decimals(value, R.nan_of(case["expected"]), case["decimals"]), (float(value), case)


def make(case):
    return getattr(R, case["transform"])(*case["params"])


@pytest.mark.parametrize("case", PINS["transforms"], ids=_id)
def test_transform_pins(case):
    t, x = make(case), R.nan_of(case["input"])
    for shape in [()] + [tuple(s) for s in PINS["vector_shapes"]]:
        value = x * np.ones(shape)
        got = t.backward(t.forward(value)) if case["direction"] == "roundtrip" else getattr(t, case["direction"])(value)
        assert got.dtype == F and got.shape == shape
        assert R.within_decimals(got, R.nan_of(case["expected"]) * np.ones(shape), case["decimals"]), (got, case)


def test_the_two_exact_pins_are_exact():
    """assertAlmostEqual to 7 places at 1e5 is equality of the float32"""
    assert R.sea_level_pressure(101325.0, 20, 273.15)[0] == F(101578.0)
    assert R.sea_level_pressure(101325.0, 50, 273.15)[0] == F(101960.25)


# ---- the quirks, one hand-worked case each -----------------------------------------------------------------------------------------------
def test_dewpoint_returns_the_temperature_where_td_does_not_compare():
    """humidity.cpp:12: td <= temperature ? td : temperature -- log 0 and log of a negative give a NaN td, which fails the comparison"""
    assert R.dewpoint(280, 0) == F(280) and R.dewpoint(280, -0.5) == F(280)
    assert R.dewpoint(293.15, 1) == F(293.15)          # td comes out a hair above: the temperature caps it
    assert R.dewpoint(293.15, 1.2) == F(293.15)        # supersaturated: capped as well
    assert np.isnan(R.dewpoint(np.inf, 0.5)) and np.isnan(R.dewpoint(280, np.nan))


def test_relative_humidity_table_rules():
    ewt = lambda i: F(R._EWT[i])
    assert R.relative_humidity(100, 100) == 1 and R.relative_humidity(250, 260) == 1      # :43-44 before anything else
    assert R.relative_humidity(170, 160) == 1                                              # both clamped to x = 0: mEwt[0] / mEwt[0]
    # x = 39 reads mEwt[39] and mEwt[40] with weight 0; 273.16 K is x = 20 exactly (float32(273.16) - 173.16 = 100.0000037, * 0.2 rounds to 20)
    assert R.relative_humidity(500, 273.16) == ewt(20) / ewt(39)
    assert R.relative_humidity(373.16, 363.16) == ewt(38) / ewt(39)
    # halfway between two entries: 275.66 K -> x = 20.5 (float32(275.66) = 275.66000366, x = 20.5000007 -> 20.500002 in float32)
    x = F((np.float64(F(275.66)) - 173.16) * 0.2)
    et = ewt(20) + (ewt(21) - ewt(20)) * (x - F(20))
    assert R.relative_humidity(500, 275.66) == et / ewt(39)
    assert 0 <= R.relative_humidity(300, 170) <= 1
    assert np.isnan(R.relative_humidity(np.inf, 280)) and np.isnan(R.relative_humidity(280, -np.inf))


def test_wetbulb_order_of_tests():
    assert np.isnan(R.wetbulb(30, 100000, 0.5))          # temperatureC <= -243.04
    assert np.isnan(R.wetbulb(280, 100000, 0)) and np.isnan(R.wetbulb(280, 100000, -1))
    assert np.isnan(R.wetbulb(np.nan, 100000, 0.5))      # a NaN fails both early tests and reaches the validity test
    assert np.isnan(R.wetbulb(280, np.inf, 0.5))
    # gamma + delta == 0 needs pressure 0 and a vapour pressure that underflows; log 0 has made Td NaN by then: NaN either way
    assert np.isnan(R.wetbulb(200, 0, 1e-45))
    assert np.isfinite(R.wetbulb(273.15, 0, 0.5))        # pressure 0 alone is fine: gamma = 0, the result is Td


def test_pressure_has_no_guards():
    assert np.isnan(R.pressure(0, 0, 101325, 0)) and np.isnan(R.pressure(0, 0, 0, 0))     # -0 / 0
    assert R.pressure(0, 1000, 0) == 0 and R.pressure(0, 0, 0) == 0
    assert R.pressure(10, 10, 12345.0, 250) == F(12345.0)
    assert R.pressure(0, 1000, 101325, 0) == 0           # -x / 0 = -inf, exp = 0
    assert R.pressure(1000, 0, 101325, 0) == np.inf


def test_qnh_zero_pressure_comes_first():
    assert R.qnh(0, np.nan) == 0 and R.qnh(0, np.inf) == 0 and R.qnh(-0.0, 100) == 0
    assert np.isnan(R.qnh(-1, 0)) and np.isnan(R.qnh(-90000, 1000))      # pow of a negative base
    assert np.isnan(R.qnh(np.inf, 0))
    assert R.qnh(101325, 0) == F(101325)


def test_wind_has_no_validity_test():
    assert np.isnan(R.wind_speed(np.nan, 1)) and np.isnan(R.wind_direction(1, np.nan))
    assert R.wind_speed(np.inf, 0) == np.inf and R.wind_speed(3, 4) == 5
    assert R.wind_direction(0, 0) == 180                 # atan2(-0, -0) = -pi
    assert R.wind_direction(1, 0) == 270                 # -90 + 360
    d = R.wind_direction(0.0, -1)                        # atan2(-0, 1) = -0: not < 0, stays -0
    assert d == 0 and np.signbit(d)
    d = R.wind_direction(-0.0, -1)
    assert d == 0 and not np.signbit(d)


def test_sea_level_pressure_checks_and_their_order():
    code = lambda *a: int(R.sea_level_pressure(*a)[1])
    assert code(101325, np.nan, np.nan) == 1 and code(-1, np.inf, 290) == 1
    assert code(-1, 20, np.nan) == 2 and code(101325, 20, np.inf, 2) == 2
    for args in ((-1, 20, 290), (101325, 20, -1), (101325, 20, 290, -0.1), (101325, 20, 290, 1.5), (101325, 20, 290, 0.5, -1), (101325, 20, 290, np.inf)):
        assert code(*args) == 3
    # made on the inputs as given: 0.5 K and 0.5 Pa pass, NaNs pass the third test
    assert code(0.5, 20, 0.5) == 0 and code(np.nan, 20, 290, np.nan, np.nan) == 0
    assert np.isnan(R.sea_level_pressure(np.nan, 20, 290)[0])
    assert code(101325, 20, 290, 0, 0) == 0 and code(101325, 20, 290, 1, 0) == 0


def test_sea_level_pressure_branches_by_hand():
    """the three humidity branches and the two altitude branches in plain double arithmetic (the float32 roundings of a dozen steps
    stay below 1e-6 relative)"""
    def by_hand(ps, alt, t, rh=None, dew=None):
        T, Ts, e = t - 273.15, t, 0.0
        ps *= 0.01
        if rh is not None:
            e = rh * 6.11 * 10 ** (7.5 * T / (237.3 + T))
            dewc = 243.04 * math.log(e / 6.1094) / (17.625 - math.log(e / 6.1094))
        elif dew is not None:
            dewc = dew - 273.15
            e = 6.11 * 10 ** (7.5 * dewc / (237.3 + dewc))
        else:
            dewc = T - 3
        if alt >= 50:
            return 100 * ps * math.exp((9.80665 * alt / 287.05) / (Ts + 0.5 * 0.0065 * alt + e * 0.12))
        tv = (273.15 + T) / (1 - 0.379 * (6.11 * 10 ** (7.5 * dewc / (237.7 + dewc)) / ps))
        return 100 * (ps + ps * alt / (29.27 * tv))
    for alt in (-20.0, 0.0, 49.9, 50.0, 800.0):
        for kw in ({}, {"rh": 0.6}, {"dew": 278.0}):
            got = R.sea_level_pressure(98000.0, alt, 285.0, kw.get("rh", np.nan), kw.get("dew", np.nan))[0]
            assert abs(got - by_hand(98000.0, alt, 285.0, **kw)) < 1e-6 * got, (alt, kw)
    # both given: the relative humidity wins (:52, :60)
    assert R.sea_level_pressure(98000, 800, 285, 0.6, 250)[0] == R.sea_level_pressure(98000, 800, 285, 0.6)[0]
    # 237.3 in the vapour pressure, 237.7 in the virtual temperature: the two low-altitude results differ from a 237.3-only formula
    assert R.sea_level_pressure(98000, 20, 285, np.nan, 278)[0] != R.sea_level_pressure(98000, 20, 285)[0]


def test_log_tests_only_the_validity():
    assert R.Log().forward(0) == -np.inf and np.isnan(R.Log().forward(-1))
    assert np.isnan(R.Log().forward(np.inf)) and np.isnan(R.Log().backward(-np.inf))
    assert R.Log().backward(0) == 1 and R.Log().backward(1000) == np.inf


def test_boxcox_quirks():
    b = R.BoxCox(0.1)
    assert b.forward(-5) == b.forward(0) == F(-10)       # value <= 0 -> 0 first; (0 - 1) / 0.1f rounds to -10
    assert b.backward(-20) == 0 and b.backward(-10) == 0      # clamped to float32(-1.0 / 0.1f) = -10: 1 + 0.1f * -10 = 0
    assert b.backward(0) == 1
    z = R.BoxCox(0)
    assert z.forward(1) == 0 and abs(z.forward(math.e) - 1) < 1e-7 and z.forward(0) == -np.inf and z.forward(-3) == -np.inf
    assert z.backward(0) == 1 and z.backward(-1000) == 0
    n = R.BoxCox(-0.5)                                   # no validation of the threshold
    assert n.forward(4) == F(1) and n.forward(0) == -np.inf       # (4^-0.5 - 1) / -0.5 = 1;  (inf - 1) / -0.5
    assert n.backward(0) == np.inf                       # below -1.0 / -0.5 = 2: clamped, 1 - 0.5 * 2 = 0, 0^-2
    assert n.backward(5) == F((1 - 2.5) ** -2)
    assert np.isnan(R.BoxCox(np.nan).forward(2))


def test_started_boxcox_quirks():
    for bad in (0, -1, np.nan, np.inf):
        with pytest.raises(ValueError, match="threshold parameter must be > 0 in the started Box-Cox distribution"):
            R.StartedBoxCox(bad, 1)
        with pytest.raises(ValueError, match="Scaling factor parameter must be > 0 in the started Box-Cox distribution"):
            R.StartedBoxCox(0.5, bad)
    with pytest.raises(ValueError, match="threshold parameter"):   # the threshold is tested first
        R.StartedBoxCox(0, 0)
    s = R.StartedBoxCox(0.5, 2)
    assert s.forward(-3) == 0 and s.forward(1.25) == F(1.25) and s.forward(2) == 2
    assert s.forward(8) == F(2 * (1 + (2.0 - 1) / 0.5))  # (8 / 2)^0.5 = 2
    assert s.backward(-1) == 0 and s.backward(1.25) == F(1.25)
    assert s.backward(6) == F(8)                         # 2 * (1 + 0.25 * 4)^2
    assert np.isnan(s.forward(np.nan)) and np.isnan(s.backward(np.inf))


def test_the_base_class_returns_minus_one():
    assert R.Transform().forward(3.0) == -1 and R.Transform().backward(np.nan) == -1
    assert np.all(R.Transform().forward(np.zeros((2, 3))) == -1)


def test_mismatches_is_the_measure_the_issue_states():
    a = np.array([np.nan, np.inf, -np.inf, 0.0, 1.0, 1.0, np.inf, 1.0, np.nan], F)
    b = np.array([np.nan, np.inf, -np.inf, -0.0, 1.000005, 1.00002, -np.inf, np.nan, 1.0], F)
    assert list(R.mismatches(a, b, R.RTOL)) == [5, 6, 7, 8]
    assert list(R.mismatches(a, b, 0)) == [4, 5, 6, 7, 8]
