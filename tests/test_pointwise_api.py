"""CPU: the weather diagnostics and the value transforms through `import gridpp` without a GPU -- names, argument names and defaults,
the constants, every known answer of the reference's tests through the host-only scalar forms, 20 000 seeded scalar cases per function
against the numpy restatement (tests/pointwise_ref.py; the scalar forms compile the per-value source of the kernels), every ValueError
text, the three messages of sea_level_pressure and their order, the constructor errors of StartedBoxCox, the empty shapes, "no HIP
device" for a real vector call where no GPU is visible, the constants of include/gridpp_hip.h against their Python mirror, and the
declarations of gridpp_amd/host/gridpp.hpp.

Tolerance: bit for bit for Identity, wind_speed and relative_humidity (no transcendental: the same IEEE operations in the same order);
1e-5 relative for the rest (pointwise_ref.RTOL: NaN matches NaN, infinities by sign, -0.0 equals 0), BoxCox.forward near an input of 1
on the power it computed (pointwise_ref.transform_mismatches)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import pointwise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = R.pins()
NCASES = 20000
F = np.float32


@pytest.fixture(scope="module")
def gridpp():
    import __graft_entry__ as g
    g.build()
    import gridpp
    assert gridpp.implementation == "gridpp_amd"
    return gridpp


@pytest.fixture(scope="module")
def lib(gridpp):
    from gridpp_amd import _capi
    return _capi.lib()


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def _id(c):
    return "%s%s@%s" % (c.get("fn") or c["transform"] + "." + c["direction"], c.get("args", c.get("input")), c["source"].split("/")[-1])


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_names_arguments_and_defaults(gridpp):
    """include/gridpp.h:1249-1367"""
    import gridpp_amd
    want = {"dewpoint": ["temperature", "relative_humidity"], "relative_humidity": ["temperature", "dewpoint"],
            "wetbulb": ["temperature", "pressure", "relative_humidity"], "pressure": ["ielev", "oelev", "ipressure", "itemperature"],
            "sea_level_pressure": ["ps", "altitude", "temperature", "rh", "dewpoint"], "qnh": ["pressure", "altitude"],
            "wind_speed": ["xwind", "ywind"], "wind_direction": ["xwind", "ywind"]}
    assert set(want) == set(R.DIAGNOSTICS)
    for name, params in want.items():
        assert getattr(gridpp, name) is getattr(gridpp_amd, name)
        sig = inspect.signature(getattr(gridpp, name))
        assert list(sig.parameters) == params and len(params) == R.DIAGNOSTICS[name]
        defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
        if name == "pressure":
            assert defaults == {"itemperature": 288.15}
        elif name == "sea_level_pressure":
            assert list(defaults) == ["rh", "dewpoint"] and all(np.isnan(v) for v in defaults.values())
        else:
            assert defaults == {}
    for name, params in (("Transform", []), ("Identity", []), ("Log", []), ("BoxCox", ["threshold"]), ("StartedBoxCox", ["threshold", "scaling_factor"])):
        cls = getattr(gridpp, name)
        assert issubclass(cls, gridpp.Transform)
        assert list(inspect.signature(cls).parameters) == params
        assert list(inspect.signature(cls.forward).parameters) == ["self", "input"] and list(inspect.signature(cls.backward).parameters) == ["self", "input"]
    for missing in ("Gamma", "gamma_inv", "metric_optimizer_curve", "get_optimal_threshold", "local_distribution_correction"):
        assert not hasattr(gridpp, missing)   # outside the scope: not even as stubs


def test_constants(gridpp):
    """include/gridpp.h:49-67: `static const float`, so the float32 value"""
    want = {"MV_CML": -999, "pi": 3.14159265, "lapse_rate": 0.0065, "standard_surface_temperature": 288.15, "gravit": 9.80665,
            "molar_mass": 0.0289644, "gas_constant_mol": 8.31447, "gas_constant_si": 287.05}
    for name, value in want.items():
        got = getattr(gridpp, name)
        assert isinstance(got, float) and got == float(F(value)), name
    assert np.isnan(gridpp.MV) and gridpp.radius_earth == 6.378137e6


def test_header_constants_follow_their_python_mirror(gridpp):
    from gridpp_amd import _capi
    text = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (GPP_(?:POINTWISE|TRANSFORM|DIAG)_[A-Z_]+) (\d+)", text)}
    assert defs == {"GPP_POINTWISE_BLOCK": _capi.POINTWISE_BLOCK, "GPP_POINTWISE_MAX_BLOCKS": _capi.POINTWISE_MAX_BLOCKS,
                    "GPP_TRANSFORM_IDENTITY": _capi.TRANSFORM_IDENTITY, "GPP_TRANSFORM_LOG": _capi.TRANSFORM_LOG,
                    "GPP_TRANSFORM_BOXCOX": _capi.TRANSFORM_BOXCOX, "GPP_TRANSFORM_STARTED_BOXCOX": _capi.TRANSFORM_STARTED_BOXCOX,
                    "GPP_DIAG_DEWPOINT": _capi.DIAG_DEWPOINT, "GPP_DIAG_RELATIVE_HUMIDITY": _capi.DIAG_RELATIVE_HUMIDITY,
                    "GPP_DIAG_WETBULB": _capi.DIAG_WETBULB, "GPP_DIAG_PRESSURE": _capi.DIAG_PRESSURE,
                    "GPP_DIAG_SEA_LEVEL_PRESSURE": _capi.DIAG_SEA_LEVEL_PRESSURE, "GPP_DIAG_QNH": _capi.DIAG_QNH,
                    "GPP_DIAG_WIND_SPEED": _capi.DIAG_WIND_SPEED, "GPP_DIAG_WIND_DIRECTION": _capi.DIAG_WIND_DIRECTION}
    assert _capi.POINTWISE_BLOCK % 64 == 0
    for name in R.DIAGNOSTICS:   # every entry cites the lines it replaces
        assert re.search(r"/\* gridpp::%s[^\n]*\(src/api/\w+\.cpp:\d+-\d+\)" % name.replace("wind_direction", "wind_speed / wind_direction"), text), name


# ---- the pins through the scalar forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PINS["diagnostics"], ids=_id)
def test_diagnostic_pins_scalar(gridpp, case):
    fn, args = getattr(gridpp, case["fn"]), R.nan_of(case["args"])
    if "raises" in case:
        with pytest.raises(RuntimeError, match="sea_level_pressure: "):
            fn(*args)
        return
    got = fn(*args)
    assert isinstance(got, float)
    assert R.within_decimals(got, R.nan_of(case["expected"]), case["decimals"]), (got, case)


@pytest.mark.parametrize("case", PINS["transforms"], ids=_id)
def test_transform_pins_scalar(gridpp, case):
    t, x = getattr(gridpp, case["transform"])(*case["params"]), R.nan_of(case["input"])
    got = t.backward(t.forward(x)) if case["direction"] == "roundtrip" else getattr(t, case["direction"])(x)
    assert isinstance(got, float)
    assert R.within_decimals(got, R.nan_of(case["expected"]), case["decimals"]), (got, case)


def test_the_two_exact_pins_are_exact(gridpp):
    assert gridpp.sea_level_pressure(101325.0, 20, 273.15) == 101578.0
    assert gridpp.sea_level_pressure(101325.0, 50, 273.15) == 101960.25


def test_base_class_scalars_return_minus_one(gridpp):
    assert gridpp.Transform().forward(3.5) == -1 and gridpp.Transform().backward(np.nan) == -1


# ---- seeded scalar cases against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in R.DIAGNOSTICS if n != "sea_level_pressure"])
def test_seeded_scalars_against_the_restatement(gridpp, name):
    args = R.seeded_inputs(name, NCASES)
    want = getattr(R, name)(*args)
    fn = getattr(gridpp, name)
    got = np.array([fn(*row) for row in zip(*[a.tolist() for a in args])], F)
    bad = R.mismatches(got, want, 0 if name in R.EXACT else R.RTOL)
    print("%s: %d of %d scalar cases not bit-identical to the restatement" % (name, R.bit_differences(got, want), NCASES))
    assert bad.size == 0, (name, [(tuple(a[i] for a in args), got[i], want[i]) for i in bad[:5]])


def test_seeded_scalars_sea_level_pressure(gridpp):
    """values where the reference returns one, the message of the reference's first failing test where it throws"""
    args = R.seeded_inputs("sea_level_pressure", NCASES)
    want, codes = R.sea_level_pressure(*args)
    assert set(np.unique(codes)) == {0, 1, 2, 3}
    got = np.full(NCASES, np.nan, F)
    for i, row in enumerate(zip(*[a.tolist() for a in args])):
        if codes[i] == 0:
            got[i] = gridpp.sea_level_pressure(*row)
        else:
            with pytest.raises(RuntimeError) as e:
                gridpp.sea_level_pressure(*row)
            assert str(e.value) == R.SLP_MESSAGES[int(codes[i])], row
    bad = R.mismatches(got, want, R.RTOL)
    print("sea_level_pressure: %d of %d scalar cases not bit-identical to the restatement" % (R.bit_differences(got, want), NCASES))
    assert bad.size == 0, [(tuple(a[i] for a in args), got[i], want[i]) for i in bad[:5]]


@pytest.mark.parametrize("direction", ["forward", "backward"])
@pytest.mark.parametrize("tid,cls,params", R.transforms(), ids=[t[0] for t in R.transforms()])
def test_seeded_transform_scalars_against_the_restatement(gridpp, tid, cls, params, direction):
    values = R.seeded_values(direction, NCASES)
    want = getattr(getattr(R, cls)(*params), direction)(values)
    fn = getattr(getattr(gridpp, cls)(*params), direction)
    got = np.array([fn(v) for v in values.tolist()], F)
    bad = R.transform_mismatches(tid, direction, values, got, want)
    print("%s.%s: %d of %d scalar cases not bit-identical to the restatement" % (tid, direction, R.bit_differences(got, want), NCASES))
    assert bad.size == 0, (tid, direction, [(values[i], got[i], want[i]) for i in bad[:5]])


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_value_error_texts(gridpp):
    """the reference's std::invalid_argument texts, before any device work"""
    one, two = [280.0], [280.0, 281.0]
    cases = [(gridpp.dewpoint, (one, two), "Temperature and relative_humidity vectors are not the same size"),
             (gridpp.relative_humidity, (one, two), "Temperature and dewpoint vectors are not the same size"),
             (gridpp.wetbulb, (one, two, one), "Temperature and pressure vectors are not the same size"),
             (gridpp.wetbulb, (one, one, two), "Temperature and relative_humidity vectors are not the same size"),
             (gridpp.wetbulb, (one, two, two), "Temperature and pressure vectors are not the same size"),   # humidity.cpp:111-114: in that order
             (gridpp.qnh, (one, two), "Pressure and altitude vectors are not the same size"),
             (gridpp.wind_speed, (one, two), "xwind and ywind must be of the same size"),
             (gridpp.wind_direction, (two, one), "xwind and ywind must be of the same size"),
             (gridpp.wind_speed, ([], two), "xwind and ywind must be of the same size"),
             (gridpp.wind_direction, (one, []), "xwind and ywind must be of the same size")]
    for k in range(4):
        args = [one] * 4
        args[k] = two
        cases.append((gridpp.pressure, tuple(args), "pressure: Input arguments must be of the same size"))
    for k in range(5):
        args = [one] * 5
        args[k] = two
        cases.append((gridpp.sea_level_pressure, tuple(args), "slp: Input arguments must be of the same size"))
    for fn, args, message in cases:
        with pytest.raises(ValueError) as e:
            fn(*args)
        assert str(e.value) == message


def test_wrong_dimensions_raise_like_the_typemap(gridpp):
    with pytest.raises(RuntimeError):
        gridpp.dewpoint(np.zeros((2, 2)), np.zeros((2, 2)))
    with pytest.raises(RuntimeError):
        gridpp.qnh([101325.0], 0.0)          # a scalar beside a vector matches no overload
    with pytest.raises(RuntimeError):
        gridpp.pressure([0.0], [0.0], [101325.0])   # the default belongs to the scalar overload only
    with pytest.raises(RuntimeError):
        gridpp.sea_level_pressure([101325.0], [20.0], [290.0])
    with pytest.raises(RuntimeError):
        gridpp.Identity().forward(np.zeros((1, 1, 1, 1)))


def test_sea_level_pressure_messages_and_their_order(gridpp):
    nan = np.nan
    for args, message in (((101325, nan, 290), "altitude is NAN"), ((101325, np.inf, nan, 2, -1), "altitude is NAN"), ((-1, nan, nan), "altitude is NAN"),
                          ((101325, 20, nan), "temperature is NAN"), ((-1, 20, -np.inf, 2), "temperature is NAN"),
                          ((-1, 20, 290), "unphysical values in input"), ((101325, 20, -1), "unphysical values in input"),
                          ((101325, 20, 290, -0.1), "unphysical values in input"), ((101325, 20, 290, 1.1), "unphysical values in input"),
                          ((101325, 20, 290, 0.7, -1), "unphysical values in input")):
        with pytest.raises(RuntimeError) as e:
            gridpp.sea_level_pressure(*args)
        assert str(e.value) == "sea_level_pressure: " + message
    assert np.isnan(gridpp.sea_level_pressure(nan, 20, 290))   # a NaN pressure passes all three


def test_started_boxcox_constructor_errors(gridpp, lib):
    from gridpp_amd import _capi
    for bad in (0, -1, np.nan, np.inf):
        with pytest.raises(ValueError) as e:
            gridpp.StartedBoxCox(bad, 1)
        assert str(e.value) == "threshold parameter must be > 0 in the started Box-Cox distribution"
        with pytest.raises(ValueError) as e:
            gridpp.StartedBoxCox(0.5, bad)
        assert str(e.value) == "Scaling factor parameter must be > 0 in the started Box-Cox distribution"
        out = C.c_float(7)
        assert lib.gpp_transform_scalar(1.0, _capi.TRANSFORM_STARTED_BOXCOX, 0, bad, 1.0, C.byref(out)) == _capi.GPP_EINVAL
        assert "threshold parameter must be > 0" in lib.gpp_last_error().decode()
        a = np.ones(4, F)
        assert lib.gpp_transform(ptr(a), 4, _capi.TRANSFORM_STARTED_BOXCOX, 1, 0.5, bad, ptr(a), 0) == _capi.GPP_EINVAL
        assert "Scaling factor parameter must be > 0" in lib.gpp_last_error().decode()
    with pytest.raises(ValueError, match="threshold parameter"):
        gridpp.StartedBoxCox(0, 0)
    gridpp.BoxCox(-1), gridpp.BoxCox(np.nan)   # transform.cpp:97-99: no validation


def test_c_abi_checks_before_device_work(lib):
    from gridpp_amd import _capi
    a, out = np.ones(8, F), np.full(8, 7, F)
    for kind in (-1, 4, 99):
        assert lib.gpp_transform(ptr(a), 8, kind, 0, 0.1, 1.0, ptr(out), 0) == _capi.GPP_EINVAL
        assert lib.gpp_transform_scalar(1.0, kind, 0, 0.1, 1.0, C.byref(C.c_float())) == _capi.GPP_EINVAL
    # n == 0: GPP_OK, nothing written, no pointer looked at
    assert lib.gpp_transform(None, 0, _capi.TRANSFORM_LOG, 0, 0, 0, None, 0) == _capi.GPP_OK
    assert lib.gpp_dewpoint(None, None, 0, None, 0) == _capi.GPP_OK and lib.gpp_wetbulb(ptr(a), ptr(a), ptr(a), 0, ptr(out), 0) == _capi.GPP_OK
    assert lib.gpp_sea_level_pressure(None, None, None, None, None, 0, None, 0) == _capi.GPP_OK
    assert lib.gpp_qnh(ptr(a), ptr(a), -1, ptr(out), 0) == _capi.GPP_EINVAL
    assert lib.gpp_wind_speed(ptr(a), None, 8, ptr(out), 0) == _capi.GPP_EINVAL and "NULL" in lib.gpp_last_error().decode()
    assert np.all(out == 7)
    vals = (C.c_float * 5)(101325, 20, 290, np.nan, np.nan)
    res = C.c_float(7)
    assert lib.gpp_diagnostic_scalar(_capi.DIAG_SEA_LEVEL_PRESSURE, vals, 4, C.byref(res)) == _capi.GPP_EINVAL   # a wrong nargs
    assert lib.gpp_diagnostic_scalar(8, vals, 2, C.byref(res)) == _capi.GPP_EINVAL and lib.gpp_diagnostic_scalar(-1, vals, 2, C.byref(res)) == _capi.GPP_EINVAL
    vals[1] = np.nan
    assert lib.gpp_diagnostic_scalar(_capi.DIAG_SEA_LEVEL_PRESSURE, vals, 5, C.byref(res)) == _capi.GPP_ERUNTIME
    assert lib.gpp_last_error().decode() == "sea_level_pressure: altitude is NAN" and res.value == 7


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------
def test_empty_inputs_without_a_device(gridpp):
    for name, nin in R.DIAGNOSTICS.items():
        for empty in ([], np.zeros(0), np.zeros(0, F)):
            out = getattr(gridpp, name)(*([empty] * nin))
            assert isinstance(out, np.ndarray) and out.dtype == F and out.shape == (0,)
    transforms = [gridpp.Transform(), gridpp.Identity(), gridpp.Log(), gridpp.BoxCox(0.1), gridpp.StartedBoxCox(0.3, 2.5)]
    shapes = [((0,), (0,)), ((0, 0), (0, 0)), ((0, 3, 3), (0, 0, 0)), ((0, 0, 5), (0, 0, 0)), ((2, 0, 3), (2, 0, 0))]
    shapes += [(tuple(s["input"]), tuple(s["output"])) for s in PINS["empty_shapes"]]
    for t in transforms:
        for shape, want in shapes:
            for out in (t.forward(np.zeros(shape)), t.backward(np.zeros(shape, F))):
                assert isinstance(out, np.ndarray) and out.dtype == F and out.shape == want, (shape, out.shape)


def test_a_real_vector_call_fails_loudly_without_a_gpu(gridpp, lib):
    """no CPU path behind the vector forms: "no HIP device" where none is visible (where one is, the call simply works)"""
    from gridpp_amd import _capi
    calls = [lambda: gridpp.dewpoint([293.15], [0.8]), lambda: gridpp.relative_humidity([293.15], [280.0]), lambda: gridpp.wetbulb([270], [1e5], [0.8]),
             lambda: gridpp.pressure([0], [1000], [101325], [288.15]), lambda: gridpp.sea_level_pressure([101325], [20], [273.15], [np.nan], [np.nan]),
             lambda: gridpp.qnh([90000], [1000]), lambda: gridpp.wind_speed([3], [4]), lambda: gridpp.wind_direction([1], [0]),
             lambda: gridpp.Identity().forward([1.0]), lambda: gridpp.Log().backward(np.ones((2, 2))), lambda: gridpp.BoxCox(0.1).forward(np.ones((2, 2, 2))),
             lambda: gridpp.StartedBoxCox(0.3, 2.5).backward([1.0, 2.0])]
    if gridpp.device_count() > 0:
        assert gridpp.wind_speed([3], [4])[0] == 5 and gridpp.Identity().forward([1.0])[0] == 1
        return
    for call in calls:
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
    a, out = np.ones(8, F), np.zeros(8, F)
    assert lib.gpp_qnh(ptr(a), ptr(a), 8, ptr(out), 0) == _capi.GPP_ENODEVICE
    assert lib.gpp_transform(ptr(a), 8, _capi.TRANSFORM_LOG, 0, 0, 0, ptr(out), 0) == _capi.GPP_ENODEVICE


def test_mixed_host_and_device_arguments_are_refused(gridpp):
    class FakeTensor:   # what _mem looks at
        is_cuda = True

        def data_ptr(self):
            return 0

        def dim(self):
            return 1
    with pytest.raises(ValueError, match="either all field arguments are torch CUDA tensors or none is"):
        gridpp.wind_speed(FakeTensor(), [1.0])


# ---- the C++ mirror -----------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_declarations():
    hpp = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp.hpp")).read()
    for decl in ("inline float dewpoint(float temperature, float relative_humidity)", "inline vec dewpoint(const vec& temperature, const vec& relative_humidity)",
                 "inline float relative_humidity(float temperature, float dewpoint)", "inline vec relative_humidity(const vec& temperature, const vec& dewpoint)",
                 "inline float wetbulb(float temperature, float pressure, float relative_humidity)",
                 "inline vec wetbulb(const vec& temperature, const vec& pressure, const vec& relative_humidity)",
                 "inline float pressure(float ielev, float oelev, float ipressure, float itemperature = 288.15)",
                 "inline vec pressure(const vec& ielev, const vec& oelev, const vec& ipressure, const vec& itemperature)",
                 "inline float sea_level_pressure(float ps, float altitude, float temperature, float rh = MV, float dewpoint = MV)",
                 "inline vec sea_level_pressure(const vec& ps, const vec& altitude, const vec& temperature, const vec& rh, const vec& dewpoint)",
                 "inline float qnh(float pressure, float altitude)", "inline vec qnh(const vec& pressure, const vec& altitude)",
                 "inline float wind_speed(float xwind, float ywind)", "inline vec wind_speed(const vec& xwind, const vec& ywind)",
                 "inline float wind_direction(float xwind, float ywind)", "inline vec wind_direction(const vec& xwind, const vec& ywind)",
                 "class Transform {", "class Identity : public Transform {", "class Log : public Transform {", "class BoxCox : public Transform {",
                 "class StartedBoxCox : public Transform {", "BoxCox(float threshold)", "StartedBoxCox(float threshold, float scaling_factor)",
                 "virtual float forward(float value) const", "virtual float backward(float value) const",
                 "vec forward(const vec& input) const", "vec2 backward(const vec2& input) const", "vec3 forward(const vec3& input) const",
                 "static const float MV_CML = -999;", "static const float pi = 3.14159265;", "static const float lapse_rate = 0.0065;",
                 "static const float standard_surface_temperature = 288.15;", "static const float gravit = 9.80665;",
                 "static const float molar_mass = 0.0289644;", "static const float gas_constant_mol = 8.31447;", "static const float gas_constant_si = 287.05;"):
        assert decl in hpp, decl
    for message in ("Temperature and relative_humidity vectors are not the same size", "Temperature and dewpoint vectors are not the same size",
                    "Temperature and pressure vectors are not the same size", "pressure: Input arguments must be of the same size",
                    "slp: Input arguments must be of the same size", "Pressure and altitude vectors are not the same size",
                    "xwind and ywind must be of the same size", "threshold parameter must be > 0 in the started Box-Cox distribution",
                    "Scaling factor parameter must be > 0 in the started Box-Cox distribution"):
        assert 'std::invalid_argument("%s")' % message in hpp, message
    assert "class Gamma" not in hpp and "gamma_inv" not in hpp
