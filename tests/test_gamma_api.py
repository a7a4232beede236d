"""CPU: gamma_inv and the Gamma transform through `import gridpp_amd` without a GPU -- names, argument names and the default tolerance,
their absence from the `gridpp` alias, the constructor messages, the reference's known answers and the whole golden file
(tests/golden/gamma_cases.npz, mpmath) through the two host-only scalar entries, 20 000 seeded scalar cases per function against the scipy
restatement (tests/gamma_ref.py; the scalar forms compile the per-value source of the kernels), every gamma_inv message with its formatted
value and the order of the three checks, unequal lengths, the empty shapes, 4-D input, "no HIP device" for a real vector call where no GPU
is visible, and the header's constants and declarations against the Python mirror and gridpp_gamma.hpp.

The lowest offending index of SEVERAL elements is the kernel's to find (the status word): tests/test_gpu_gamma_parity.py.
Tolerance: the rule of tests/gamma_ref.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import gamma_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCASES = 20000
F = np.float32


@pytest.fixture(scope="module")
def amd():
    import __graft_entry__ as g
    g.build()
    import gridpp_amd
    return gridpp_amd


@pytest.fixture(scope="module")
def lib(amd):
    from gridpp_amd import _capi
    return _capi.lib()


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def scalar_gamma_inv(lib, level, shape, scale):
    out = np.empty(len(level), F)
    res = C.c_float()
    for i, (lv, a, s) in enumerate(zip(level, shape, scale)):
        assert lib.gpp_gamma_inv_scalar(float(lv), float(a), float(s), C.byref(res)) == 0, lib.gpp_last_error()
        out[i] = res.value
    return out


def scalar_transform(lib, values, backward, params):
    out = np.empty(len(values), F)
    res = C.c_float()
    p = [float(v) for v in params]
    for i, v in enumerate(values):
        assert lib.gpp_gamma_transform_scalar(float(v), backward, p[0], p[1], p[2], C.byref(res)) == 0, lib.gpp_last_error()
        out[i] = res.value
    return out


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_names_arguments_and_defaults(amd):
    """include/gridpp.h:573,2438-2455 of the reference"""
    assert list(inspect.signature(amd.gamma_inv).parameters) == ["levels", "shape", "scale"]
    sig = inspect.signature(amd.Gamma)
    assert list(sig.parameters) == ["shape", "scale", "tolerance"]
    assert {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == {"tolerance": 0.01}
    assert issubclass(amd.Gamma, amd.Transform)
    assert list(inspect.signature(amd.Gamma.forward).parameters) == ["self", "input"] and list(inspect.signature(amd.Gamma.backward).parameters) == ["self", "input"]
    assert "ValueError" in amd.gamma_inv.__doc__ and "unequal lengths" in amd.gamma_inv.__doc__


def test_the_alias_does_not_carry_them(amd):
    """the edges return IEEE values where the reference raises: a script written for the reference asks for them by gridpp_amd's name"""
    import gridpp
    assert gridpp.implementation == "gridpp_amd"
    assert not hasattr(gridpp, "Gamma") and not hasattr(gridpp, "gamma_inv")
    assert gridpp.BoxCox is amd.BoxCox
    hpp = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp.hpp")).read()
    assert "class Gamma" not in hpp and "gamma_inv" not in hpp


def test_constructor_messages(amd, lib):
    """transform.cpp:158-163, tested on the float32 values"""
    from gridpp_amd import _capi
    texts = ("Shape parameter must be > 0 in the gamma distribution", "Scale parameter must be > 0 in the gamma distribution",
             "Tolerance must be >= 0 in the gamma distribution")
    a, res = np.ones(4, F), C.c_float(7)
    for bad in (-1, 0, np.nan, np.inf, 1e-60):   # 1e-60 is 0 as a float32
        for k in (0, 1):
            args = [1, 2, 0.01]
            args[k] = bad
            with pytest.raises(ValueError) as e:
                amd.Gamma(*args)
            assert str(e.value) == texts[k]
            assert lib.gpp_gamma_transform_scalar(1.0, 0, *[F(v) for v in args], C.byref(res)) == _capi.GPP_EINVAL
            assert lib.gpp_last_error().decode() == texts[k] and res.value == 7
            assert lib.gpp_gamma_transform(ptr(a), 4, 1, *[F(v) for v in args], ptr(a), 0) == _capi.GPP_EINVAL
            assert lib.gpp_last_error().decode() == texts[k]
    for bad in (-1, np.nan, -np.inf):
        with pytest.raises(ValueError) as e:
            amd.Gamma(1, 2, bad)
        assert str(e.value) == texts[2]
        assert lib.gpp_gamma_transform_scalar(1.0, 0, 1, 2, F(bad), C.byref(res)) == _capi.GPP_EINVAL and lib.gpp_last_error().decode() == texts[2]
    with pytest.raises(ValueError, match="Shape parameter"):   # the order of the three checks
        amd.Gamma(0, 0, -1)
    with pytest.raises(ValueError, match="Scale parameter"):
        amd.Gamma(1, 0, -1)
    amd.Gamma(1, 2, 0)   # tests/test_transform.py:96-97 of the reference
    assert amd.Gamma(1, 2).forward(0.0) == amd.Gamma(1, 2, 0.01).forward(0.0) != amd.Gamma(1, 2, 0).forward(0.0)


# ---- the reference's known answers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,want", R.PINS_GAMMA_INV)
def test_gamma_inv_pins(amd, args, want):
    """tests/test_distribution.py:11-16 of the reference"""
    got = amd.gamma_inv(*args)
    assert isinstance(got, float) and abs(got - want) < 1.5 * 10 ** -R.PIN_DECIMALS


@pytest.mark.parametrize("direction,value,want", R.PINS_TRANSFORM)
def test_transform_pins(amd, direction, value, want):
    """tests/test_transform.py:67-75 of the reference"""
    got = getattr(amd.Gamma(1, 2, 0.01), direction)(value)
    assert isinstance(got, float) and abs(got - want) < 1.5 * 10 ** -R.PIN_DECIMALS


def test_edges_return_ieee_values(amd):
    """where the reference raises (Boost's policies) and where it returns the missing value"""
    g = amd.Gamma(1, 2, 0.01)
    for bad in (np.nan, np.inf, -np.inf):
        assert np.isnan(g.forward(bad)) and np.isnan(g.backward(bad))
    assert np.isnan(g.forward(-0.02)) and g.forward(-0.01) == -np.inf and np.isfinite(g.forward(-0.005))   # x = value + tolerance: < 0, 0, > 0
    assert g.forward(40.0) == np.inf and g.forward(35.0) == np.inf and np.isfinite(g.forward(30.0))
    assert amd.Gamma(1, 2, 0).forward(0.0) == -np.inf
    assert np.isfinite(g.backward(5.4)) and g.backward(5.5) == np.inf
    assert g.backward(-14.5) == float(F(-F(0.01))) and amd.Gamma(1, 2, 0).backward(-15.0) == 0.0
    assert amd.gamma_inv(0.0, 1.0, 2.0) == 0.0 and amd.gamma_inv(1.0, 1.0, 2.0) == np.inf


# ---- the golden file and the seeded soaks through the scalar forms -----------------------------------------------------------------------------
def test_golden_gamma_inv_scalar(lib):
    g = R.golden()
    got = scalar_gamma_inv(lib, g.gi_level, g.gi_shape, g.gi_scale)
    idx = R.mismatches(got, g.gi_want)
    assert len(idx) == 0, R.report(idx, got, g.gi_want, g.gi_level, g.gi_shape, g.gi_scale)
    assert len(got) > 1500 and np.sum(np.abs(g.gi_want) < R.TINY) > 20 and np.isinf(g.gi_want).any()


def test_golden_transform_scalar(lib):
    g = R.golden()
    total = 0
    for params, values, want, neighbours in g.forward_sets():
        got = scalar_transform(lib, values, 0, params)
        idx = R.mismatches(got, want, neighbours)
        assert len(idx) == 0, "forward %s: %s" % (params, R.report(idx, got, want, values))
        total += len(values)
    for params, values, want in g.backward_sets():
        got = scalar_transform(lib, values, 1, params)
        idx = R.mismatches(got, want)
        assert len(idx) == 0, "backward %s: %s" % (params, R.report(idx, got, want, values))
        total += len(values)
    assert total == len(g.fw_in) + len(g.bw_in) > 1500


def test_seeded_gamma_inv_against_scipy(lib):
    r = R.restatement()
    level, shape, scale = R.seeded_gamma_inv(NCASES)
    got, want = scalar_gamma_inv(lib, level, shape, scale), r.gamma_inv(level, shape, scale)
    idx = R.mismatches(got, want)
    assert len(idx) == 0, R.report(idx, got, want, level, shape, scale)


def test_seeded_transform_against_scipy(lib):
    r = R.restatement()
    rng = np.random.default_rng(20240613)
    per = NCASES // 10
    for params in R.seeded_params(10):
        values = R.seeded_forward_inputs(params, per, rng)
        got, (want, lo, hi) = scalar_transform(lib, values, 0, params), r.forward(values, *params, neighbours=True)
        idx = R.mismatches(got, want, (lo, hi))
        assert len(idx) == 0, "forward %s: %s" % (params, R.report(idx, got, want, values))
        values = R.seeded_backward_inputs(per, rng)
        got, want = scalar_transform(lib, values, 1, params), r.backward(values, *params)
        idx = R.mismatches(got, want)
        assert len(idx) == 0, "backward %s: %s" % (params, R.report(idx, got, want, values))


def test_backward_undoes_forward_scalar(amd):
    """tests/test_transform.py:82-86 of the reference asks 5 decimals of backward(forward(x)) at 0 and 1.99 for Gamma(1, 2, 0.01); here 1e-5
    absolute over [0, 6] (why 6: tests/test_gpu_gamma_parity.py::test_backward_undoes_forward)"""
    g = amd.Gamma(1, 2, 0.01)
    for x in np.linspace(0, 6, 97).astype(F):
        assert abs(g.backward(g.forward(float(x))) - float(x)) <= 1e-5, x


# ---- the errors of gamma_inv --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,text", [
    ((-0.1, 1, 1), "Invalid level '-0.1'. Levels must be on the interval [0, 1]."),
    ((1.1, 1, 1), "Invalid level '1.1'. Levels must be on the interval [0, 1]."),
    ((np.nan, 1, 1), "Invalid level 'nan'. Levels must be on the interval [0, 1]."),
    ((np.inf, 1, 1), "Invalid level 'inf'. Levels must be on the interval [0, 1]."),
    ((1.0000001, 1, 1), "Invalid level '1'. Levels must be on the interval [0, 1]."),   # six significant digits, as an ostream prints
    ((-1e-30, 1, 1), "Invalid level '-1e-30'. Levels must be on the interval [0, 1]."),
    ((0.1, -1, 1), "Invalid shape '-1'. Shapes must be > 0."),
    ((0.1, 0, 1), "Invalid shape '0'. Shapes must be > 0."),
    ((0.1, np.nan, 1), "Invalid shape 'nan'. Shapes must be > 0."),
    ((0.1, np.inf, 1), "Invalid shape 'inf'. Shapes must be > 0."),
    ((0.1, 1, -2.5), "Invalid scale '-2.5'. Scale must be > 0."),
    ((0.1, 1, 0), "Invalid scale '0'. Scale must be > 0."),
    ((0.1, 1, -np.inf), "Invalid scale '-inf'. Scale must be > 0."),
    ((0.1, 1, -1234567.0), "Invalid scale '-1.23457e+06'. Scale must be > 0."),
    ((2, 0, 0), "Invalid level '2'. Levels must be on the interval [0, 1]."),           # level before shape before scale
    ((0.5, -3, 0), "Invalid shape '-3'. Shapes must be > 0."),
])
def test_gamma_inv_messages(amd, lib, args, text):
    """distribution.cpp:8-22: built on the C++ side, `ss << value` of a float"""
    from gridpp_amd import _capi
    with pytest.raises(ValueError) as e:
        amd.gamma_inv(*args)
    assert str(e.value) == text
    res = C.c_float(7)
    assert lib.gpp_gamma_inv_scalar(*[F(v) for v in args], C.byref(res)) == _capi.GPP_EINVAL and res.value == 7


def test_unequal_lengths(amd):
    for args in (([0.5], [1, 1], [1, 1]), ([0.5, 0.5], [1], [1, 1]), ([0.5, 0.5], [1, 1], [1]), ([], [1], [1]), (np.ones(3), np.ones(2, F), [1, 2, 3])):
        with pytest.raises(ValueError) as e:
            amd.gamma_inv(*args)
        assert str(e.value) == "gamma_inv: levels, shape and scale must be of the same size"
    with pytest.raises(RuntimeError, match="must have 1 dimensions"):
        amd.gamma_inv(np.ones((2, 2)), np.ones((2, 2)), np.ones((2, 2)))


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------
def test_empty_inputs_without_a_device(amd):
    for empty in ([], np.zeros(0), np.zeros(0, F)):
        out = amd.gamma_inv(empty, empty, empty)
        assert isinstance(out, np.ndarray) and out.dtype == F and out.shape == (0,)
    g = amd.Gamma(1, 2, 0.01)
    for shape, want in (((0,), (0,)), ((2, 0), (2, 0)), ((3, 3, 0), (3, 3, 0)), ((0, 1), (0, 0)), ((0, 3, 3), (0, 0, 0)), ((2, 0, 3), (2, 0, 0))):
        for out in (g.forward(np.zeros(shape)), g.backward(np.zeros(shape, F))):
            assert isinstance(out, np.ndarray) and out.dtype == F and out.shape == want, (shape, out.shape)


def test_four_dimensions_are_refused(amd):
    g = amd.Gamma(1, 2)
    for call in (g.forward, g.backward):
        with pytest.raises(RuntimeError, match="input must be a scalar or have 1, 2 or 3 dimensions, got 4"):
            call(np.zeros((2, 2, 2, 2)))


def test_a_real_vector_call_fails_loudly_without_a_gpu(amd, lib):
    """no CPU path behind the vector forms: "no HIP device" where none is visible (where one is, the call simply works)"""
    from gridpp_amd import _capi
    g = amd.Gamma(1, 2, 0.01)
    calls = [lambda: amd.gamma_inv([0.5], [1], [2]), lambda: g.forward([1.99]), lambda: g.backward(np.ones((2, 2))), lambda: g.forward(np.ones((2, 2, 2)))]
    if amd.device_count() > 0:
        assert abs(amd.gamma_inv([0.5], [1], [2])[0] - 1.38629) < 1e-5 and abs(g.forward([1.99])[0] - 0.33747494) < 1e-5
        return
    for call in calls:
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
    a, out = np.full(8, 0.5, F), np.zeros(8, F)
    assert lib.gpp_gamma_inv(ptr(a), ptr(a), ptr(a), 8, ptr(out), 0) == _capi.GPP_ENODEVICE
    assert lib.gpp_gamma_transform(ptr(a), 8, 0, 1, 2, 0.01, ptr(out), 0) == _capi.GPP_ENODEVICE


def test_c_abi_checks_before_device_work(lib):
    from gridpp_amd import _capi
    a, out = np.full(8, 0.5, F), np.full(8, 7, F)
    assert lib.gpp_gamma_inv(None, None, None, 0, None, 0) == _capi.GPP_OK and lib.gpp_gamma_transform(None, 0, 0, 1, 2, 0.01, None, 0) == _capi.GPP_OK
    assert lib.gpp_gamma_inv(ptr(a), ptr(a), ptr(a), -1, ptr(out), 0) == _capi.GPP_EINVAL
    assert lib.gpp_gamma_inv(ptr(a), None, ptr(a), 8, ptr(out), 0) == _capi.GPP_EINVAL and "NULL" in lib.gpp_last_error().decode()
    assert lib.gpp_gamma_transform(ptr(a), 8, 0, 1, 2, 0.01, None, 0) == _capi.GPP_EINVAL and "NULL" in lib.gpp_last_error().decode()
    assert lib.gpp_gamma_inv_scalar(0.5, 1, 2, None) == _capi.GPP_EINVAL and lib.gpp_gamma_transform_scalar(1, 0, 1, 2, 0.01, None) == _capi.GPP_EINVAL
    assert np.all(out == 7)


def test_mixed_host_and_device_arguments_are_refused(amd):
    class FakeTensor:   # what _mem looks at
        is_cuda = True

        def data_ptr(self):
            return 0

        def dim(self):
            return 1
    with pytest.raises(ValueError, match="either all field arguments are torch CUDA tensors or none is"):
        amd.gamma_inv(FakeTensor(), [1.0], [1.0])


# ---- the header, its Python mirror and the C++ header ---------------------------------------------------------------------------------------
def test_header_constants_and_declarations(amd):
    from gridpp_amd import _capi
    text = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (GPP_GAMMA_[A-Z_]+) (\d+)", text)}
    assert defs == {"GPP_GAMMA_BLOCK": _capi.GAMMA_BLOCK, "GPP_GAMMA_MAX_BLOCKS": _capi.GAMMA_MAX_BLOCKS}
    assert _capi.GAMMA_BLOCK % 64 == 0
    for decl in ("int gpp_gamma_inv(const float* levels, const float* shape, const float* scale, long long n, float* out, int mem);",
                 "int gpp_gamma_transform(const float* in, long long n, int backward, float shape, float scale, float tolerance, float* out, int mem);",
                 "int gpp_gamma_inv_scalar(float level, float shape, float scale, float* out);",
                 "int gpp_gamma_transform_scalar(float value, int backward, float shape, float scale, float tolerance, float* out);"):
        assert decl in text, decl
        at = text.index(decl)
        assert re.search(r"\(src/api/\w+\.cpp:\d+-\d+", text[text.rindex("/*", 0, at):at]), decl   # every entry cites the lines it replaces
    for name in ("gpp_gamma_inv", "gpp_gamma_transform", "gpp_gamma_inv_scalar", "gpp_gamma_transform_scalar"):
        assert name in _capi.SIGNATURES
    assert "gpp_gamma_inv for its three inputs" in text[text.index("With GPP_MEM_HOST"):text.index("#define GPP_HOST_F64")]
    assert text.count("int gpp_transform(") == 1 and "int gpp_transform(const float* in, long long n, int kind, int backward, float p0, float p1, float* out, int mem);" in text


def test_cpp_header_declarations():
    hpp = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp_gamma.hpp")).read()
    for decl in ('#include "gridpp.hpp"', "inline vec gamma_inv(const vec& levels, const vec& shape, const vec& scale)", "class Gamma : public Transform {",
                 "Gamma(float shape, float scale, float tolerance = 0.01)", "using Transform::forward;", "using Transform::backward;",
                 "float forward(float value) const", "float backward(float value) const"):
        assert decl in hpp, decl
    for message in ("Shape parameter must be > 0 in the gamma distribution", "Scale parameter must be > 0 in the gamma distribution",
                    "Tolerance must be >= 0 in the gamma distribution", "gamma_inv: levels, shape and scale must be of the same size"):
        assert 'std::invalid_argument("%s")' % message in hpp, message
    assert "boost" not in hpp.replace("Boost's error policies", "").replace("minus the Boost members", "").lower()


def test_loop_bounds_are_named_constants():
    text = open(os.path.join(ROOT, "gridpp_amd", "csrc", "gamma_fn.h")).read()
    for name in ("SERIES_MAX_TERMS", "FRACTION_MAX_STEPS", "INVERSE_MAX_STEPS"):
        assert re.search(r"constexpr int %s = \d+;" % name, text) and re.search(r"for\(n = 1; n <= %s; n\+\+\)" % name, text), name
    assert not re.search(r"\bwhile\s*\(", text) and text.count("for(") == 4   # the series, the fraction, the two branches of the inverse
