"""CPU: get_optimal_threshold and metric_optimizer_curve through `import gridpp_amd` without a GPU -- the two names and their arguments,
their absence from the `gridpp` alias and from gridpp.hpp, the exported C-ABI symbols with their declarations in gridpp_hip.h and _capi.py,
the C++ header gridpp_metric_optimizer.hpp, the cases that need no device (empty vectors, empty thresholds, the two exceptions, NULL
pointers), "no HIP device" for a real call where no GPU is visible -- and the brute-force restatement tests/metric_optimizer_ref.py, the
yardstick of the GPU tests, against the reference project's own known answers and against hand-worked corners of the definition
(DESIGN.md 4.13)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import metric_optimizer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_names_and_arguments(amd):
    assert list(inspect.signature(amd.get_optimal_threshold).parameters) == ["ref", "fcst", "threshold", "metric"]
    assert list(inspect.signature(amd.metric_optimizer_curve).parameters) == ["ref", "fcst", "thresholds", "metric"]
    assert "DESIGN.md 4.13" in amd.get_optimal_threshold.__doc__ and "brent_find_minima" in amd.get_optimal_threshold.__doc__


def test_the_alias_does_not_carry_them(amd):
    """the exact optimum, not the point Brent's search ends on: a script written for the reference asks for them by gridpp_amd's name"""
    import gridpp
    assert gridpp.implementation == "gridpp_amd"
    assert not hasattr(gridpp, "get_optimal_threshold") and not hasattr(gridpp, "metric_optimizer_curve")
    assert gridpp.calc_score is amd.calc_score
    hpp = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp.hpp")).read()
    assert "get_optimal_threshold" not in hpp and "metric_optimizer_curve" not in hpp


def test_c_abi_symbols_and_declarations(amd, lib):
    from gridpp_amd import _capi
    text = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    for decl in ("int gpp_get_optimal_threshold(const float* ref, const float* fcst, long long n, float threshold, int metric, float* out, int mem);",
                 "int gpp_metric_optimizer_curve(const float* ref, const float* fcst, long long n, const float* thresholds, int num_thresholds, int metric,\n"
                 "                               float* out_ref, float* out_fcst, int* out_count, int mem);"):
        assert decl in text, decl
    assert "metric_optimizer.cpp:105-184" in text and "metric_optimizer.cpp:105-127" in text
    assert len(_capi.SIGNATURES["gpp_get_optimal_threshold"]) == 7 and len(_capi.SIGNATURES["gpp_metric_optimizer_curve"]) == 10
    for name in ("gpp_get_optimal_threshold", "gpp_metric_optimizer_curve"):
        assert callable(getattr(lib, name))   # the symbol is exported and bound
    defs = {k: int(v) for k, v in re.findall(r"#define (GPP_MO_[A-Z_]+) (\d+)", text)}
    assert defs == {"GPP_MO_TILE_ITEMS": _capi.MO_TILE_ITEMS, "GPP_MO_GROUP": _capi.MO_GROUP}
    assert "gpp_get_optimal_threshold and gpp_metric_optimizer_curve" in text[text.index("With GPP_MEM_HOST"):text.index("#define GPP_HOST_F64")]


def test_cpp_header_declarations():
    hpp = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp_metric_optimizer.hpp")).read()
    for decl in ('#include "gridpp.hpp"', "inline float get_optimal_threshold(const vec& ref, const vec& fcst, float threshold, Metric metric)",
                 "inline vec metric_optimizer_curve(const vec& ref, const vec& fcst, const vec& thresholds, Metric metric, vec& output_fcst)"):
        assert decl in hpp, decl
    assert hpp.count('std::invalid_argument("ref and fcst not the same size")') == 2


# ---- what needs no device ---------------------------------------------------------------------------------------------------------------
def test_empty_vectors_give_nan(amd):
    for empty in ([], np.zeros(0), np.zeros(0, F)):
        for metric in R.METRICS:
            assert np.isnan(amd.get_optimal_threshold(empty, empty, 0.5, metric))
    assert np.isnan(amd.get_optimal_threshold([1.0, 2.0], [], 0.5, amd.Ets))   # nothing of ref is read
    a, b = amd.metric_optimizer_curve([], [], [1, 2, 3], amd.Ets)
    assert a.shape == (0,) and b.shape == (0,) and a.dtype == F and b.dtype == F
    assert np.isnan(R.get_optimal_threshold([], [], 0.5, R.Ets))


def test_empty_thresholds_give_two_empty_vectors(amd):
    for thresholds in ([], np.zeros(0)):
        a, b = amd.metric_optimizer_curve([1.0, 2.0, 3.0], [1.5, 2.5, 0.5], thresholds, amd.Ets)
        assert isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == F and b.dtype == F and a.shape == (0,) and b.shape == (0,)


def test_exceptions(amd):
    with pytest.raises(ValueError, match="^ref and fcst not the same size$"):
        amd.get_optimal_threshold([1.0], [1.0, 2.0], 0.5, amd.Ets)
    for ref, fcst in (([1.0], [1.0, 2.0]), ([1.0, 2.0, 3.0], [1.0, 2.0])):
        with pytest.raises(ValueError, match="^ref and fcst not the same size$"):
            amd.metric_optimizer_curve(ref, fcst, [0.5], amd.Ets)
    with pytest.raises(ValueError, match="^ref and fcst not the same size$"):
        amd.metric_optimizer_curve([1.0], [1.0, 2.0], [], amd.Ets)
    for bad in (2, -1, 60):
        with pytest.raises(ValueError, match="^Unknown metric$"):
            amd.get_optimal_threshold([1.0, 2.0], [1.0, 2.0], 0.5, bad)
        with pytest.raises(ValueError, match="^Unknown metric$"):
            amd.metric_optimizer_curve([1.0, 2.0], [1.0, 2.0], [0.5], bad)
        with pytest.raises(ValueError, match="^Unknown metric$"):
            R.get_optimal_threshold([1.0, 2.0], [1.0, 2.0], 0.5, bad)


def test_c_abi_checks_before_device_work(lib):
    from gridpp_amd import _capi
    a, out, count = np.full(8, 0.5, F), np.full(8, 7, F), C.c_int(7)
    res = C.c_float(7)
    assert lib.gpp_get_optimal_threshold(ptr(a), ptr(a), 8, 0.5, 0, None, 0) == _capi.GPP_EINVAL and "NULL" in lib.gpp_last_error().decode()
    assert lib.gpp_get_optimal_threshold(None, ptr(a), 8, 0.5, 0, C.byref(res), 0) == _capi.GPP_EINVAL and "NULL" in lib.gpp_last_error().decode()
    assert lib.gpp_get_optimal_threshold(ptr(a), None, 8, 0.5, 0, C.byref(res), 0) == _capi.GPP_EINVAL
    assert lib.gpp_get_optimal_threshold(ptr(a), ptr(a), -1, 0.5, 0, C.byref(res), 0) == _capi.GPP_EINVAL
    assert lib.gpp_get_optimal_threshold(ptr(a), ptr(a), 8, 0.5, 7, C.byref(res), 0) == _capi.GPP_EINVAL and lib.gpp_last_error().decode() == "Unknown metric"
    assert lib.gpp_get_optimal_threshold(None, None, 0, 0.5, 0, C.byref(res), 0) == _capi.GPP_OK and np.isnan(res.value)
    assert lib.gpp_metric_optimizer_curve(ptr(a), ptr(a), 8, ptr(a), 8, 0, ptr(out), ptr(out), None, 0) == _capi.GPP_EINVAL
    assert lib.gpp_metric_optimizer_curve(ptr(a), ptr(a), 8, None, 8, 0, ptr(out), ptr(out), C.byref(count), 0) == _capi.GPP_EINVAL
    assert lib.gpp_metric_optimizer_curve(ptr(a), ptr(a), 8, ptr(a), 8, 0, None, ptr(out), C.byref(count), 0) == _capi.GPP_EINVAL
    assert lib.gpp_metric_optimizer_curve(None, ptr(a), 8, ptr(a), 8, 0, ptr(out), ptr(out), C.byref(count), 0) == _capi.GPP_EINVAL
    assert lib.gpp_metric_optimizer_curve(ptr(a), ptr(a), 8, ptr(a), -1, 0, ptr(out), ptr(out), C.byref(count), 0) == _capi.GPP_EINVAL
    assert lib.gpp_metric_optimizer_curve(ptr(a), ptr(a), 8, ptr(a), 8, 3, ptr(out), ptr(out), C.byref(count), 0) == _capi.GPP_EINVAL
    count.value = 7
    assert lib.gpp_metric_optimizer_curve(ptr(a), ptr(a), 8, None, 0, 0, None, None, C.byref(count), 0) == _capi.GPP_OK and count.value == 0
    count.value = 7
    assert lib.gpp_metric_optimizer_curve(None, None, 0, ptr(a), 8, 0, ptr(out), ptr(out), C.byref(count), 0) == _capi.GPP_OK and count.value == 0
    assert np.all(out == 7)


def test_a_real_call_fails_loudly_without_a_gpu(amd):
    """no CPU path behind the two names: "no HIP device" where none is visible (where one is, the call simply works)"""
    obs, fcst = [0, 1, 1.4, 1.6, 2], [1, 2, 2.4, 2.6, 3]
    if amd.device_count() > 0:
        assert amd.get_optimal_threshold(obs, fcst, 1.5, amd.Bias) == 2.5
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        amd.get_optimal_threshold(obs, fcst, 1.5, amd.Bias)
    with pytest.raises(RuntimeError, match="no HIP device"):
        amd.metric_optimizer_curve(obs, fcst, [1.5], amd.Bias)


# ---- the yardstick itself -----------------------------------------------------------------------------------------------------------------
def test_the_restatement_satisfies_the_reference_known_answers():
    """tests/test_metric_optimizer.py of the reference pins ranges only: (2.4, 2.6), and curve_ref within 1.5 of curve_fcst squared"""
    x = R.get_optimal_threshold([0, 1, 1.4, 1.6, 2], [1, 2, 2.4, 2.6, 3], 1.5, R.Bias)
    assert 2.4 < x < 2.6 and x == F(2.5)
    obs = np.linspace(0, 10, 101)
    for metric in (R.Pc, R.Bias):
        curve_ref, curve_fcst = R.metric_optimizer_curve(obs, obs ** 2, [1, 2, 3, 4], metric)
        assert list(curve_fcst) == [1, 2, 3, 4]
        assert np.all(np.abs(curve_ref - curve_fcst ** 2) < 1.5)
        np.testing.assert_allclose(curve_ref, [1.105, 4.205, 9.305, 16.405], rtol=0, atol=1e-5)


def test_the_restatement_on_hand_worked_corners():
    nan = np.nan
    # ref > 1.5 at the fcst values 3 .. 6; Ts = a / (a + b + c): x = 1: 4 / (4 + 2 + 0), x = 2: 4 / (4 + 1 + 0), x = 3: 3 / (3 + 1 + 1), ...,
    # x = 7: 0 / (0 + 0 + 4)
    ref, fcst = [0, 0, 3, 3, 3, 3, 0], [1, 2, 3, 4, 5, 6, 7]
    u, s = R.plateau_scores(ref, fcst, 1.5, R.Ts)
    assert list(u) == [1, 2, 3, 4, 5, 6, 7] and s[0] == F(4 / 6) and s[1] == F(4 / 5) and s[2] == F(3 / 5) and s[6] == 0
    assert R.get_optimal_threshold(ref, fcst, 1.5, R.Ts) == F(2.5)           # the plateau [2, 3) alone
    # all fcst equal: one plateau, best = s(u_0)
    assert np.isnan(R.get_optimal_threshold([0, 3, 3], [2, 2, 2], 1.5, R.Pc))
    # -0 and +0 are one plateau
    assert list(R.plateaus(np.array([-0.0, 0.0, 1.0], F))) == [0, 1] and not np.signbit(R.plateaus(np.array([-0.0], F))[0])
    # non-finite fcst defines no plateau
    assert list(R.plateaus(np.array([nan, np.inf, -np.inf, 2, 1], F))) == [1, 2]
    assert np.isnan(R.get_optimal_threshold([1, 2], [nan, np.inf], 1.5, R.Ets))
