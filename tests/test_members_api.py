"""CPU: neighbourhood_members and calc_gradient_members through `import gridpp_amd` without a GPU -- the two names and their arguments, their
absence from the `gridpp` alias and from gridpp.hpp, the header of their own (it compiles with the host compiler, together with the program the
GPU test drives), the C-ABI declarations and bindings, the errors of the two wrappers and of the two entry points in their order (all before any
device work), the empty shapes and "no HIP device" for a real call where no GPU is visible; and the yardstick of the GPU tests: the numpy
restatement of tests/members_ref.py against the oracle's neighbourhood and calc_gradient per plane, and the margin of its exact data
(DESIGN.md 4.21)."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import members_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MEDIAN = "^neighbourhood_members does not compute the statistic Median: order statistics per member are not supported$"
RANDOM = "^neighbourhood_members does not compute the statistic RandomChoice: order statistics per member are not supported$"
QUANTILE = "^Use neighbourhood_quantile for computing neighbourhood quantiles$"


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
    assert list(inspect.signature(amd.neighbourhood_members).parameters) == ["input", "halfwidth", "statistic"]
    sig = inspect.signature(amd.calc_gradient_members)
    assert list(sig.parameters) == ["base", "values", "gradient_type", "halfwidth", "num_min", "min_range", "default_gradient"]
    assert sig.parameters["num_min"].default == 2 and np.isnan(sig.parameters["min_range"].default) and sig.parameters["default_gradient"].default == 0
    assert inspect.signature(amd.calc_gradient).parameters.keys() == sig.parameters.keys()
    assert "DESIGN.md 4.21" in amd.neighbourhood_members.__doc__ and "DESIGN.md 4.21" in amd.calc_gradient_members.__doc__


def test_the_alias_does_not_carry_them(amd):
    import gridpp
    assert gridpp.implementation == "gridpp_amd"
    assert callable(amd.neighbourhood_members) and callable(amd.calc_gradient_members)
    assert not hasattr(gridpp, "neighbourhood_members") and not hasattr(gridpp, "calc_gradient_members")
    assert gridpp.neighbourhood is amd.neighbourhood and gridpp.calc_gradient is amd.calc_gradient


def test_cpp_header_of_its_own():
    hpp = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp.hpp")).read()
    assert "neighbourhood_members" not in hpp and "calc_gradient_members" not in hpp and "gridpp_members" not in hpp
    own = " ".join(open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp_members.hpp")).read().split())
    for decl in ('#include "gridpp.hpp"',
                 "inline vec3 neighbourhood_members(const vec3& input, int halfwidth, Statistic statistic)",
                 "inline vec3 calc_gradient_members(const vec2& base, const vec3& values, GradientType gradient_type, int halfwidth, int min_num = 2, "
                 "float min_range = MV, float default_gradient = 0)",
                 "inline vec3 calc_gradient_members(const vec3& base, const vec3& values, GradientType gradient_type, int halfwidth, int min_num = 2, "
                 "float min_range = MV, float default_gradient = 0)",
                 "inline void neighbourhood_members_device(", "inline void calc_gradient_members_device(",
                 'std::invalid_argument("Half width must be > 0")'):
        assert decl in own, decl
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "gridpp_amd", "host"), os.path.join(ROOT, "tests", "cpp", "test_members.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_c_abi_declarations_and_bindings(amd, lib):
    from gridpp_amd import _capi
    text = " ".join(open(os.path.join(ROOT, "include", "gridpp_hip.h")).read().split())
    for decl in ("int gpp_neighbourhood_members(const float* input, int ny, int nx, int ne, int halfwidth, int statistic, float* out, int mem);",
                 "int gpp_calc_gradient_members(const float* base, int base_members, const float* values, int ny, int nx, int ne, int gradient_type, "
                 "int halfwidth, int num_min, float min_range, float default_gradient, float* out, int mem);"):
        assert decl in text, decl
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    assert _capi.SIGNATURES["gpp_neighbourhood_members"] == [vp, i, i, i, i, i, vp, i]
    assert _capi.SIGNATURES["gpp_calc_gradient_members"] == [vp, i, vp, i, i, i, i, i, i, f, f, vp, i]
    assert callable(lib.gpp_neighbourhood_members) and callable(lib.gpp_calc_gradient_members)


# ---- errors, in their order, before any device work ---------------------------------------------------------------------------------------
def test_neighbourhood_members_errors_and_their_order(amd):
    f = np.zeros((4, 5, 3), F)
    with pytest.raises(ValueError, match="^Half width must be > 0$"):
        amd.neighbourhood_members(f, -1, amd.Mean)
    with pytest.raises(ValueError, match="^Half width must be > 0$"):
        amd.neighbourhood_members(f, -1, amd.Quantile)                                   # ... before the statistic
    with pytest.raises(ValueError, match="^Half width must be > 0$"):
        amd.neighbourhood_members(np.zeros((0, 5, 3), F), -2, amd.Median)                # ... and before the empty cube
    with pytest.raises(ValueError, match=QUANTILE):
        amd.neighbourhood_members(f, 1, amd.Quantile)
    with pytest.raises(ValueError, match=MEDIAN):
        amd.neighbourhood_members(f, 1, amd.Median)
    with pytest.raises(ValueError, match=RANDOM):
        amd.neighbourhood_members(f, 0, amd.RandomChoice)
    with pytest.raises(ValueError, match=MEDIAN):
        amd.neighbourhood_members(np.zeros((4, 0, 3), F), 1, amd.Median)                 # the statistic before the empty cube
    with pytest.raises(ValueError, match="unknown statistic"):
        amd.neighbourhood_members(f, 1, 12345)
    for wrong in (np.zeros(4, F), np.zeros((4, 5), F), np.zeros((2, 2, 2, 2), F)):
        with pytest.raises(RuntimeError, match="input must have 3 dimensions"):
            amd.neighbourhood_members(wrong, 1, amd.Mean)


def test_calc_gradient_members_errors_and_their_order(amd):
    b, v = np.zeros((4, 5), F), np.zeros((4, 5, 3), F)
    mm = amd.MinMax
    for call, other in ((lambda *a: amd.calc_gradient_members(*a), v), (lambda *a: amd.calc_gradient(*a), b)):     # the same checks, order and messages
        with pytest.raises(ValueError, match="^Halwidth cannot be <= 0; must be positive integer$"):
            call(b, other, mm, 0, -1, -1.0)
        with pytest.raises(ValueError, match="^min_range must be >= 0$"):
            call(b, other, mm, 1, -1, -1.0)
        with pytest.raises(ValueError, match="^num_min must be >= 0$"):
            call(b, other, mm, 1, -1, 0.0)
        with pytest.raises(ValueError, match="^base input has no size$"):
            call(np.zeros((0, 5), F), other, mm, 1)
        with pytest.raises(ValueError, match="^base is not the same size as values$"):
            call(np.zeros((4, 6), F), other, mm, 1)
        with pytest.raises(ValueError, match="^unknown gradient type$"):
            call(b, other, 5, 1)
    with pytest.raises(ValueError, match="^num_min must be >= 0$"):
        amd.calc_gradient_members(np.zeros((0, 5), F), v, mm, 1, -1)                      # ... before the size of base
    for base in (np.zeros((4, 5, 2), F), np.zeros((4, 5, 1), F), np.zeros((5, 4, 3), F), np.zeros(20, F), np.zeros((4, 5, 3, 1), F), np.float32(1.0)):
        with pytest.raises(ValueError, match="^base is not the same size as values$"):
            amd.calc_gradient_members(base, v, mm, 1)
    for wrong in (np.zeros((4, 5), F), np.zeros(4, F), np.zeros((2, 2, 2, 2), F)):
        with pytest.raises(RuntimeError, match="values must have 3 dimensions"):
            amd.calc_gradient_members(b, wrong, mm, 1)


def test_empty_shapes(amd):
    for shape in ((0, 5, 3), (4, 0, 3), (4, 5, 0), (0, 0, 0)):
        for stat in (amd.Mean, amd.Max, amd.Std, amd.Count):
            out = amd.neighbourhood_members(np.zeros(shape, F), 1, stat)
            assert isinstance(out, np.ndarray) and out.dtype == F and out.shape == shape
    for shape in ((4, 0, 3), (4, 5, 0)):
        for gt in (amd.MinMax, amd.LinearRegression):
            out = amd.calc_gradient_members(np.zeros(shape[:2], F), np.zeros(shape, F), gt, 1)
            assert isinstance(out, np.ndarray) and out.dtype == F and out.shape == shape
            out = amd.calc_gradient_members(np.zeros(shape, F), np.zeros(shape, F), gt, 1)
            assert out.shape == shape


# ---- the C-ABI without a device ---------------------------------------------------------------------------------------------------------------
def test_c_abi_checks_before_device_work(amd, lib):
    from gridpp_amd import _capi
    nbh, grad = lib.gpp_neighbourhood_members, lib.gpp_calc_gradient_members
    f, b, out = np.full((4, 5, 3), 0.5, F), np.full((4, 5), 2.0, F), np.full((4, 5, 3), 7, F)
    nan = float("nan")

    def message():
        return lib.gpp_last_error().decode()
    assert nbh(None, 4, 5, 3, -1, amd.Quantile, None, 0) == _capi.GPP_EINVAL and message() == "Half width must be > 0"        # first of all
    assert nbh(ptr(f), 4, 5, 3, 1, amd.Quantile, ptr(out), 0) == _capi.GPP_EINVAL and message() == QUANTILE[1:-1]
    assert nbh(ptr(f), 0, 5, 3, 1, amd.Median, ptr(out), 0) == _capi.GPP_EINVAL and message() == MEDIAN[1:-1]                 # before the empty cube
    assert nbh(ptr(f), 4, 5, 3, 1, amd.RandomChoice, ptr(out), 0) == _capi.GPP_EINVAL and message() == RANDOM[1:-1]
    assert nbh(ptr(f), 4, 5, 3, 1, 12345, ptr(out), 0) == _capi.GPP_EINVAL and "unknown statistic" in message()
    assert nbh(ptr(f), 4, -5, 3, 1, amd.Mean, ptr(out), 0) == _capi.GPP_EINVAL
    for args in ((None, 4, 5, 3, 1, amd.Mean, ptr(out), 0), (ptr(f), 4, 5, 3, 1, amd.Mean, None, 0)):
        assert nbh(*args) == _capi.GPP_EINVAL and "NULL" in message()
    for shape in ((0, 5, 3), (4, 0, 3), (4, 5, 0)):
        assert nbh(None, *shape, 1, amd.Mean, None, 0) == _capi.GPP_OK
    mm = amd.MinMax
    assert grad(None, 7, None, 0, 5, 3, 5, 0, -1, -1.0, 0.0, None, 0) == _capi.GPP_EINVAL and message() == "Halwidth cannot be <= 0; must be positive integer"
    assert grad(None, 7, None, 0, 5, 3, 5, 1, -1, -1.0, 0.0, None, 0) == _capi.GPP_EINVAL and message() == "min_range must be >= 0"
    assert grad(None, 7, None, 0, 5, 3, 5, 1, -1, nan, 0.0, None, 0) == _capi.GPP_EINVAL and message() == "num_min must be >= 0"
    assert grad(None, 7, None, 0, 5, 3, 5, 1, 2, nan, 0.0, None, 0) == _capi.GPP_EINVAL and message() == "base input has no size"
    assert grad(None, 7, None, 4, 5, 3, 5, 1, 2, nan, 0.0, None, 0) == _capi.GPP_EINVAL and message() == "base is not the same size as values"
    for members in (0, 2, 4, -1):
        assert grad(ptr(f), members, ptr(f), 4, 5, 3, mm, 1, 2, nan, 0.0, ptr(out), 0) == _capi.GPP_EINVAL and message() == "base is not the same size as values"
    assert grad(ptr(b), 1, ptr(f), 4, 5, 3, 5, 1, 2, nan, 0.0, ptr(out), 0) == _capi.GPP_EINVAL and message() == "unknown gradient type"
    for args in ((None, 1, ptr(f), 4, 5, 3, mm, 1, 2, nan, 0.0, ptr(out), 0), (ptr(b), 1, None, 4, 5, 3, mm, 1, 2, nan, 0.0, ptr(out), 0),
                 (ptr(b), 1, ptr(f), 4, 5, 3, mm, 1, 2, nan, 0.0, None, 0)):
        assert grad(*args) == _capi.GPP_EINVAL and "NULL" in message()
    assert grad(None, 1, None, 4, 0, 3, mm, 1, 2, nan, 0.0, None, 0) == _capi.GPP_OK
    assert grad(None, 0, None, 4, 5, 0, mm, 1, 2, nan, 0.0, None, 0) == _capi.GPP_OK
    assert np.all(out == 7)                                                                  # nothing was written


def test_a_real_call_fails_loudly_without_a_gpu(amd, lib):
    """no CPU path behind the names: "no HIP device" where none is visible (where one is, the call simply works)"""
    from gridpp_amd import _capi
    f, b = np.arange(60, dtype=F).reshape(4, 5, 3), np.arange(20, dtype=F).reshape(4, 5)
    if amd.device_count() > 0:
        assert amd.neighbourhood_members(f, 1, amd.Mean).shape == (4, 5, 3) and amd.calc_gradient_members(b, f, amd.MinMax, 1).shape == (4, 5, 3)
        return
    for call in (lambda: amd.neighbourhood_members(f, 1, amd.Mean), lambda: amd.neighbourhood_members(f, 40, amd.Max),
                 lambda: amd.neighbourhood_members(f.astype(np.float64), 0, amd.Std), lambda: amd.calc_gradient_members(b, f, amd.MinMax, 1),
                 lambda: amd.calc_gradient_members(f, f, amd.LinearRegression, 2)):
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
    out = np.zeros((4, 5, 3), F)
    assert lib.gpp_neighbourhood_members(ptr(f), 4, 5, 3, 1, amd.Mean, ptr(out), 0) == _capi.GPP_ENODEVICE
    assert lib.gpp_calc_gradient_members(ptr(b), 1, ptr(f), 4, 5, 3, amd.LinearRegression, 1, 2, float("nan"), 0.0, ptr(out), 0) == _capi.GPP_ENODEVICE


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [0, 1, 7, 40])
def test_restatement_gives_the_oracles_neighbourhood_per_plane(hw):
    from oracle import oracle as O
    from tests.test_gpu_neighbourhood_parity import close
    cube = R.general_cube(12, (12, 9, 5))
    assert np.isnan(cube).any() and np.isinf(cube).any() and np.isnan(cube[:, :, 2]).all()
    for name in ("Mean", "Sum"):
        close(R.expected(cube, hw, name), R.per_plane(O.neighbourhood, cube, hw, getattr(O, name)))
    for name in ("Count", "Min", "Max"):
        close(R.expected(cube, hw, name), R.per_plane(O.neighbourhood, cube, hw, getattr(O, name)), exact=True)
    var = R.per_plane(O.neighbourhood, cube, hw, O.Variance)
    ours = R.variance(cube, hw)
    assert (np.isnan(var) == np.isnan(ours)).all()
    ok = ~np.isnan(var)
    assert (np.abs(var[ok] - ours[ok]) <= 1e-5 * R.mean_of_squares(cube, hw)[ok] + 1e-9).all()
    exact = R.exact_cube(13, (12, 9, 5))
    for name in ("Mean", "Sum", "Count", "Min", "Max"):                                   # on exact data the oracle's float32 results are the restatement's, bit for bit
        close(R.expected(exact, hw, name), R.per_plane(O.neighbourhood, exact, hw, getattr(O, name)), exact=True)


def test_restatement_gives_the_oracles_gradients_per_plane():
    from oracle import oracle as O
    rng = np.random.default_rng(23)
    shape = (14, 11, 3)
    base = rng.uniform(0, 1500, shape[:2]).astype(F)
    values = (280 - 0.0065 * base[:, :, None] + rng.normal(0, 0.3, shape)).astype(F)
    base[4:7, 2:8] = np.nan
    values[rng.random(shape) < 0.05] = np.nan
    for hw, num_min, min_range, dflt in ((1, 0, np.nan, -0.0065), (3, 5, 100.0, 0.0), (7, 2, 0.0, 1.0)):
        ref = R.per_plane(lambda p: O.calc_gradient(base, p, 0, hw, num_min, min_range, dflt), values)
        np.testing.assert_array_equal(R.per_plane(lambda p: R.gradient_minmax(base, p, hw, num_min, min_range, dflt), values), ref)
        if hw == 1:
            continue     # (three-point windows: the float32 moments of the reference cancel, a float64 restatement says nothing about them)
        ref = R.per_plane(lambda p: O.calc_gradient(base, p, 10, hw, num_min, min_range, dflt), values)
        ours = R.per_plane(lambda p: R.gradient_linear(base, p, hw, num_min, min_range, dflt), values)
        assert np.array_equal(np.isnan(ours), np.isnan(ref))
        np.testing.assert_allclose(ours, ref, rtol=2e-3, atol=1e-6)


def test_exact_means_are_far_from_rounding_boundaries():
    """float32(s / n) of the exact data does not change when the double quotient moves by 4 ulp either way, at every halfwidth used, with 5 % missing"""
    rng = np.random.default_rng(3)
    plane = (rng.integers(-512, 513, (37, 29)) / 8).astype(F)
    plane[rng.random(plane.shape) < 0.05] = np.nan
    for hw in R.HALFWIDTHS:
        s, n, _, _ = R.window_stats(plane, hw)
        q = s[n > 0] / n[n > 0]
        lo = hi = q
        for _ in range(4):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        assert (lo.astype(F) == q.astype(F)).all() and (hi.astype(F) == q.astype(F)).all()
