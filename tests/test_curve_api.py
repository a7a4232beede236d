"""CPU: the curve functions through `import gridpp` and through the C-ABI without a GPU -- names and enum values, the #defines of
include/gridpp_hip.h, every ValueError raised before device work, and the host-only entry points (scalar apply_curve, scalar
interpolate, monotonize_curve, quantile_mapping_curve): they reproduce the reference's known answers and agree bit for bit with
the restatement of tests/curve_ref.py.  The scalar forms compile gridpp_amd/csrc/curve.h, the per-value source the kernels run."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from tests import curve_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CASES = [c for c in R.CASES if not R.needs_device(c)]


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


def test_names_and_enum_values(gridpp):
    import gridpp_amd
    assert (gridpp.OneToOne, gridpp.MeanSlope, gridpp.NearestSlope, gridpp.Zero, gridpp.Unchanged) == (0, 10, 20, 30, 40)   # include/gridpp.h:79-85
    for name in ("apply_curve", "interpolate", "quantile_mapping_curve", "monotonize_curve"):
        assert callable(getattr(gridpp, name)) and getattr(gridpp, name) is getattr(gridpp_amd, name)
    assert (R.OneToOne, R.MeanSlope, R.NearestSlope, R.Zero, R.Unchanged) == (0, 10, 20, 30, 40)


def test_defines_follow_the_header(gridpp):
    text = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    defs = dict(re.findall(r"#define (GPP_[A-Z_0-9]+) (-?\d+)", text))
    assert {k: int(defs[k]) for k in ("GPP_ONE_TO_ONE", "GPP_MEAN_SLOPE", "GPP_NEAREST_SLOPE", "GPP_ZERO", "GPP_UNCHANGED")} == \
        {"GPP_ONE_TO_ONE": gridpp.OneToOne, "GPP_MEAN_SLOPE": gridpp.MeanSlope, "GPP_NEAREST_SLOPE": gridpp.NearestSlope, "GPP_ZERO": gridpp.Zero,
         "GPP_UNCHANGED": gridpp.Unchanged}
    hpp = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp.hpp")).read()
    m = re.search(r"enum Extrapolation \{([^}]*)\}", hpp)
    assert m and dict((k.strip(), int(v)) for k, v in (p.split("=") for p in m.group(1).split(","))) == \
        {"OneToOne": 0, "MeanSlope": 10, "NearestSlope": 20, "Zero": 30, "Unchanged": 40}


@pytest.mark.parametrize("case", HOST_CASES, ids=[c["id"] for c in HOST_CASES])
def test_host_side_known_answers_through_the_library(gridpp, case):
    """every known answer that needs no array kernel: the scalar forms, the curve builders, empty inputs, every expected exception"""
    R.check_case(case, gridpp)


def test_host_side_cases_cover_the_four_functions():
    fns = [c["function"] for c in HOST_CASES if "raises" not in c]
    for fn in ("apply_curve", "interpolate", "quantile_mapping_curve", "monotonize_curve"):
        assert fn in fns
    assert sum(c["id"].startswith("mono_with_missing_") for c in HOST_CASES) == 14


def test_scalar_results_are_python_floats(gridpp):
    assert type(gridpp.apply_curve(1.5, [2, 5, 6], [1, 2, 3], gridpp.OneToOne, gridpp.OneToOne)) is float
    assert gridpp.apply_curve(1.5, [2, 5, 6], [1, 2, 3], gridpp.OneToOne, gridpp.OneToOne) == 3.5
    assert type(gridpp.interpolate(0.5, [0, 1], [0, 1])) is float
    for out in gridpp.quantile_mapping_curve([3, 1, 2], [6, 5, 4]) + gridpp.monotonize_curve([1, 2, 3], [1, 2, 3]):
        assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.ndim == 1


def random_curve(rng, C, kind):
    r, f = R.random_curves(rng, (), C, kind)
    return r, f


@pytest.mark.parametrize("kind", ["sorted", "unsorted", "duplicates", "nans"])
@pytest.mark.parametrize("C", [1, 2, 3, 10])
def test_scalar_forms_agree_bit_for_bit_with_the_restatement(gridpp, C, kind):
    """seeded random scalar cases, all 25 policy pairs: 16 (C, kind) x 25 pairs x 3 curves x 20 inputs = 24 000 values of each form"""
    rng = np.random.default_rng(17 * C + len(kind))
    for pb, pa in itertools.product(R.POLICIES, R.POLICIES):
        for _ in range(3):
            r, f = random_curve(rng, C, kind)
            xs = R.random_inputs(rng, (20,), f)
            xs[:3] = [np.nan, np.inf, -np.inf]
            got = np.array([gridpp.apply_curve(float(x), r, f, pb, pa) for x in xs], np.float32)
            np.testing.assert_array_equal(got, R.apply_curve(xs, r, f, pb, pa), err_msg="%s %s %s %d %d" % (f, r, xs, pb, pa))
            got = np.array([gridpp.interpolate(float(x), f, r) for x in xs], np.float32)
            np.testing.assert_array_equal(got, R.interpolate(xs, f, r), err_msg="%s %s %s" % (f, r, xs))


def test_curve_builders_agree_with_the_restatement_on_random_curves(gridpp):
    rng = np.random.default_rng(23)
    for it in range(600):
        n = int(rng.integers(1, 14))
        fcst = np.cumsum(rng.normal(0.4, 0.6, n)).astype(np.float32)   # mostly increasing, with knots
        ref = rng.normal(0, 1, n).astype(np.float32)
        if it % 3 == 0:
            fcst[rng.random(n) < 0.2] = np.nan
            ref[rng.random(n) < 0.2] = np.inf
        for got, want in zip(gridpp.monotonize_curve(ref, fcst), R.monotonize_curve(ref, fcst)):
            np.testing.assert_array_equal(got, want)
        a, b = rng.normal(0, 1, n).astype(np.float32), rng.normal(0, 1, n).astype(np.float32)
        q = rng.random(int(rng.integers(0, 5))).astype(np.float32)
        if q.size and it % 5 == 0:
            q[0] = 1.0
        for got, want in zip(gridpp.quantile_mapping_curve(a, b, q), R.quantile_mapping_curve(a, b, q)):
            np.testing.assert_array_equal(got, want)


def test_monotonize_with_no_valid_pair_gives_two_empty_arrays(gridpp):
    a, b = gridpp.monotonize_curve([np.nan, 1], [0, np.inf])
    assert a.shape == b.shape == (0,)


def test_quantile_mapping_indexes_the_unsorted_inputs_and_sorts_nan_last(gridpp):
    ref, fcst = [5, 1, 3], [30, 10, 20]
    a, b = gridpp.quantile_mapping_curve(ref, fcst, [0, 0.5, 1])   # quantile_mapping.cpp:41-42: elements 0, 1, 2 as given
    np.testing.assert_array_equal(a, ref)
    np.testing.assert_array_equal(b, fcst)
    a, b = gridpp.quantile_mapping_curve([2, np.nan, 1], [np.nan, 3, np.nan])
    np.testing.assert_array_equal(a, [1, 2, np.nan])
    np.testing.assert_array_equal(b, [3, np.nan, np.nan])


def test_value_errors_from_python_before_device_work(gridpp):
    P = gridpp.OneToOne
    for fcst in (0, [0, 1], [[0], [1]]):
        with pytest.raises(ValueError, match="cannot have size 0"):
            gridpp.apply_curve(fcst, [], [], P, P)
        with pytest.raises(ValueError, match="must be the same size"):
            gridpp.apply_curve(fcst, [1, 2, 3], [1, 2], P, P)
    for fcst in ([0, 1], [[0], [1]], []):   # the array forms: whatever the data (nothing extrapolates in the first, the last is empty)
        with pytest.raises(ValueError, match="Unknown extrapolation policy"):
            gridpp.apply_curve(fcst, [0, 1], [0, 1], P, 41)
        with pytest.raises(ValueError, match="Unknown extrapolation policy"):
            gridpp.apply_curve(fcst, [0, 1], [0, 1], -1, P)
    # the scalar form: the reference's lazy check (curve.cpp:41-72)
    with pytest.raises(ValueError, match="Unknown extrapolation policy"):
        gridpp.apply_curve(3, [3, 4, 5], [0, 1, 2], -1, -1)
    assert gridpp.apply_curve(1, [3, 4, 5], [0, 1, 2], -1, -1) == 4      # inside the curve
    assert gridpp.apply_curve(3, [3, 4, 5], [0, 1, 2], -1, P) == 6       # extrapolates above: policy_below is not looked at
    assert gridpp.apply_curve(3, [7], [0], -1, -1) == 10                 # C <= 1 forces slope 1 before the policy is looked at
    x3, c3, c4 = np.zeros((2, 3)), np.zeros((2, 3, 3)), np.zeros((2, 3, 4))
    with pytest.raises(ValueError, match="curve_ref and curve_fcst dimension sizes mismatch"):
        gridpp.apply_curve(x3, c3, c4, P, P)
    with pytest.raises(ValueError, match="Fcst and curve_ref dimension sizes mismatch"):
        gridpp.apply_curve(np.zeros((2, 4)), c4, c4, P, P)
    with pytest.raises(ValueError, match="Unknown extrapolation policy"):
        gridpp.apply_curve(x3, c4, c4, P, 3)
    with pytest.raises(ValueError):
        gridpp.apply_curve(x3, [[]], [[]], P, P)
    with pytest.raises(ValueError):
        gridpp.apply_curve(x3, np.zeros((2, 3, 0)), np.zeros((2, 3, 0)), P, P)
    with pytest.raises(ValueError, match="Dimension mismatch. Cannot interpolate."):
        gridpp.interpolate([0], [0, 1, 2], [0, 1])
    with pytest.raises(ValueError, match="Dimension mismatch. Cannot interpolate."):
        gridpp.interpolate(0, [0, 1, 2], [0, 1])
    assert np.isnan(gridpp.interpolate(np.nan, [0, 1, 2], [0, 1]))   # util.cpp:378-379 comes before the size check
    with pytest.raises(ValueError, match="Quantiles must be >= 0 and <= 1"):
        gridpp.quantile_mapping_curve([1, 2], [1, 2], [0.5, 1.5])
    with pytest.raises(ValueError, match="Quantiles must be >= 0 and <= 1"):
        gridpp.quantile_mapping_curve([], [], [np.nan])
    with pytest.raises(ValueError, match="ref and fcst must be of the same size"):
        gridpp.quantile_mapping_curve([1, 2], [1], [])
    with pytest.raises(ValueError, match="cannot have size 0"):
        gridpp.monotonize_curve([], [])
    with pytest.raises(ValueError, match="must be the same size"):
        gridpp.monotonize_curve([1, 2], [1])


def f32(*v):
    return np.asarray(v, np.float32)


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def test_value_errors_from_the_c_abi_itself(lib):
    """GPP_EINVAL (-1) with the reference's message, before any device work: these return the same without a GPU"""
    from gridpp_amd import _capi
    x, out, c2, c3 = f32(0, 1), f32(0, 0), f32(1, 2), f32(1, 2, 3)

    def einval(rc, message):
        assert rc == _capi.GPP_EINVAL
        assert message in lib.gpp_last_error().decode()

    einval(lib.gpp_apply_curve(ptr(x), 2, ptr(c3), 3, ptr(c2), 2, 0, 0, ptr(out), 0), "curve_ref and curve_fcst must be the same size")
    einval(lib.gpp_apply_curve(ptr(x), 2, ptr(c2), 0, ptr(c2), 0, 0, 0, ptr(out), 0), "curve_ref and curve_fcst cannot have size 0")
    for pb, pa in ((5, 0), (0, -1), (41, 40), (1, 10)):
        einval(lib.gpp_apply_curve(ptr(x), 2, ptr(c2), 2, ptr(c2), 2, pb, pa, ptr(out), 0), "Unknown extrapolation policy")
        einval(lib.gpp_apply_curve(ptr(x), 0, ptr(c2), 2, ptr(c2), 2, pb, pa, ptr(out), 0), "Unknown extrapolation policy")
        einval(lib.gpp_apply_curve_field(ptr(x), ptr(c2), ptr(c2), 1, 2, 1, 1, pb, pa, ptr(out), 0), "Unknown extrapolation policy")
    einval(lib.gpp_apply_curve_field(ptr(x), ptr(c2), ptr(c2), 1, 1, 2, 1, 0, 0, ptr(out), 0), "curve_ref and curve_fcst dimension sizes mismatch")
    einval(lib.gpp_apply_curve_field(ptr(x), ptr(c2), ptr(c2), 1, 2, 0, 0, 0, 0, ptr(out), 0), "cannot have size 0")
    einval(lib.gpp_interpolate(ptr(x), 2, ptr(c3), 3, ptr(c2), 2, ptr(out), 0), "Dimension mismatch. Cannot interpolate.")
    y = C.c_float(0)
    einval(lib.gpp_apply_curve_scalar(3.0, ptr(c3), 3, ptr(c2), 2, 0, 0, C.byref(y)), "must be the same size")
    einval(lib.gpp_apply_curve_scalar(3.0, ptr(c3), 0, ptr(c3), 0, 0, 0, C.byref(y)), "cannot have size 0")
    einval(lib.gpp_apply_curve_scalar(9.0, ptr(c3), 3, ptr(c3), 3, 0, 7, C.byref(y)), "Unknown extrapolation policy")
    assert lib.gpp_apply_curve_scalar(2.5, ptr(c3), 3, ptr(c3), 3, 7, 7, C.byref(y)) == _capi.GPP_OK and y.value == 2.5
    einval(lib.gpp_interpolate_scalar(0.0, ptr(c3), 3, ptr(c2), 2, C.byref(y)), "Dimension mismatch. Cannot interpolate.")
    n = C.c_int(-1)
    o1, o2 = f32(0, 0, 0), f32(0, 0, 0)
    einval(lib.gpp_monotonize_curve(ptr(c3), 3, ptr(c2), 2, ptr(o1), ptr(o2), C.byref(n)), "must be the same size")
    einval(lib.gpp_monotonize_curve(ptr(c3), 0, ptr(c3), 0, ptr(o1), ptr(o2), C.byref(n)), "cannot have size 0")
    einval(lib.gpp_quantile_mapping_curve(ptr(c3), 3, ptr(c2), 2, None, 0, ptr(o1), ptr(o2), C.byref(n)), "ref and fcst must be of the same size")
    einval(lib.gpp_quantile_mapping_curve(ptr(c3), 3, ptr(c3), 3, ptr(f32(0.5, -1)), 2, ptr(o1), ptr(o2), C.byref(n)), "Quantiles must be >= 0 and <= 1")
    # and the good calls of the host-only forms
    assert lib.gpp_quantile_mapping_curve(ptr(f32(3, 1, 2)), 3, ptr(f32(6, 5, 4)), 3, None, 0, ptr(o1), ptr(o2), C.byref(n)) == _capi.GPP_OK
    assert n.value == 3 and list(o1) == [1, 2, 3] and list(o2) == [4, 5, 6]
    assert lib.gpp_monotonize_curve(ptr(f32(0, 1, 2)), 3, ptr(f32(0, 1, 1)), 3, ptr(o1), ptr(o2), C.byref(n)) == _capi.GPP_OK
    assert n.value == 1 and o1[0] == 0 and o2[0] == 0


def test_empty_inputs_give_empty_results_without_device_work(gridpp, lib):
    from gridpp_amd import _capi
    P = gridpp.OneToOne
    q = gridpp.apply_curve([], [1, 2], [1, 2], P, P)
    assert isinstance(q, np.ndarray) and q.shape == (0,)
    assert gridpp.apply_curve([[]], [1, 2], [1, 2], P, P).shape == (1, 0)
    assert gridpp.apply_curve(np.zeros((0, 4)), np.zeros((0, 4, 3)), np.zeros((0, 4, 3)), P, P).shape == (0, 4)
    assert gridpp.interpolate([], [0, 1], [0, 1]).shape == (0,)
    c2 = f32(1, 2)
    assert lib.gpp_apply_curve(None, 0, ptr(c2), 2, ptr(c2), 2, 0, 0, None, 0) == _capi.GPP_OK
    assert lib.gpp_apply_curve_field(None, None, None, 0, 5, 2, 2, 0, 0, None, 0) == _capi.GPP_OK
    assert lib.gpp_interpolate(None, 0, ptr(c2), 2, ptr(c2), 2, None, 0) == _capi.GPP_OK


def test_array_forms_fail_loudly_without_a_gpu(gridpp):
    """no CPU path behind the array forms: "no HIP device" where none is visible (where one is, they simply work)"""
    P = gridpp.OneToOne
    for call, want in ((lambda: gridpp.apply_curve([0.5, 1.5], [1, 2], [1, 2], P, P), [0.5, 1.5]),
                       (lambda: gridpp.apply_curve([[0.5], [1.5]], [1, 2], [1, 2], P, P), [[0.5], [1.5]]),
                       (lambda: gridpp.apply_curve(np.ones((2, 3)), np.ones((2, 3, 4)), np.ones((2, 3, 4)), P, P), np.ones((2, 3))),
                       (lambda: gridpp.interpolate([0.5], [0, 1], [0, 1]), [0.5])):
        if gridpp.device_count() > 0:
            np.testing.assert_array_equal(call(), want)
        else:
            with pytest.raises(RuntimeError, match="no HIP device"):
                call()
