"""CPU: downscale_probability, mask_threshold_downscale_consensus / _quantile, smart and the ComparisonOperator values exist
under both import names, raise their argument errors before any device work, and fail loudly (no CPU path) without a GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("Lt", "Leq", "Gt", "Geq", "downscale_probability", "mask_threshold_downscale_consensus", "mask_threshold_downscale_quantile", "smart")


@pytest.fixture(scope="module")
def gridpp():
    import __graft_entry__ as g
    g.build()
    import gridpp_amd
    return gridpp_amd


def _grid(gridpp, Y, X, type=0):
    lons, lats = np.meshgrid(np.arange(X) * 10.0, 30 + np.arange(Y) * 10.0)
    return gridpp.Grid(lats, lons, np.zeros((Y, X)), np.full((Y, X), 0.5), type)


def test_names_are_the_same_objects_through_import_gridpp(gridpp):
    import gridpp as alias
    for name in NAMES:
        assert getattr(alias, name) is getattr(gridpp, name)
    assert (gridpp.Lt, gridpp.Leq, gridpp.Gt, gridpp.Geq) == (0, 10, 20, 30)   # include/gridpp.h:138-143


def test_row_capacity_constant_follows_the_header(gridpp):
    text = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    assert int(re.search(r"#define GPP_ENSEMBLE_ROW_CAP (\d+)", text).group(1)) == gridpp._capi.ENSEMBLE_ROW_CAP
    for name, value in (("GPP_LT", 0), ("GPP_LEQ", 10), ("GPP_GT", 20), ("GPP_GEQ", 30)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value


def test_value_errors_before_device_work(gridpp):
    gi, go, gc = _grid(gridpp, 2, 3), _grid(gridpp, 3, 4), _grid(gridpp, 3, 4, gridpp.Cartesian)
    cube, thr = np.zeros((2, 3, 5)), np.zeros((3, 4))
    P, C, Q, S = (gridpp.downscale_probability, gridpp.mask_threshold_downscale_consensus, gridpp.mask_threshold_downscale_quantile,
                  gridpp.smart)
    st = gridpp.BarnesStructure(10000)
    raises = [
        (lambda: P(gi, go, np.zeros((3, 2, 5)), thr, gridpp.Lt), "Grid size is not the same as values"),
        (lambda: C(gi, go, np.zeros((2, 2, 5)), np.zeros((2, 2, 5)), np.zeros((2, 2, 5)), thr, gridpp.Lt, gridpp.Mean), "Grid size is not the same as values"),
        (lambda: S(gi, go, np.zeros((3, 2)), 3, st), "Grid size is not the same as values"),
        (lambda: C(gi, go, cube, np.zeros((2, 3, 4)), cube, thr, gridpp.Lt, gridpp.Mean), "same shape"),
        (lambda: Q(gi, go, cube, cube, np.zeros((2, 3, 6)), thr, gridpp.Lt, 0.5), "same shape"),
        (lambda: P(gi, go, cube, np.zeros((4, 3)), gridpp.Lt), "Grid size is not the same as threshold"),
        (lambda: Q(gi, go, cube, cube, cube, np.zeros((3, 3)), gridpp.Lt, 0.5), "Grid size is not the same as threshold"),
        (lambda: P(gi, gc, cube, thr, gridpp.Lt), "Coordinate types must be the same"),
        (lambda: C(gi, gc, cube, cube, cube, thr, gridpp.Lt, gridpp.Mean), "Coordinate types must be the same"),
        (lambda: S(gi, gc, np.zeros((2, 3)), 3, st), "Coordinate types must be the same"),
        (lambda: P(gi, go, cube, thr, 5), "Invalid comparison operator"),
        (lambda: P(gi, go, cube, thr, 40), "Invalid comparison operator"),
        (lambda: C(gi, go, cube, cube, cube, thr, -1, gridpp.Mean), "Invalid comparison operator"),
        (lambda: Q(gi, go, cube, cube, cube, thr, gridpp.Geq, 1.5), "calc_quantile: Quantile must be between 0 and 1 inclusive"),
        (lambda: Q(gi, go, cube, cube, cube, thr, gridpp.Geq, -0.1), "calc_quantile: Quantile must be between 0 and 1 inclusive"),
    ]
    for f, msg in raises:
        with pytest.raises(ValueError, match=msg):
            f()
    for bad in (5, gridpp.Unknown, 100):
        with pytest.raises(RuntimeError, match="Internal error. Cannot compute statistic"):
            C(gi, go, cube, cube, cube, thr, gridpp.Lt, bad)


def test_capi_checks_before_device_work(gridpp):
    """the same refusals from the C-ABI itself (what the C++ mirror and other callers get)"""
    import ctypes as C
    lib = gridpp._capi.lib()
    gi, go, gc = _grid(gridpp, 2, 3), _grid(gridpp, 3, 4), _grid(gridpp, 3, 4, gridpp.Cartesian)
    cube, thr, out = np.zeros((2, 3, 5), np.float32), np.zeros((3, 4), np.float32), np.zeros((3, 4), np.float32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    EINVAL, ERUNTIME = gridpp._capi.GPP_EINVAL, gridpp._capi.GPP_ERUNTIME
    assert lib.gpp_downscale_probability(gi._h, go._h, p(cube), 5, p(thr), 15, p(out), 0) == EINVAL
    assert lib.gpp_downscale_probability(gi._h, gc._h, p(cube), 5, p(thr), 0, p(out), 0) == EINVAL
    assert lib.gpp_mask_threshold_downscale(gi._h, go._h, p(cube), p(cube), p(cube), 5, p(thr), 7, 0, 0.0, p(out), 0) == EINVAL
    assert lib.gpp_mask_threshold_downscale(gi._h, go._h, p(cube), p(cube), p(cube), 5, p(thr), 0, 40, 2.0, p(out), 0) == EINVAL
    assert lib.gpp_mask_threshold_downscale(gi._h, go._h, p(cube), p(cube), p(cube), 5, p(thr), 0, 45, 0.0, p(out), 0) == ERUNTIME
    assert b"Cannot compute statistic" in lib.gpp_last_error()
    st = gridpp.BarnesStructure(10000)
    assert lib.gpp_smart(gi._h, gc._h, p(cube), 3, C.byref(st._s), p(out), 0) == EINVAL


def test_empty_output_gives_empty_result(gridpp):
    gi = _grid(gridpp, 2, 3)
    e = gridpp.Grid(np.zeros((0, 0)), np.zeros((0, 0)))
    cube, thr = np.zeros((2, 3, 5)), np.zeros((0, 0))
    assert np.shape(gridpp.downscale_probability(gi, e, cube, thr, gridpp.Lt)) == (0, 0)
    assert np.shape(gridpp.mask_threshold_downscale_consensus(gi, e, cube, cube, cube, thr, gridpp.Lt, gridpp.Mean)) == (0, 0)
    assert np.shape(gridpp.mask_threshold_downscale_quantile(gi, e, cube, cube, cube, thr, gridpp.Lt, 0.5)) == (0, 0)
    assert np.shape(gridpp.smart(gi, e, np.zeros((2, 3)), 3, gridpp.BarnesStructure(10000))) == (0, 0)


def test_compute_fails_loudly_without_gpu(gridpp):
    if gridpp.device_count() > 0:
        pytest.skip("a GPU is visible")
    gi, go = _grid(gridpp, 2, 3), _grid(gridpp, 3, 4)
    cube, thr = np.zeros((2, 3, 5)), np.zeros((3, 4))
    for f in (lambda: gridpp.downscale_probability(gi, go, cube, thr, gridpp.Leq),
              lambda: gridpp.mask_threshold_downscale_consensus(gi, go, cube, cube, cube, thr, gridpp.Gt, gridpp.Median),
              lambda: gridpp.mask_threshold_downscale_quantile(gi, go, cube, cube, cube, thr, gridpp.Geq, 0.9),
              lambda: gridpp.smart(gi, go, np.zeros((2, 3)), 3, gridpp.BarnesStructure(10000))):
        with pytest.raises(RuntimeError, match="no HIP device"):
            f()
