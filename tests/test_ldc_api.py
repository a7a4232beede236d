"""CPU: gridpp_amd.local_distribution_correction exists, dispatches on pobs.ndim, refuses every shape the reference
would read out of bounds with (src/api/local_distribution_correction.cpp:43-54 checks the number of times only) and fails
loudly without a device."""
import ctypes as C

import numpy as np
import pytest

EINVAL = -1


@pytest.fixture(scope="module")
def gridpp():
    import __graft_entry__ as g
    g.build()
    import gridpp_amd
    return gridpp_amd


@pytest.fixture()
def setup(gridpp):
    lons, lats = np.meshgrid(np.arange(4) * 1000.0, np.arange(3) * 1000.0)
    grid = gridpp.Grid(lats, lons, ((),), ((),), gridpp.Cartesian)
    points = gridpp.Points([0, 500, 900, 1500, 2000], [100, 700, 1500, 2500, 3000], (), (), gridpp.Cartesian)
    return dict(grid=grid, bg=np.ones((3, 4), np.float32), points=points, pobs=np.ones((2, 5), np.float32), pbg=np.ones((2, 5), np.float32),
                st=gridpp.BarnesStructure(2500), q0=0.1, q1=0.9, n=5)


def call(gridpp, s, **kw):
    a = dict(s, **kw)
    return gridpp.local_distribution_correction(a["grid"], a["bg"], a["points"], a["pobs"], a["pbg"], a["st"], a["q0"], a["q1"], a["n"])


def test_the_function_exists_and_is_bound(gridpp):
    """in gridpp_amd; the alias package `gridpp` keeps the surface tests/test_pointwise_api.py pins for it, which leaves this name out"""
    import inspect
    assert list(inspect.signature(gridpp.local_distribution_correction).parameters) == [
        "bgrid", "background", "points", "pobs", "pbackground", "structure", "min_quantile", "max_quantile", "min_points"]
    from gridpp_amd import _capi
    assert "gpp_local_distribution_correction" in _capi.SIGNATURES


def test_shapes_the_reference_would_misread_are_refused(gridpp, setup):
    s = setup
    with pytest.raises(ValueError, match=r"pobs \(2,5\) is not the same size as pbackground \(3,5\)"):   # the reference's own check and message
        call(gridpp, s, pbg=np.ones((3, 5)))
    with pytest.raises(ValueError, match=r"pobs \(2,5\) is not the same shape as pbackground \(2,4\)"):
        call(gridpp, s, pbg=np.ones((2, 4)))
    with pytest.raises(ValueError, match=r"input field \(4, 3\) is not the same size as the grid \(3, 4\)"):
        call(gridpp, s, bg=np.ones((4, 3)))
    with pytest.raises(ValueError, match=r"pobs \(6\) and points \(5\) size mismatch"):
        call(gridpp, s, pobs=np.ones((2, 6)), pbg=np.ones((2, 6)))
    with pytest.raises(ValueError, match=r"pobs \(4\) and points \(5\) size mismatch"):
        call(gridpp, s, pobs=np.ones(4), pbg=np.ones(4))
    with pytest.raises(ValueError, match="pobs and pbackground must both be 1-D"):
        call(gridpp, s, pobs=np.ones(5))
    with pytest.raises(ValueError, match="pobs and pbackground must both be 1-D"):
        call(gridpp, s, pobs=np.ones((1, 2, 5)), pbg=np.ones((1, 2, 5)))
    geodetic = gridpp.Points([0, 0, 0, 0, 0], [0, 1, 2, 3, 4])
    with pytest.raises(ValueError, match="Both background grid and observations points must be of same coordinate type"):
        call(gridpp, s, points=geodetic)
    with pytest.raises(TypeError):
        call(gridpp, s, grid=s["points"])
    with pytest.raises(RuntimeError, match="structure must be one of the gridpp_amd structure functions"):
        call(gridpp, s, st=None)


@pytest.mark.parametrize("q0,q1", [(-0.1, 0.9), (0.1, 1.1), (0.9, 0.1), (np.nan, 0.9), (0.1, np.nan), (0.1, np.inf), (-np.inf, 0.5)])
def test_quantiles_out_of_order_or_range_are_refused(gridpp, setup, q0, q1):
    with pytest.raises(ValueError, match="min_quantile and max_quantile must be finite with 0 <= min_quantile <= max_quantile <= 1"):
        call(gridpp, setup, q0=q0, q1=q1)
    # the C entry point refuses them itself
    s = setup
    out = np.empty((3, 4), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = gridpp._capi.lib()
    rc = lib.gpp_local_distribution_correction(s["grid"]._h, p(s["bg"]), s["points"]._h, p(s["pobs"]), p(s["pbg"]), 2, C.byref(s["st"]._s),
                                               q0, q1, 5, p(out), 0)
    assert rc == EINVAL and b"min_quantile" in lib.gpp_last_error()


def test_the_c_entry_point_checks_the_coordinate_types(gridpp, setup):
    s = setup
    out = np.empty((3, 4), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = gridpp._capi.lib()
    geodetic = gridpp.Points([0, 0, 0, 0, 0], [0, 1, 2, 3, 4])
    rc = lib.gpp_local_distribution_correction(s["grid"]._h, p(s["bg"]), geodetic._h, p(s["pobs"]), p(s["pbg"]), 2, C.byref(s["st"]._s),
                                               0.1, 0.9, 5, p(out), 0)
    assert rc == EINVAL and b"same coordinate type" in lib.gpp_last_error()


def test_an_empty_grid_gives_an_empty_result(gridpp, setup):
    empty = gridpp.Grid(((),), ((),), ((),), ((),), gridpp.Cartesian)
    out = call(gridpp, setup, grid=empty, bg=np.zeros((0, 0)))
    assert np.shape(out) == (0, 0)


def test_any_min_points_and_equal_quantiles_are_legal(gridpp, setup):
    """they reach the device: the only failure left on a machine without one is the missing device"""
    has_device = gridpp.device_count() > 0
    for kw in (dict(n=-3), dict(n=0), dict(n=10 ** 6), dict(q0=0.5, q1=0.5), dict(q0=0.0, q1=0.0), dict(q0=1.0, q1=1.0),
               dict(pobs=np.ones(5), pbg=np.ones(5)),                                        # the 1-D overload
               dict(pobs=[[1.0] * 5], pbg=[[2.0] * 5]), dict(bg=np.ones((3, 4), np.float64)),  # lists, float64
               dict(points=gridpp.Points((), (), (), (), gridpp.Cartesian), pobs=np.zeros((2, 0)), pbg=np.zeros((2, 0)))):
        if has_device:
            assert np.shape(call(gridpp, setup, **kw)) == (3, 4)
        else:
            with pytest.raises(RuntimeError, match="no HIP device"):
                call(gridpp, setup, **kw)
