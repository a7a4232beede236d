"""CPU: gridpp.window through `import gridpp` and through the C-ABI without a GPU -- the name and its defaults, both ValueErrors and
their order against the empty shapes (src/api/window.cpp:10-28), the empty shapes without a device, the statistics refused before
device work, "no HIP device" for a real call where no GPU is visible, the constants of include/gridpp_hip.h against their Python
mirror, and the C++ declaration in gridpp_amd/host/gridpp.hpp."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import window_ref as R

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


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def test_name_and_defaults(gridpp):
    import gridpp_amd
    assert gridpp.window is gridpp_amd.window
    sig = inspect.signature(gridpp.window)
    assert list(sig.parameters) == ["array", "length", "statistic", "before", "keep_missing", "missing_edges"]   # include/gridpp.h:1611
    assert [p.default for p in sig.parameters.values()][3:] == [False, False, True]
    assert [p.default for p in sig.parameters.values()][:3] == [inspect.Parameter.empty] * 3


def test_tile_constants_follow_the_header(gridpp):
    from gridpp_amd import _capi
    text = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    defs = dict(re.findall(r"#define (GPP_WINDOW_[A-Z_]+) (\d+)", text))
    assert {k: int(v) for k, v in defs.items()} == {"GPP_WINDOW_TILE_ROWS": _capi.WINDOW_TILE_ROWS, "GPP_WINDOW_TILE_COLS": _capi.WINDOW_TILE_COLS,
                                                    "GPP_WINDOW_FUSED_SPAN": _capi.WINDOW_FUSED_SPAN}


@pytest.mark.parametrize("case", HOST_CASES, ids=[c["id"] for c in HOST_CASES])
def test_known_answers_that_need_no_device(gridpp, case):
    """the reference's empty shapes and invalid lengths"""
    R.check_case(case, gridpp)


def test_host_cases_are_the_empty_shapes_and_the_invalid_lengths():
    assert sorted(c["id"] for c in HOST_CASES) == ["invalid_length_0", "invalid_length_1", "no_anything", "no_cases", "no_times"]


def test_value_errors_and_their_order(gridpp):
    """window.cpp:10-28: the length first (whatever the shape), then the empty shapes, only then the odd-length rule"""
    for shape in ((0, 0), (0, 5), (5, 0), (5, 5)):
        for length in (0, -1, -1001):
            with pytest.raises(ValueError, match="Length variable must be > 0"):
                gridpp.window(np.zeros(shape), length, gridpp.Sum)
    for length in (2, 4, 1000):
        assert gridpp.window(np.zeros((0, 5)), length, gridpp.Sum).shape == (0, 0)
        assert gridpp.window(np.zeros((5, 0)), length, gridpp.Sum).shape == (5, 0)
        with pytest.raises(ValueError, match="Length variable must be an odd number"):
            gridpp.window(np.zeros((5, 5)), length, gridpp.Sum)
        with pytest.raises(ValueError, match="Length variable must be an odd number"):
            gridpp.window(np.zeros((5, 5)), length, gridpp.Max, False)


def test_empty_shapes_without_a_device(gridpp):
    for statistic in (gridpp.Sum, gridpp.Median, gridpp.Quantile, gridpp.Unknown):   # (the reference never looks at the statistic of an empty call)
        for array, shape in ((np.zeros((0, 0)), (0, 0)), (np.zeros((0, 10), np.float32), (0, 0)), (np.zeros((10, 0)), (10, 0)), ([], (0, 0)), ([[]], (1, 0)),
                             ([[], []], (2, 0))):
            out = gridpp.window(array, 3, statistic)
            assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == shape


def test_statistics_refused_before_device_work(gridpp):
    """calc_statistic throws for Quantile and Unknown inside the reference's loop (util.cpp:97-106): a RuntimeError here, before any
    device work (the same without a GPU) and after the argument checks"""
    for statistic in (gridpp.Quantile, gridpp.Unknown, 7, 100):
        with pytest.raises(RuntimeError, match="Cannot compute statistic"):
            gridpp.window(np.zeros((3, 4)), 3, statistic)
        with pytest.raises(ValueError, match="odd number"):
            gridpp.window(np.zeros((3, 4)), 2, statistic)


def test_c_abi_checks_before_device_work(lib):
    from gridpp_amd import _capi
    a, out = np.zeros(12, np.float32), np.full(12, 7, np.float32)

    def status(rc, code, message):
        assert rc == code
        assert message in lib.gpp_last_error().decode()

    for ny, nx in ((3, 4), (0, 4), (3, 0), (0, 0)):
        status(lib.gpp_window(ptr(a), ny, nx, 0, 70, 0, 0, 1, ptr(out), 0), _capi.GPP_EINVAL, "Length variable must be > 0")
        status(lib.gpp_window(ptr(a), ny, nx, -3, 70, 1, 0, 1, ptr(out), 0), _capi.GPP_EINVAL, "Length variable must be > 0")
    status(lib.gpp_window(ptr(a), 3, 4, 2, 70, 0, 0, 1, ptr(out), 0), _capi.GPP_EINVAL, "Length variable must be an odd number")
    for statistic in (40, -1, 7):
        status(lib.gpp_window(ptr(a), 3, 4, 3, statistic, 0, 0, 1, ptr(out), 0), _capi.GPP_ERUNTIME, "Cannot compute statistic")
        status(lib.gpp_window(ptr(a), 3, 4, 2, statistic, 0, 0, 1, ptr(out), 0), _capi.GPP_EINVAL, "Length variable must be an odd number")
    # ny * nx == 0: GPP_OK, nothing written, no pointer looked at, whatever the parity of the length and the statistic
    for ny, nx in ((0, 4), (3, 0), (0, 0)):
        for length, statistic in ((3, 70), (2, 70), (3, 40)):
            assert lib.gpp_window(None, ny, nx, length, statistic, 0, 0, 1, None, 0) == _capi.GPP_OK
            assert lib.gpp_window(ptr(a), ny, nx, length, statistic, 0, 0, 1, ptr(out), 0) == _capi.GPP_OK
    assert np.all(out == 7)
    status(lib.gpp_window(None, 3, 4, 3, 70, 0, 0, 1, ptr(out), 0), _capi.GPP_EINVAL, "NULL")


def test_a_real_call_fails_loudly_without_a_gpu(gridpp, lib):
    """no CPU path behind window: "no HIP device" where none is visible (where one is, the call simply works)"""
    from gridpp_amd import _capi
    row = [[0, 1, 2, np.nan, 3, 4, 5]]
    if gridpp.device_count() > 0:
        np.testing.assert_array_equal(gridpp.window(row, 3, gridpp.Sum, False, False, False), [[1, 3, 3, 5, 7, 12, 9]])
        return
    for statistic in (gridpp.Sum, gridpp.Max, gridpp.RandomChoice):
        with pytest.raises(RuntimeError, match="no HIP device"):
            gridpp.window(row, 3, statistic)
    a, out = np.zeros(12, np.float32), np.zeros(12, np.float32)
    assert lib.gpp_window(ptr(a), 3, 4, 3, 70, 0, 0, 1, ptr(out), 0) == _capi.GPP_ENODEVICE


def test_cpp_mirror_declares_window_with_the_reference_defaults():
    hpp = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp.hpp")).read()
    assert re.search(r"inline vec2 window\(const vec2& array, int length, Statistic statistic, bool before = false, bool keep_missing = false, "
                     r"bool missing_edges = true\)", hpp)
    body = hpp[hpp.index("inline vec2 window("):]
    body = body[:body.index("\n}\n")]
    assert "gpp_window(" in body and 'std::invalid_argument("Length variable must be > 0")' in body
    header = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    assert re.search(r"int gpp_window\(const float\* array, long long ny, int nx, int length, int statistic, int before, int keep_missing, "
                     r"int missing_edges,\s+float\* out, int mem\);", header)
    assert "src/api/window.cpp:6-156" in header
