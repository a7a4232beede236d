"""CPU: calc_score / neighbourhood_score and the Metric constants through `import gridpp` and through the C-ABI without a GPU -- the
names, the enum values, the scalar calc_score against the reference's known answers and the hand-worked guard branches (Python and
gpp_calc_score_table, bit for bit against tests/score_ref.py), every ValueError and their order, the empty shapes without a device,
"no HIP device" for a real call where no GPU is visible, the constants of include/gridpp_hip.h against their Python mirror, and the
C++ declarations in gridpp_amd/host/gridpp.hpp."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("Ets", "Ts", "Kss", "Pc", "Bias", "Hss")


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


def table(lib, a, b, c, d, metric):
    out = C.c_float(7)
    rc = lib.gpp_calc_score_table(a, b, c, d, metric, C.byref(out))
    return rc, np.float32(out.value)


def test_names_and_enum_values(gridpp):
    import gridpp_amd
    assert gridpp.calc_score is gridpp_amd.calc_score
    assert gridpp.neighbourhood_score is gridpp_amd.neighbourhood_score
    for name in NAMES:
        assert getattr(gridpp, name) == R.METRIC[name] == getattr(R, name)
    header = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    defs = dict(re.findall(r"#define GPP_METRIC_([A-Z]+) (\d+)", header))
    assert {k.capitalize(): int(v) for k, v in defs.items()} == R.METRIC


def test_constants_follow_the_header(gridpp):
    from gridpp_amd import _capi
    text = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    defs = dict(re.findall(r"#define (GPP_SCORE_[A-Z_]+) (\d+)", text))
    assert {k: int(v) for k, v in defs.items()} == {"GPP_SCORE_FUSED_MAXHW": _capi.SCORE_FUSED_MAXHW, "GPP_SCORE_TILE_COLS": _capi.SCORE_TILE_COLS,
                                                    "GPP_SCORE_TILE_ROWS": _capi.SCORE_TILE_ROWS}
    assert (2 * _capi.SCORE_FUSED_MAXHW + 1) ** 2 < 65536   # the packing bound of the fused kernel


def tables():
    """contingency tables: what the known answers count, the guard rows, and fractions as neighbourhood_score forms them"""
    k = R.KNOWN
    rows = [R.counts(k["obs"], k["fcst"], t, t) for t in k["thresholds"]]
    rows += [r[:4] for r in R.GUARDS]
    rng = np.random.default_rng(11)
    for _ in range(200):
        n = rng.integers(0, 40, 4)
        area = max(int(n.sum()) + int(rng.integers(0, 30)), 1)
        rows.append(tuple(np.float32(np.float64(v) / area) for v in n))
    rows += [(1e30, 1e30, 1e30, 1e30), (np.nan, 1, 1, 1), (np.inf, 1, 2, 3), (16777216, 0, 0, 0)]
    return rows


@pytest.mark.parametrize("name", NAMES)
def test_scalar_calc_score_through_python_and_the_c_abi(gridpp, lib, name):
    from gridpp_amd import _capi
    metric = R.METRIC[name]
    for a, b, c, d in tables():
        want = R.calc_score_table(a, b, c, d, metric)
        got = gridpp.calc_score(a, b, c, d, metric)
        assert isinstance(got, float)
        R.same_bits(np.float32(got), want)
        rc, got = table(lib, a, b, c, d, metric)
        assert rc == _capi.GPP_OK
        R.same_bits(got, want)


def test_known_answers_of_the_reference_as_tables(gridpp):
    k = R.KNOWN
    for name in NAMES:
        for t, threshold in enumerate(k["thresholds"]):
            a, b, c, d = R.counts(k["obs"], k["fcst"], threshold, threshold)
            want = k["expected"][name][t]
            np.testing.assert_almost_equal(gridpp.calc_score(a, b, c, d, getattr(gridpp, name)), np.nan if want is None else want, R.GOLDEN["decimals"])


@pytest.mark.parametrize("row", R.GUARDS, ids=["%s-%d-%d-%d-%d" % (r[4], r[0], r[1], r[2], r[3]) for r in R.GUARDS])
def test_guard_branches(gridpp, row):
    a, b, c, d, name, want = row
    got = gridpp.calc_score(a, b, c, d, getattr(gridpp, name))
    assert np.isnan(got) if want is None else got == want


def test_unknown_metric(gridpp, lib):
    from gridpp_amd import _capi
    for metric in (2, -1, 10, 60, 51):
        with pytest.raises(ValueError, match="Unknown metric"):
            gridpp.calc_score(1, 1, 1, 1, metric)
        with pytest.raises(ValueError, match="Unknown metric"):
            gridpp.calc_score([1.0], [1.0], 0.5, metric)
        with pytest.raises(ValueError, match="Unknown metric"):
            gridpp.calc_score([], [], 0.5, 0.5, metric)
        rc, out = table(lib, 1, 1, 1, 1, metric)
        assert rc == _capi.GPP_EINVAL and out == 7 and b"Unknown metric" in lib.gpp_last_error()
        out = C.c_float(7)
        a = np.ones(3, np.float32)
        assert lib.gpp_calc_score(ptr(a), ptr(a), 3, 0.5, 0.5, metric, C.byref(out), 0) == _capi.GPP_EINVAL and out.value == 7
    with pytest.raises(TypeError):
        gridpp.calc_score(1, 1, 1)


def test_vector_calc_score_checks_and_empty_input_without_a_device(gridpp, lib):
    from gridpp_amd import _capi
    with pytest.raises(ValueError, match="ref and fcst not the same size"):
        gridpp.calc_score([1.0], [1.0, 2.0], 0.5, gridpp.Pc)
    with pytest.raises(ValueError, match="ref and fcst not the same size"):
        gridpp.calc_score([], [1.0], 0.5, 0.5, gridpp.Pc)
    for ref in ([], [3.0, 4.0], np.zeros(0)):      # nothing to count: all four counts are 0, whatever ref holds beyond fcst
        assert gridpp.calc_score(ref, [], 0.5, gridpp.Bias) == 1
        assert gridpp.calc_score(ref, [], 0.5, 0.7, gridpp.Bias) == 1
        for name in ("Ets", "Ts", "Kss", "Pc", "Hss"):
            assert np.isnan(gridpp.calc_score(ref, [], 0.5, getattr(gridpp, name)))
    out = C.c_float(7)
    assert lib.gpp_calc_score(None, None, 0, 0.5, 0.5, 40, C.byref(out), 0) == _capi.GPP_OK and out.value == 1
    assert lib.gpp_calc_score(None, None, 0, 0.5, 0.5, 30, C.byref(out), 0) == _capi.GPP_OK and np.isnan(out.value)
    assert lib.gpp_calc_score(None, None, -1, 0.5, 0.5, 30, C.byref(out), 0) == _capi.GPP_EINVAL
    assert lib.gpp_calc_score(None, None, 3, 0.5, 0.5, 30, C.byref(out), 0) == _capi.GPP_EINVAL and b"NULL" in lib.gpp_last_error()


def small(gridpp):
    lats, lons = R.geometry(3, 4, True)
    return gridpp.Grid(lats, lons), gridpp.Points([60.0, 60.01], [10.0, 10.02]), np.ones((3, 4)), [1.0, 0.0]


def test_neighbourhood_score_value_errors_and_their_order(gridpp):
    """neighbourhood_score.cpp:8-14, calc_score's metric check, then gridding_nearest's size check (gridding.cpp:72-73)"""
    grid, points, fcst, ref = small(gridpp)
    bad_fcst, bad_ref = np.ones((4, 3)), [1.0]
    with pytest.raises(ValueError, match="Grid size is not the same as forecast values"):
        gridpp.neighbourhood_score(grid, points, bad_fcst, bad_ref, 0, 99, 0.5)
    with pytest.raises(ValueError, match="half_width must be greater than 0"):
        gridpp.neighbourhood_score(grid, points, fcst, bad_ref, 0, 99, 0.5)
    with pytest.raises(ValueError, match="half_width must be greater than 0"):
        gridpp.neighbourhood_score(grid, points, fcst, ref, -3, gridpp.Ets, 0.5)
    with pytest.raises(ValueError, match="Unknown metric"):
        gridpp.neighbourhood_score(grid, points, fcst, bad_ref, 1, 99, 0.5)
    with pytest.raises(ValueError, match="Points size is not the same as values"):
        gridpp.neighbourhood_score(grid, points, fcst, bad_ref, 1, gridpp.Ets, 0.5)
    with pytest.raises(ValueError, match="Grid size is not the same as forecast values"):   # the reference reads fcst[0] of an empty vector
        gridpp.neighbourhood_score(grid, points, np.zeros((0, 0)), ref, 1, gridpp.Ets, 0.5)


def test_neighbourhood_score_of_an_empty_grid_needs_no_device(gridpp):
    empty = gridpp.Grid()
    for fcst in (np.zeros((0, 0)), [], np.zeros((0, 0), np.float32)):
        out = gridpp.neighbourhood_score(empty, gridpp.Points([60.0], [10.0]), fcst, [1.0], 2, gridpp.Ets, 0.5)
        assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (0, 0)
    with pytest.raises(ValueError, match="half_width"):
        gridpp.neighbourhood_score(empty, gridpp.Points(), [], [], 0, gridpp.Ets, 0.5)
    with pytest.raises(ValueError, match="Grid size"):
        gridpp.neighbourhood_score(empty, gridpp.Points(), np.ones((2, 2)), [], 1, gridpp.Ets, 0.5)


def test_c_abi_checks_before_device_work(gridpp, lib):
    from gridpp_amd import _capi
    grid, points, _, _ = small(gridpp)
    f, r, out = np.ones(12, np.float32), np.ones(2, np.float32), np.full(12, 7, np.float32)

    def status(rc, code, message):
        assert rc == code
        assert message in lib.gpp_last_error().decode()

    status(lib.gpp_neighbourhood_score(grid._h, points._h, ptr(f), ptr(r), 0, 99, 0.5, ptr(out), 0), _capi.GPP_EINVAL, "half_width must be greater than 0")
    status(lib.gpp_neighbourhood_score(grid._h, points._h, ptr(f), ptr(r), -1, 0, 0.5, ptr(out), 0), _capi.GPP_EINVAL, "half_width must be greater than 0")
    status(lib.gpp_neighbourhood_score(grid._h, points._h, ptr(f), ptr(r), 1, 99, 0.5, ptr(out), 0), _capi.GPP_EINVAL, "Unknown metric")
    status(lib.gpp_neighbourhood_score(None, points._h, ptr(f), ptr(r), 1, 0, 0.5, ptr(out), 0), _capi.GPP_EINVAL, "NULL")
    status(lib.gpp_neighbourhood_score(points._h, points._h, ptr(f), ptr(r), 1, 0, 0.5, ptr(out), 0), _capi.GPP_EINVAL, "not a Grid")
    status(lib.gpp_neighbourhood_score(grid._h, points._h, None, ptr(r), 1, 0, 0.5, ptr(out), 0), _capi.GPP_EINVAL, "NULL")
    assert lib.gpp_neighbourhood_score(gridpp.Grid()._h, points._h, None, ptr(r), 1, 0, 0.5, None, 0) == _capi.GPP_OK
    assert np.all(out == 7)


def test_a_real_call_fails_loudly_without_a_gpu(gridpp, lib):
    """no CPU path behind either function: "no HIP device" where none is visible (where one is, the calls simply work)"""
    from gridpp_amd import _capi
    grid, points, fcst, ref = small(gridpp)
    k = R.KNOWN
    if gridpp.device_count() > 0:
        np.testing.assert_almost_equal(gridpp.calc_score(k["obs"], k["fcst"], 1.5, gridpp.Pc), 0.333, 3)
        assert gridpp.neighbourhood_score(grid, points, fcst, ref, 1, gridpp.Pc, 0.5).shape == (3, 4)
        return
    with pytest.raises(RuntimeError, match="no HIP device"):
        gridpp.calc_score(k["obs"], k["fcst"], 1.5, gridpp.Pc)
    with pytest.raises(RuntimeError, match="no HIP device"):
        gridpp.calc_score(k["obs"], k["fcst"], 1.5, 1.5, gridpp.Pc)
    with pytest.raises(RuntimeError, match="no HIP device"):
        gridpp.neighbourhood_score(grid, points, fcst, ref, 1, gridpp.Pc, 0.5)
    a, out = np.ones(3, np.float32), C.c_float(7)
    assert lib.gpp_calc_score(ptr(a), ptr(a), 3, 0.5, 0.5, 30, C.byref(out), 0) == _capi.GPP_ENODEVICE and out.value == 7


def test_cpp_mirror_declares_the_reference_signatures():
    hpp = open(os.path.join(ROOT, "gridpp_amd", "host", "gridpp.hpp")).read()
    assert re.search(r"enum Metric \{ Ets = 0, Ts = 1, Kss = 20, Pc = 30, Bias = 40, Hss = 50 \};", hpp)
    assert re.search(r"inline float calc_score\(float a, float b, float c, float d, Metric metric\)", hpp)
    assert re.search(r"inline float calc_score\(const vec& ref, const vec& fcst, float threshold, Metric metric\)", hpp)
    assert re.search(r"inline float calc_score\(const vec& ref, const vec& fcst, float threshold, float fthreshold, Metric metric\)", hpp)
    assert re.search(r"inline vec2 neighbourhood_score\(const Grid& grid, const Points& points, const vec2& fcst, const vec& ref, int half_width, "
                     r"Metric metric, float threshold\)", hpp)
    body = hpp[hpp.index("inline vec2 neighbourhood_score("):]
    body = body[:body.index("\n}\n")]
    assert "gpp_neighbourhood_score(" in body
    order = [body.index(m) for m in ("Grid size is not the same as forecast values", "half_width must be greater than 0", "calc_score(0, 0, 0, 0, metric)",
                                     "Points size is not the same as values")]
    assert order == sorted(order)
    header = open(os.path.join(ROOT, "include", "gridpp_hip.h")).read()
    assert re.search(r"int gpp_calc_score_table\(float a, float b, float c, float d, int metric, float\* out\);", header)
    assert re.search(r"int gpp_calc_score\(const float\* ref, const float\* fcst, long long n, float threshold, float fthreshold, int metric, float\* out, "
                     r"int mem\);", header)
    assert re.search(r"int gpp_neighbourhood_score\(gpp_points\* grid, gpp_points\* points, const float\* fcst, const float\* ref, int half_width, "
                     r"int metric,\s+float threshold, float\* out, int mem\);", header)
    assert "src/api/neighbourhood_score.cpp" in header and "metric_optimizer.cpp:207-244" in header
