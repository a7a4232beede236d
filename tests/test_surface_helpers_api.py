"""CPU-only: the container-side helpers of include/gridpp.h (is_valid_lat / is_valid_lon, num_missing_values, init_*,
compatible_size), on gridpp_amd and on its alias.  The values are those of the reference's tests/test_util.py:138-145,164-183,
194-212 and tests/test_init_vec.py, plus the edges src/api/util.cpp:427-474,617-624 spell out."""
import numpy as np
import pytest


@pytest.fixture(scope="module", params=["gridpp_amd", "gridpp"])
def g(request):
    import importlib
    return importlib.import_module(request.param)


def test_is_valid_lat(g):
    for v in (0, -90, 90, 90.001, -90.001):          # the bound is +-90.001 (util.cpp:620): 90.001f lies just inside it
        assert g.is_valid_lat(v, g.Geodetic) is True
    for v in (-91, 91, 90.002, -90.002, np.nan, np.inf, -np.inf):
        assert g.is_valid_lat(v, g.Geodetic) is False
    for v in (0, 91, -1e6, 3.5e7):                   # a Cartesian y is any valid value
        assert g.is_valid_lat(v, g.Cartesian) is True
    for v in (np.nan, np.inf):
        assert g.is_valid_lat(v, g.Cartesian) is False


def test_is_valid_lon(g):
    for ctype in (g.Geodetic, g.Cartesian):
        for v in (-1000, -180, 0, 180, 1000):
            assert g.is_valid_lon(v, ctype) is True
        for v in (np.nan, np.inf, -np.inf):
            assert g.is_valid_lon(v, ctype) is False


def test_num_missing_values(g):
    nan = np.nan
    assert g.num_missing_values([[0, nan, 1, nan]]) == 2
    assert g.num_missing_values([[nan, nan]]) == 2
    assert g.num_missing_values([[0, 0, 1, 1]]) == 0
    assert g.num_missing_values([[0, nan], [1, nan]]) == 2
    assert g.num_missing_values([[nan, nan], [nan, nan]]) == 4
    assert g.num_missing_values([[0, 0], [1, 1]]) == 0
    assert g.num_missing_values([[]]) == 0
    assert g.num_missing_values(np.zeros((0, 0))) == 0
    assert g.num_missing_values([[np.inf, -np.inf, 1e38, 0]]) == 2     # is_valid: neither NaN nor infinite
    assert isinstance(g.num_missing_values([[0, nan]]), int)


def test_init_vec2(g):
    for func, dtype in ((g.init_vec2, np.float32), (g.init_ivec2, np.int32)):
        np.testing.assert_array_equal(func(2, 2, -1), [[-1, -1], [-1, -1]])
        np.testing.assert_array_equal(func(1, 2, -1), [[-1, -1]])
        np.testing.assert_array_equal(func(2, 1, -1), [[-1], [-1]])
        assert func(2, 3, -1).dtype == dtype and func(2, 3, -1).shape == (2, 3) and func(0, 3, -1).shape == (0, 3)
    out = g.init_vec2(3, 2)                          # value = MV
    assert out.shape == (3, 2) and out.dtype == np.float32 and np.isnan(out).all()


def test_init_vec3(g):
    X = -1
    for func, dtype in ((g.init_vec3, np.float32), (g.init_ivec3, np.int32)):
        np.testing.assert_array_equal(func(2, 2, 3, X), [[[X, X, X], [X, X, X]], [[X, X, X], [X, X, X]]])
        np.testing.assert_array_equal(func(1, 2, 3, X), [[[X, X, X], [X, X, X]]])
        np.testing.assert_array_equal(func(2, 1, 3, X), [[[X, X, X]], [[X, X, X]]])
        np.testing.assert_array_equal(func(2, 2, 1, X), [[[X], [X]], [[X], [X]]])
        assert func(2, 3, 4, X).dtype == dtype and func(2, 3, 4, X).shape == (2, 3, 4)
    out = g.init_vec3(1, 2, 3)
    assert out.shape == (1, 2, 3) and out.dtype == np.float32 and np.isnan(out).all()


@pytest.fixture(scope="module")
def grid(g):
    lons, lats = np.meshgrid([0, 10, 20, 30], [30, 40, 50])
    return g.Grid(lats, lons)  # 3 x 4


def test_compatible_size_grid_vec2(g, grid):
    assert g.compatible_size(grid, np.zeros([2, 4])) is False
    assert g.compatible_size(grid, np.zeros([3, 4])) is True
    assert g.compatible_size(grid, np.zeros([4, 3])) is False
    assert g.compatible_size(grid, []) is True                       # v.size() == 0 (util.cpp:428)
    assert g.compatible_size(grid, np.zeros([0, 4])) is True


def test_compatible_size_grid_vec3(g, grid):
    assert g.compatible_size(grid, np.zeros([3, 2, 4])) is False
    assert g.compatible_size(grid, np.zeros([3, 3, 4])) is True
    assert g.compatible_size(grid, np.zeros([7, 3, 4])) is True      # the first size is free
    assert g.compatible_size(grid, np.zeros([0, 3, 4])) is True      # v.size() == 0 (:431)
    assert g.compatible_size(grid, np.zeros([2, 0, 4])) is True      # v[0].size() == 0 (:431)
    assert g.compatible_size(grid, np.zeros([2, 3, 5])) is False


def test_compatible_size_points(g):
    points = g.Points([0, 1, 2], [0, 1, 2])
    assert g.compatible_size(points, [0, 0, 0]) is True
    assert g.compatible_size(points, [0, 0]) is False
    assert g.compatible_size(g.Points(), []) is True
    assert g.compatible_size(points, np.zeros([1, 3])) is True
    assert g.compatible_size(points, np.zeros([2, 3])) is True
    assert g.compatible_size(points, np.zeros([3, 2])) is False
    assert g.compatible_size(points, np.zeros([0, 2])) is True       # v.size() == 0 (:434)


def test_compatible_size_arrays(g):
    z = np.zeros
    # (vec2, vec2), :439-447
    assert g.compatible_size(z([2, 3]), z([2, 3])) is True
    assert g.compatible_size(z([2, 3]), z([2, 4])) is False
    assert g.compatible_size(z([2, 3]), z([3, 3])) is False
    assert g.compatible_size(z([0, 0]), z([0, 0])) is True
    # (vec2, vec3), :448-461: the first two sizes only
    assert g.compatible_size(z([2, 3]), z([2, 3, 9])) is True
    assert g.compatible_size(z([2, 3]), z([2, 4, 9])) is False
    assert g.compatible_size(z([2, 3]), z([3, 3, 9])) is False
    assert g.compatible_size(z([0, 0]), z([0, 0, 0])) is True        # no y
    assert g.compatible_size(z([2, 0]), z([2, 0, 0])) is True        # no x
    assert g.compatible_size(z([2, 0]), z([2, 1, 0])) is False
    # (vec3, vec3), :462-474
    assert g.compatible_size(z([2, 3, 4]), z([2, 3, 4])) is True
    assert g.compatible_size(z([2, 3, 4]), z([2, 3, 5])) is False
    assert g.compatible_size(z([2, 3, 4]), z([2, 2, 4])) is False
    assert g.compatible_size(z([2, 3, 4]), z([1, 3, 4])) is False
    with pytest.raises(TypeError):
        g.compatible_size(z([2]), z([2]))
