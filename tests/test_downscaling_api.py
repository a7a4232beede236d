"""CPU: downscaling / simple_gradient / full_gradient exist under both import names, raise the reference's argument errors
before any device work, and fail loudly (no CPU path) when there is no GPU."""
import numpy as np
import pytest

from tests import downscaling_ref as R


@pytest.fixture(scope="module")
def gridpp():
    import __graft_entry__ as g
    g.build()
    import gridpp_amd
    return gridpp_amd


def _grid(gridpp, Y=3, X=3):
    lons, lats = np.meshgrid(np.arange(X) * 10.0, 30 + np.arange(Y) * 10.0)
    return gridpp.Grid(lats, lons, np.zeros((Y, X)), np.full((Y, X), 0.5))


def test_names_are_the_same_objects_through_import_gridpp(gridpp):
    import gridpp as alias
    for name in ("Nearest", "Bilinear", "downscaling", "simple_gradient", "full_gradient"):
        assert getattr(alias, name) is getattr(gridpp, name)
    assert (gridpp.Nearest, gridpp.Bilinear) == (0, 1)


def _make(gridpp, d):
    lats, lons, elevs, lafs = R.set_arrays(d)
    if d["type"] == "grid":
        return gridpp.Grid(lats, lons, elevs if elevs is not None else ((),), lafs if lafs is not None else ((),))
    return gridpp.Points(lats, lons, elevs if elevs is not None else (), lafs if lafs is not None else ())


ERRORS = [c for c in R.known_answers() if "error" in c]


@pytest.mark.parametrize("case", ERRORS, ids=[c["id"] for c in ERRORS])
def test_known_answer_errors(gridpp, case):
    lats, lons, elevs, _ = R.set_arrays(case["igrid"])
    igrid = gridpp.Grid(lats, lons, elevs if elevs is not None else ((),))
    out = _make(gridpp, case["output"])
    f = getattr(gridpp, case["function"])
    with pytest.raises(ValueError, match="Grid size is not the same as values"):
        if case["function"] == "downscaling":
            f(igrid, out, np.asarray(case["values"]), gridpp.Nearest)
        else:
            f(igrid, out, np.asarray(case["values"]), case["elev_gradient"])


def test_value_errors_before_device_work(gridpp):
    g, p = _grid(gridpp), gridpp.Points([30, 40], [0, 10], [0, 0], [0, 1])
    v2, v3 = np.zeros((3, 3)), np.zeros((2, 3, 3))
    raises = [
        (lambda: gridpp.downscaling(g, p, v2, 2), "Invalid downscaler"),
        (lambda: gridpp.downscaling(g, g, v3, -1), "Invalid downscaler"),
        (lambda: gridpp.simple_gradient(g, p, v2, 1.0, 7), "Invalid downscaler"),
        (lambda: gridpp.full_gradient(g, g, v2, v2, v2, 3), "Invalid downscaler"),
        (lambda: gridpp.simple_gradient(g, p, np.zeros((3, 2)), 1.0), "Grid size is not the same as values"),
        (lambda: gridpp.simple_gradient(g, g, np.zeros((2, 3, 2)), 1.0), "Grid size is not the same as values"),
        (lambda: gridpp.full_gradient(g, g, np.zeros((3, 2)), v2, v2), "Values is the wrong size"),
        (lambda: gridpp.full_gradient(g, g, np.zeros((0, 3)), v2, v2), "Values is the wrong size"),
        (lambda: gridpp.full_gradient(g, g, v2, np.zeros((3, 2)), v2), "Elevation gradient is the wrong size"),
        (lambda: gridpp.full_gradient(g, g, v2, v2, np.zeros((2, 3))), "Laf gradient is the wrong size"),
        (lambda: gridpp.full_gradient(g, g, v2, np.zeros((3, 2)), np.zeros((2, 3))), "Laf gradient is the wrong size"),   # gradient.cpp:13-20 order
        (lambda: gridpp.full_gradient(g, p, np.zeros((3, 2)), v2, v2), "Grid size is not the same as values"),
        (lambda: gridpp.full_gradient(g, p, v2, np.zeros((3, 2)), v2), "Elevation gradient is the wrong size"),
        # the overloads where the reference only asserts (and would read past the end)
        (lambda: gridpp.full_gradient(g, g, v3, np.zeros((1, 3, 3)), v3), "Elevation gradient is the wrong size"),
        (lambda: gridpp.full_gradient(g, g, v3, v3, np.zeros((3, 3, 3))), "Laf gradient is the wrong size"),
        (lambda: gridpp.full_gradient(g, p, v3, v2, v3), "Elevation gradient is the wrong size"),
        (lambda: gridpp.full_gradient(g, p, v3, v3, np.zeros((2, 3, 2))), "Laf gradient is the wrong size"),
        # values that are empty while the grid is not: nothing to read
        (lambda: gridpp.simple_gradient(g, p, np.zeros((0, 3)), 1.0), "Grid size is not the same as values"),
        (lambda: gridpp.full_gradient(g, p, np.zeros((2, 0, 3)), [], []), "Grid size is not the same as values"),
    ]
    for f, msg in raises:
        with pytest.raises(ValueError, match=msg):
            f()


def test_type_errors(gridpp):
    g, p = _grid(gridpp), gridpp.Points([30, 40], [0, 10])
    v2 = np.zeros((3, 3))
    for f in (lambda: gridpp.downscaling(p, p, v2, 0), lambda: gridpp.simple_gradient(p, g, v2, 1.0),
              lambda: gridpp.full_gradient(p, g, v2, v2, v2),
              # only the Grid -> Grid 2-D overload has a default laf_gradient (include/gridpp.h:1065-1098)
              lambda: gridpp.full_gradient(g, p, v2, v2), lambda: gridpp.full_gradient(g, g, np.zeros((2, 3, 3)), np.zeros((2, 3, 3)))):
        with pytest.raises(TypeError):
            f()


def test_empty_output_gives_empty_result(gridpp):
    g = _grid(gridpp)
    e = gridpp.Points([], [])
    assert np.shape(gridpp.simple_gradient(g, e, np.zeros((3, 3)), 1.0)) == (0,)
    assert np.shape(gridpp.full_gradient(g, e, np.zeros((4, 3, 3)), np.zeros((4, 3, 3)), [])) == (4, 0)
    assert np.shape(gridpp.full_gradient(g, g, np.zeros((0, 3, 3)), np.zeros((0, 3, 3)), [])) == (0, 3, 3)


def test_compute_fails_loudly_without_gpu(gridpp):
    if gridpp.device_count() > 0:
        pytest.skip("a GPU is visible")
    g, p = _grid(gridpp), gridpp.Points([30, 40], [0, 10], [0, 0], [0, 1])
    v2, v3 = np.zeros((3, 3)), np.zeros((2, 3, 3))
    for f in (lambda: gridpp.simple_gradient(g, p, v2, 1.0), lambda: gridpp.simple_gradient(g, g, v3, 1.0, gridpp.Bilinear),
              lambda: gridpp.full_gradient(g, g, v2, v2), lambda: gridpp.full_gradient(g, p, v3, v3, [], gridpp.Bilinear),
              lambda: gridpp.downscaling(g, p, v2, gridpp.Bilinear)):
        with pytest.raises(RuntimeError, match="no HIP device"):
            f()
    with pytest.raises(RuntimeError):   # (the dispatch to nearest, whose message is the HIP runtime's)
        gridpp.downscaling(g, g, v3, gridpp.Nearest)
