"""fill_missing, calc_gradient, neighbourhood_search, fill and doping on the device against the C oracle at the edges of the kernels
of gridpp_amd/csrc/gridops.hip.  The cases, their references and the proofs that they can tell a wrong kernel from a right one live
in tests/gridops_cases.py and tests/test_gridops_cases_oracle.py (no GPU).  Every comparison is bit for bit (NaN equals NaN) except
the LinearRegression gradient, which keeps the tolerances of tests/test_gpu_gridops_parity.py.

Which path of gpp_fill_missing a shape reaches (the choice is `nx <= FM_MAXX && ny <= FM_MAXX`, FM_MAXX = 8192, and no
GPP_FILL_MISSING_LINES; a thread of k_fill_missing_rows owns ceil(line / 256) elements):
  (3, 255) (3, 256)            rows: segment length 1, the last thread idle for 255; columns (lines of 3): one element, 253 idle threads
  (3, 257) (4, 511) (4, 512)   rows: segment length 2 -- 257 leaves threads 129 .. 255 without a segment, 511 a last segment of one
  (300, 300)                   segment length 2 in both passes, 300 workgroups each; k_transpose over 10 x 10 tiles with ragged edges
  (4, 513)                     segment length 3 (171 segments, 85 threads without one)
  (5, 1000)                    rows: segment length 4 (250 segments); columns: lines of 5
  (1000, 5)                    the transposed pass: the 1000-element lines are the rows of the transposed field (k_transpose,
                               k_fill_missing_rows on (5, 1000), k_transpose back); the direct row pass sees lines of 5
  (2, 8191) (2, 8192)          segment length 32; 8192 writes the last entries of s_v / s_next, 8191 leaves thread 255 one short
  (2, 8193) (8193, 2) (3, 8200)  one side beyond FM_MAXX: both passes go to k_fill_missing_lines (one thread per line) with no
                               environment variable set, whichever axis is the long one
Every case also runs with GPP_FILL_MISSING_LINES=1 (k_fill_missing_lines for both passes at every shape) and nine of them with the
field resident on the device (GPP_MEM_DEVICE: no staging)."""
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import gridops_cases as K

pytestmark = pytest.mark.gpu
LINES = "GPP_FILL_MISSING_LINES"


def _gridpp():
    import gridpp_amd as gridpp
    return gridpp


def _cuda(a):
    import torch
    return torch.tensor(np.asarray(a)).cuda()


# ---- fill_missing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.FM_CASES)
def test_fill_missing_both_paths(name, monkeypatch):
    gridpp = _gridpp()
    field, ref = K.fill_missing_case(name), K.fill_missing_reference(name)
    assert_array_equal(np.asarray(gridpp.fill_missing(field)), ref)
    monkeypatch.setenv(LINES, "1")
    assert_array_equal(np.asarray(gridpp.fill_missing(field)), ref)


@pytest.mark.parametrize("name", K.FM_DEVICE_CASES)
def test_fill_missing_device_tensor(name):
    out = _gridpp().fill_missing(_cuda(K.fill_missing_case(name)))
    assert out.is_cuda
    assert_array_equal(out.cpu().numpy(), K.fill_missing_reference(name))


@pytest.mark.parametrize("name, field, expected", K.fill_missing_known_answers(), ids=[k[0] for k in K.fill_missing_known_answers()])
def test_fill_missing_known_answers(name, field, expected, monkeypatch):
    gridpp = _gridpp()
    assert_array_equal(np.asarray(gridpp.fill_missing(field)), expected)
    assert_array_equal(gridpp.fill_missing(_cuda(field)).cpu().numpy(), expected)
    monkeypatch.setenv(LINES, "1")
    assert_array_equal(np.asarray(gridpp.fill_missing(field)), expected)


# ---- calc_gradient --------------------------------------------------------------------------------------------------------------
def test_gradient_type_constants():
    gridpp = _gridpp()
    assert (gridpp.MinMax, gridpp.LinearRegression, gridpp.Cartesian, gridpp.Geodetic) == (K.MINMAX, K.LINREG, K.CARTESIAN, K.GEODETIC)


@pytest.mark.parametrize("row", sorted(K.MINMAX_ROWS))
def test_minmax_with_ties(row):
    """integer base: every window holds its extremes several times, so `>=` or another walking order changes most cells
    (test_gridops_cases_oracle.py::test_minmax_case_tells_first_tie_from_last)"""
    gridpp = _gridpp()
    base, values = K.minmax_tie_case()
    ref = K.minmax_reference(row)
    assert_array_equal(np.asarray(gridpp.calc_gradient(base, values, K.MINMAX, *K.MINMAX_ROWS[row])), ref)
    assert_array_equal(gridpp.calc_gradient(_cuda(base), _cuda(values), K.MINMAX, *K.MINMAX_ROWS[row]).cpu().numpy(), ref)


def _linreg(row):
    base, values = K.linreg_case()
    return np.asarray(_gridpp().calc_gradient(base, values, K.LINREG, *K.LINREG_ROWS[row]))


def _close_to_oracle(out, ref):
    """the tolerances of test_gpu_gridops_parity.py::test_calc_gradient_matches_oracle"""
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    err = np.abs(out - ref) / np.maximum(np.abs(ref), 1e-9)
    print("LinearRegression: max rel err %.3g, median %.3g" % (np.nanmax(err), np.nanmedian(err)))
    np.testing.assert_allclose(out, ref, rtol=2e-3, atol=1e-6)
    assert np.median(err) < 1e-5


@pytest.mark.parametrize("row", sorted(K.LINREG_ROWS))
def test_linreg_matches_oracle(row):
    out, ref = _linreg(row), K.linreg_reference(row)
    _close_to_oracle(out, ref)
    dflt = np.float32(K.LINREG_DEFAULT)
    assert_array_equal(out == dflt, ref == dflt)              # the cells that take the default: count, variance and range tests agree


@pytest.mark.parametrize("row", ["block_hw2", "block_hw2_range"])
def test_linreg_constant_block_takes_the_default(row):
    out = _linreg(row)
    assert_array_equal(out[K.BLOCK_INNER], np.full_like(out[K.BLOCK_INNER], K.LINREG_DEFAULT))    # mXX - mX * mX == 0 exactly


def test_linreg_whole_field_window_gives_one_value():
    out, ref = _linreg("hw60"), K.linreg_reference("hw60")
    assert np.unique(out).size == 1 and np.unique(ref).size == 1
    _close_to_oracle(out, ref)


# ---- neighbourhood_search -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_apply", [False, True])
@pytest.mark.parametrize("row", sorted(K.SEARCH_ROWS))
def test_search_with_ties(row, with_apply):
    array, search, apply = K.search_case()
    out = _gridpp().neighbourhood_search(array, search, *K.SEARCH_ROWS[row], apply if with_apply else None)
    assert_array_equal(np.asarray(out), K.search_reference(row, with_apply))


@pytest.mark.parametrize("form", ["int32", "int64", "strided", "none"])
@pytest.mark.parametrize("row", sorted(K.SEARCH_ROWS))
def test_search_device_apply_array(row, form):
    """a CUDA apply_array goes to the kernel as a device pointer: contiguous int32 as it is, anything else through a copy"""
    import torch
    array, search, apply = K.search_case()
    if form == "none":
        d_apply = None
    elif form == "strided":
        wide = torch.zeros((apply.shape[0], 2 * apply.shape[1]), dtype=torch.int32).cuda()
        wide[:, ::2] = _cuda(apply)
        wide[:, 1::2] = 1 - _cuda(apply)                      # (what a kernel that ignored the strides would read)
        d_apply = wide[:, ::2]
        assert not d_apply.is_contiguous()
    else:
        d_apply = _cuda(apply).to(getattr(torch, form))
    out = _gridpp().neighbourhood_search(_cuda(array), _cuda(search), *K.SEARCH_ROWS[row], d_apply)
    assert out.is_cuda
    assert_array_equal(out.cpu().numpy(), K.search_reference(row, form != "none"))


# ---- fill, doping_circle, doping_square -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid(kind):
    lats, lons, elev, ct = K.grid_arrays(kind)
    return _gridpp().Grid(lats, lons, elev, np.zeros_like(elev), ct)


def _scatter(name, op, device=False):
    gridpp = _gridpp()
    c = K.scatter_cases()[name]
    ct = K.grid_arrays(c["grid"])[3]
    pts = gridpp.Points(c["lat"], c["lon"], c["elev"], np.zeros_like(c["elev"]), ct)
    bg, obs = K.background(c["grid"]), c["obs"]
    if device:
        bg, obs = _cuda(bg), _cuda(obs)
    if op == "fill_in":
        out = gridpp.fill(_grid(c["grid"]), bg, pts, c["radii"], K.FILL_VALUE, False)
    elif op == "fill_out":
        out = gridpp.fill(_grid(c["grid"]), bg, pts, c["radii"], K.FILL_VALUE, True)
    elif op == "circle":
        out = gridpp.doping_circle(_grid(c["grid"]), bg, pts, obs, c["radii"], c["med"])
    else:
        out = gridpp.doping_square(_grid(c["grid"]), bg, pts, obs, c["hw"], c["med"])
    return out.cpu().numpy() if device else np.asarray(out)


@pytest.mark.parametrize("name", sorted(K.scatter_cases()))
def test_scatter_matches_oracle(name):
    for op in K.scatter_cases()[name]["ops"]:
        ref = K.scatter_reference(name, op)
        assert_array_equal(_scatter(name, op), ref, err_msg=op)
        assert_array_equal(_scatter(name, op, device=True), ref, err_msg=op + " (device-resident fields)")


@pytest.mark.parametrize("name", sorted(K.expected_hits()))
def test_hit_sets(name):
    """radii exactly on the strict box and exactly on the distance, clamped bins, radii that reach everything or nothing, no points"""
    want = K.expected_hits()[name]
    for op in ("fill_in", "fill_out", "circle"):
        assert K.hit_set(name, _scatter(name, op), op) == want, op


@pytest.mark.parametrize("name", ["no_points", "geo_no_points"])
def test_no_points(name):
    bg = K.background(K.scatter_cases()[name]["grid"])
    for op in ("fill_in", "circle", "square"):
        assert_array_equal(_scatter(name, op), bg, err_msg=op)
    assert_array_equal(_scatter(name, "fill_out"), np.full_like(bg, K.FILL_VALUE))


def test_elevation_rule_hand_placed_cells():
    """a NaN elevation difference does not skip (doping.cpp:83-87), `>` keeps a difference equal to max_elev_diff"""
    bg = K.background("cart")
    circle, square = _scatter("elev_circle", "circle"), _scatter("elev_square", "square")
    for out in (circle, square):
        assert out[4, 4] == 7 and out[4, 5] == 8 and out[15, 21] == 10 and out[0, 0] == 11
        assert out[16, 21] == bg[16, 21] and out[10, 12] == 12
    assert circle[15, 20] == 9 and square[15, 20] == 10 and circle[9, 12] == bg[9, 12]
    for name, op in (("elev_zero_circle", "circle"), ("elev_zero_square", "square")):
        out = _scatter(name, op)
        assert out[10, 12] == 7 and out[5, 5] == bg[5, 5] and K.hit_set(name, out, op) == [K.node(10, 12)]


def test_doping_square_known_answers():
    bg = K.background("cart")
    out = _scatter("square_hw0", "square")
    assert K.hit_set("square_hw0", out, "square") == [K.node(2, 7), K.node(10, 12)] and out[10, 12] == 0 and out[2, 7] == 1
    assert_array_equal(_scatter("square_covers_all", "square"), np.zeros_like(bg))
    assert_array_equal(_scatter("square_huge_hw", "square"), np.ones_like(bg))
    out = _scatter("square_shared_cell", "square")
    assert out[10, 12] == 1 and out[9, 11] == 1 and out[8, 10] == 0 and out[12, 14] == 0 and out[2, 7] == 2      # the higher index wins
    far = _scatter("square_far_outside", "square")
    assert far[0, 0] == 4 and far[0, 24] == 5 and far[19, 0] == 6 and far[19, 24] == 7 and far[3, 3] == bg[3, 3]
